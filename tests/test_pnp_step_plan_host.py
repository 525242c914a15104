"""Which engine runs every step of ``sample_with_pnp``, under which graph key and at which timestep -- recorded by a spy on
``_StepEngine._step`` from the mini pipeline under the CPU op emulation, and compared with a plan this file derives from the three
injection schedules alone:

  * no site on                          -> the [negative, editing] twin (``nosrc``), key ``("pnp-nosrc",)``;
  * a site on, no source cache          -> the three-branch engine, key ``("pnp",) + state``;
  * a site on, cache on, first edit     -> the three-branch engine, key ``("pnp-record",) + state``;
  * a site on, cache on, further edits  -> the twin, key ``("pnp-replay",) + state``;
  * ``ANYV2V_SRC_SKIP=0``               -> every step on the three-branch engine, key ``("pnp",) + state``, and no twin at all.

``state`` = (conv, 8 x spatial attention, 8 x temporal attention), each "this step's timestep is in that schedule".  The twin is bound
(built or re-pointed) once per call that needs it and is one object for the life of the three-branch engine."""
import types

import pytest
import torch

import cpu_sampler_emulation as semu
import gpu_checks as gc

FR, HW_, STEPS = 4, 8, 6
ALL_ON, EARLY_END = (0.5, 0.75, 1.0), (0.25, 0.25, 0.5)     # (conv, spatial, temporal) shares of the steps; EARLY_END leaves source-free steps


@pytest.fixture()
def cpu_ops(monkeypatch):
    semu.install(monkeypatch)
    monkeypatch.setattr(gc, "DEV", "cpu")
    monkeypatch.setenv("ANYV2V_NO_GRAPH", "1")
    yield


def _clip():
    from anyv2v_amd.pipeline import I2VGenXLPipeline
    from anyv2v_amd.schedulers import DDIMInverseScheduler
    native, _, ocfg = gc.build_pair("mini", 1234)
    inp = gc.config1_inputs(ocfg, 3, FR, HW_)
    h = lambda x: x.half()
    c = types.SimpleNamespace(native=native, lat0=h(inp["sample"][:1]), ehs=h(inp["encoder_hidden_states"]), ie=h(inp["image_embeddings"]),
                              il=h(inp["image_latents"]))
    pipe = I2VGenXLPipeline(unet=native, scheduler=DDIMInverseScheduler())
    c.traj = pipe.invert(prompt_embeds=c.ehs[:1], image_embeddings=c.ie[:1], image_latents=c.il[:1], height=HW_ * 8, width=HW_ * 8,
                         num_frames=FR, num_inference_steps=STEPS, guidance_scale=1.0, target_fps=8, latents=c.lat0, return_trajectory=True)
    c.T = max(c.traj.keys())
    return c


def _timesteps():
    from anyv2v_amd.schedulers import DDIMScheduler
    sched = DDIMScheduler()
    sched.set_timesteps(STEPS)
    return sched, [int(t) for t in sched.timesteps]


def _edit(pipe, c, ratios):
    from anyv2v_amd import pnp_utils
    sched, _ = _timesteps()
    pipe.register_modules(scheduler=sched)
    k = lambda r: sched.timesteps[: int(STEPS * r)]
    pnp_utils.register_conv_injection(pipe, k(ratios[0]))
    pnp_utils.register_spatial_attention_pnp(pipe, k(ratios[1]))
    pnp_utils.register_temp_attention_pnp(pipe, k(ratios[2]))
    try:
        return pipe.sample_with_pnp(prompt_embeds=c.ehs[2:3], negative_prompt_embeds=c.ehs[1:2], image_embeddings=c.ie[2:3],
                                    image_latents=c.il[2:3], height=HW_ * 8, width=HW_ * 8, num_frames=FR, num_inference_steps=STEPS,
                                    guidance_scale=9.0, target_fps=8, latents=c.traj[c.T].clone(), output_type="latent",
                                    ddim_init_latents_t_idx=0, ddim_inv_latents_path=c.traj, ddim_inv_prompt_embeds=c.ehs[:1],
                                    ddim_inv_image_embeddings=c.ie[:1], ddim_inv_image_latents=c.il[:1]).frames.clone()
    finally:
        pnp_utils.clear_time(pipe)


def _plan(ratios, skip_src=True, cache=None):
    """[(engine, graph key, t)] by the rule in this file's docstring.  ``cache``: None, "record" (first edit) or "replay"."""
    _, ts = _timesteps()
    conv, spatial, temporal = (set(ts[: int(STEPS * r)]) for r in ratios)
    plan = []
    for t in ts:
        state = (t in conv,) + (t in spatial,) * 8 + (t in temporal,) * 8
        if not any(state) and skip_src:
            plan.append(("nosrc", ("pnp-nosrc",), t))
        elif cache is None or not any(state):
            plan.append(("three", ("pnp",) + state, t))
        elif cache == "record":
            plan.append(("three", ("pnp-record",) + state, t))
        else:
            plan.append(("nosrc", ("pnp-replay",) + state, t))
    return plan


class _Spy:
    """Wraps ``_StepEngine._step``, ``__init__`` and ``rebind``: the steps of one call, and how often a twin was built or re-pointed."""

    def __init__(self, monkeypatch):
        from anyv2v_amd.pipeline import _StepEngine
        self.steps, self.twin_binds, self.engines = [], 0, []
        step, init, rebind = _StepEngine._step, _StepEngine.__init__, _StepEngine.rebind
        spy = self

        def _step(eng, t_row, coef_row, key, noise=None, partner=None):
            step(eng, t_row, coef_row, key, noise, partner)
            spy.steps.append((eng, key, eng.ctx.t_buf.clone()))

        def _init(eng, pipe, sample, *a, **kw):
            init(eng, pipe, sample, *a, **kw)
            spy.twin_binds += sample.shape[0] == 2

        def _rebind(eng, sample_init, cond):
            ok = rebind(eng, sample_init, cond)
            spy.twin_binds += eng.sample.shape[0] == 2
            return ok
        monkeypatch.setattr(_StepEngine, "_step", _step)
        monkeypatch.setattr(_StepEngine, "__init__", _init)
        monkeypatch.setattr(_StepEngine, "rebind", _rebind)

    def take(self, pipe):
        """-> ([(engine kind, key, t_buf as a list)], twin binds) of the call that just ended, against the pipeline's cached PnP engine."""
        (eng,) = [e for k, e in pipe._engines.items() if k[0] in ("pnp", "pnp-droptail")]
        assert eng.sample.shape[0] == 3
        kinds = []
        for e, key, t_buf in self.steps:
            assert e is eng or e is eng.nosrc, "a step ran on an engine the pipeline does not hold"
            kinds.append(("three" if e is eng else "nosrc", key, t_buf.tolist()))
        binds, self.steps, self.twin_binds = self.twin_binds, [], 0
        return eng, kinds, binds


def _check(got, plan):
    width = {"three": 3, "nosrc": 2}
    assert [(k, key) for k, key, _ in got] == [(k, key) for k, key, _ in plan]
    assert [t_buf for _, _, t_buf in got] == [[float(t)] * width[k] for k, _, t in plan]      # ``t_buf`` after the copy: this step's timestep


@pytest.mark.parametrize("ratios,skip", [(ALL_ON, "1"), (EARLY_END, "1"), (EARLY_END, "0")],
                         ids=["no-source-free-step", "source-free-steps", "src-skip-off"])
def test_step_plan_without_the_source_cache(cpu_ops, monkeypatch, ratios, skip):
    monkeypatch.setenv("ANYV2V_SRC_SKIP", skip)
    c = _clip()
    from anyv2v_amd.pipeline import I2VGenXLPipeline
    from anyv2v_amd.schedulers import DDIMScheduler
    pipe = I2VGenXLPipeline(unet=c.native, scheduler=DDIMScheduler())
    spy = _Spy(monkeypatch)
    plan = _plan(ratios, skip_src=skip == "1")
    uses_twin = any(k == "nosrc" for k, _, _ in plan)
    assert uses_twin == (ratios == EARLY_END and skip == "1") and len(plan) == STEPS
    assert all(k == "three" for k, _, _ in plan) or skip == "1"
    twins, outs = [], []
    for _ in range(2):
        outs.append(_edit(pipe, c, ratios))
        eng, got, binds = spy.take(pipe)
        _check(got, plan)
        assert binds == int(uses_twin), "the [negative, editing] twin is bound once per call that runs a step on it"
        assert (eng.nosrc is not None) == uses_twin
        twins.append(eng.nosrc)
    assert twins[0] is twins[1] and torch.equal(outs[0], outs[1])
    assert pipe.source_cache is None


@pytest.mark.parametrize("ratios", [ALL_ON, EARLY_END], ids=["no-source-free-step", "source-free-steps"])
def test_step_plan_with_the_source_cache_across_two_calls(cpu_ops, monkeypatch, ratios):
    c = _clip()
    from anyv2v_amd.pipeline import I2VGenXLPipeline
    from anyv2v_amd.schedulers import DDIMScheduler
    pipe = I2VGenXLPipeline(unet=c.native, scheduler=DDIMScheduler())
    cache = pipe.enable_source_cache()
    spy = _Spy(monkeypatch)
    injected = sum(any(key[1:]) for _, key, _ in _plan(ratios))
    assert injected == int(STEPS * max(ratios)) > 0
    _edit(pipe, c, ratios)
    eng, got, binds = spy.take(pipe)
    _check(got, _plan(ratios, cache="record"))
    first_uses_twin = ratios == EARLY_END
    assert binds == int(first_uses_twin) and (eng.nosrc is not None) == first_uses_twin
    assert (cache.recorded_steps, cache.replayed_steps, cache.skipped_steps) == (injected, 0, 0)
    twin = eng.nosrc
    _edit(pipe, c, ratios)
    eng2, got, binds = spy.take(pipe)
    _check(got, _plan(ratios, cache="replay"))
    assert all(k == "nosrc" for k, _, _ in got)
    assert eng2 is eng and binds == 1 and eng.nosrc is not None and (twin is None or eng.nosrc is twin)
    assert (cache.recorded_steps, cache.replayed_steps) == (injected, injected)
    twin = eng.nosrc
    _edit(pipe, c, ratios)                       # a third edit replays again, on the same twin
    eng3, got, binds = spy.take(pipe)
    _check(got, _plan(ratios, cache="replay"))
    assert eng3 is eng and eng.nosrc is twin and binds == 1
    assert (cache.recorded_steps, cache.replayed_steps) == (injected, 2 * injected)
