"""The detail-preserving restore on the CPU: the structured operand sets do what they are for; the torch emulation of the kernels
(``tests/cpu_restore_detail_emulation.py``) against the definition (``tests/detail_spec.py``) byte for byte on the GPU test's shapes; the
three consequences the header states; the premise of the identity property (a constant 255 resamples to 255) and the property itself through
the geometry; the configuration keys; the header and the binding; and the edit runner with ``source_restore_detail`` on the op emulation.
No GPU."""
import ctypes
import logging
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

import cpu_restore_detail_emulation as demu
import cpu_restore_emulation as remu
import detail_spec as ds
import restore_spec as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTERS = ["box", "bilinear", "bicubic", "lanczos"]
GATE_CASES = ("crop-right", "down", "identity", "crop-tall")      # 16 x 16, 64 x 64, 24 x 16 and 16 x 16 frames


def tt(a):
    return torch.from_numpy(np.array(a, copy=True))


# ------------------------------------------------------------------------------------------------ the operand sets
@pytest.mark.parametrize("case", list(rs.CASES))
def test_the_structured_sets_do_what_they_are_for(case):
    _, _, dest, box = rs.CASES[case]
    assert (ds.expected_gate(case, "equal") == 255).all()
    values = set(np.unique(ds.expected_gate(case, "ramp")).tolist())
    assert {0, 255} <= values and len(values - {0, 255}) >= 8, sorted(values)
    # random bytes alone close the gate (which is why the sets exist)
    S, E = rs.operands(case)
    assert (ds.gate(E[0], ds.prepared(case)[0]) == 0).all()
    # under an open gate ``e + add`` leaves [0, 255] at both ends
    E, P = ds.structured(case, "clamp")
    low = high = 0
    for f in range(2):
        d, e, p, g, _ = ds.terms(S[f], E[f], P[f], np.full(E.shape[1:3], 255, dtype=np.uint8), dest, box, "lanczos")
        assert (g == 255).all()
        v = e + (((d - p) * 256 + 128) >> 8)
        low, high = low + int((v < 0).sum()), high + int((v > 255).sum())
    assert low > 0 and high > 0, (low, high)


# ------------------------------------------------------------------------------------------------ the emulation against the definition
@pytest.mark.parametrize("kind", ds.SETS)
@pytest.mark.parametrize("case", GATE_CASES)
def test_gate_emulation_equals_the_definition(case, kind):
    E, P = ds.structured(case, kind)
    for radius in ds.RADII:
        for lo, hi in ds.THRESHOLDS:
            want = ds.expected_gate(case, kind, lo, hi, radius)
            got = demu.detail_gate_u8(tt(E), tt(P), lo, hi, radius)
            assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), want), (radius, lo, hi, int((got.numpy() != want).sum()))


def test_gate_values_by_hand():
    """One changed pixel of 90 in a flat frame, radius 1, lo = 2, hi = 12: the 3 x 3 mean around it is (90 + 4) // 9 = 10, the ramp there
    (255 * 2 + 5) // 10 = 51; at radius 0 the pixel itself is 90 >= hi."""
    P = np.full((1, 7, 7, 3), 100, dtype=np.uint8)
    E = P.copy()
    E[0, 3, 3, 1] = 10
    want = np.full((7, 7), 255, dtype=np.uint8)
    want[2:5, 2:5] = 51
    assert np.array_equal(ds.gate(E[0], P[0], 2, 12, 1), want)
    assert np.array_equal(demu.detail_gate_u8(tt(E), tt(P), 2, 12, 1)[0].numpy(), want)
    assert ds.gate(E[0], P[0], 2, 12, 0)[3, 3] == 0 and int((ds.gate(E[0], P[0], 2, 12, 0) == 255).sum()) == 48
    # a corner: the clamped window counts the corner pixel four times at radius 1 -> (4 * 90 + 4) // 9 = 40 >= hi
    E = P.copy()
    E[0, 0, 0, 0] = 190
    g = ds.gate(E[0], P[0], 2, 12, 1)
    assert g[0, 0] == 0 and g[1, 1] == 51 and g[0, 1] == 0 and g[2, 2] == 255          # (0, 1): twice in the window, 180 // 9 = 20


@pytest.mark.parametrize("case", list(rs.CASES))
def test_paste_emulation_equals_the_definition(case):
    """Random operands under a random gate on every shape of the GPU test, every filter, with and without alpha, gate and alpha with one
    frame and with F; the structured sets under the gate made from them."""
    _, (w, h), dest, box = rs.CASES[case]
    S, E = rs.operands(case)
    P = ds.prepared(case)
    for name in FILTERS:
        for kind, aframes, gframes in ((None, 1, 2), ("random", 1, 1), ("random", 2, 2), ("step", 2, 1)):
            want = ds.expected(case, name, kind, aframes, gframes)
            A = None if kind is None else rs.alpha(kind, h, w, aframes)
            got = demu.restore_detail_u8(tt(E), tt(P), tt(ds.random_gate(case, gframes)), tt(S), dest, box, name, None if A is None else tt(A))
            assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), want), (name, kind, aframes, gframes, int((got.numpy() != want).sum()))
    for kind in ("ramp", "clamp"):
        E2, P2 = ds.structured(case, kind)
        G = ds.expected_gate(case, kind, 254, 255, 1) if kind == "clamp" else ds.expected_gate(case, kind)
        want = np.stack([ds.restore_detail(S[f], E2[f], P2[f], G[f], dest, box, "lanczos") for f in range(2)])
        got = demu.restore_detail_u8(tt(E2), tt(P2), tt(G), tt(S), dest, box, "lanczos")
        assert np.array_equal(got.numpy(), want), (kind, int((got.numpy() != want).sum()))


# ------------------------------------------------------------------------------------------------ the consequences
@pytest.mark.parametrize("case", list(rs.CASES))
def test_the_three_consequences(case):
    _, (w, h), dest, box = rs.CASES[case]
    S, E = rs.operands(case)
    P = ds.prepared(case)
    zero, full = np.zeros((1, h, w), dtype=np.uint8), np.full((1, h, w), 255, dtype=np.uint8)
    for name in FILTERS:
        for kind in (None, "random"):
            # g = 0: today's paste, and so Pillow
            A = None if kind is None else rs.alpha(kind, h, w, 1)
            got = demu.restore_detail_u8(tt(E), tt(P), tt(zero), tt(S), dest, box, name, None if A is None else tt(A))
            assert np.array_equal(got.numpy(), rs.expected(case, name, kind, 1)), (name, kind)
            assert np.array_equal(np.stack([ds.restore_detail(S[f], E[f], P[f], zero[0], dest, box, name, None if A is None else A[0])
                                            for f in range(2)]), rs.expected(case, name, kind, 1))
            # g = 255 with e = p: the source
            got = demu.restore_detail_u8(tt(P), tt(P), tt(full), tt(S), dest, box, name, None if A is None else tt(A))
            assert np.array_equal(got.numpy(), S), (name, kind)
        # m = 0: the source, whatever the gate
        got = demu.restore_detail_u8(tt(E), tt(P), tt(ds.random_gate(case)), tt(S), dest, box, name, tt(zero))
        assert np.array_equal(got.numpy(), S), name


@pytest.mark.parametrize("case", list(rs.CASES))
def test_a_constant_255_resamples_to_255_in_both_passes(case):
    """The premise of the identity property: the gate of an unchanged edit is 255 everywhere, and it must arrive as 255 (weight 256) at
    every byte of dest.  Bilinear, as the gate is resampled; and every other filter, for good measure."""
    from anyv2v_amd import ops
    _, (w, h), dest, box = rs.CASES[case]
    full = torch.full((1, h, w, 1), 255, dtype=torch.uint8)
    for name in FILTERS:
        for row0, rows, hp, vp in ops.restore_passes(h, w, dest, box, name):
            x = full[:, row0:row0 + rows]
            x = x if hp is None else remu._one_pass(x, 2, hp)
            assert int(x.min()) == 255, (name, "horizontal")
            assert int(remu._one_pass(x, 1, vp).min()) == 255, (name, "vertical")


# ------------------------------------------------------------------------------------------------ the identity, through the geometry
@pytest.mark.parametrize("fit,xo,yo", [("crop", -1, 0.37), ("crop", 1, -1), ("stretch", 0.0, 0.0)])
def test_an_edit_that_changes_nothing_restores_the_source(monkeypatch, fit, xo, yo):
    demu.install(monkeypatch)
    from anyv2v_amd import prepare
    S = tt(rs.operands("crop-right")[0])                                        # [2, 37, 53, 3]
    P = prepare.prepare_frames(S, 16, 16, fit, xo, yo, device="cpu")
    alpha = torch.from_numpy(np.random.default_rng(5).random((2, 16, 16), dtype=np.float32))
    for a in (None, alpha):
        got = prepare.restore_frames_detail(P, S, prepared=P, fit=fit, x_offset=xo, y_offset=yo, alpha=a, device="cpu")
        assert got.dtype == torch.uint8 and torch.equal(got, S)
        # ``prepared=None``: prepared on the spot, the same frames; PIL images in
        pil = prepare.restore_frames_detail([Image.fromarray(f) for f in P.numpy()], [Image.fromarray(f) for f in S.numpy()], fit=fit,
                                            x_offset=xo, y_offset=yo, alpha=a, device="cpu")
        assert torch.equal(pil, S)
    # and an edit that does change something is not the source, nor the plain restore (the detail arrives where the gate is open)
    E = P.clone()
    E[:, :8] = 255 - E[:, :8]
    got = prepare.restore_frames_detail(E, S, prepared=P, fit=fit, x_offset=xo, y_offset=yo, device="cpu")
    plain = prepare.restore_frames(E, S, fit, xo, yo, device="cpu")
    assert not torch.equal(got, S) and not torch.equal(got, plain)


def test_restore_frames_detail_refuses_bad_arguments(monkeypatch):
    demu.install(monkeypatch)
    from anyv2v_amd import prepare
    S, E = (tt(x) for x in rs.operands("crop-right"))
    P = tt(ds.prepared("crop-right"))
    ok = dict(fit="crop", x_offset=1, y_offset=-1, device="cpu")
    prepare.restore_frames_detail(E, S, P, **ok)
    for kw, word in [(dict(prepared=P[:, :8]), "prepared"), (dict(prepared=P[:1]), "prepared"), (dict(gate_lo=32), "lo"), (dict(gate_hi=256), "hi"),
                     (dict(gate_lo=1.5), "lo"), (dict(gate_radius=17), "radius"), (dict(gate_radius=-1), "radius"), (dict(gate_radius=True), "radius"),
                     (dict(alpha=torch.zeros(3, 16, 16)), "alpha"), (dict(alpha=torch.full((1, 16, 16), 2.0)), "alpha"),
                     (dict(prepared=None, source_resample="nearest"), "resample"), (dict(resample="nearest"), "resample")]:
        with pytest.raises(ValueError, match=word):
            prepare.restore_frames_detail(E, S, **dict(dict(ok, prepared=P), **kw))
    with pytest.raises(ValueError, match="source frames"):
        prepare.restore_frames_detail(E, S[:1], P, **ok)


def test_the_pipeline_method_is_refused_on_frame_parallel_clips():
    from anyv2v_amd.pipeline import I2VGenXLPipeline

    class Unet:
        frame_parallel = object()
    pipe = I2VGenXLPipeline.__new__(I2VGenXLPipeline)
    pipe.unet = Unet()
    with pytest.raises(NotImplementedError, match="frame-parallel"):
        pipe.restore_frames_detail(None, None)
    with pytest.raises(NotImplementedError, match="frame-parallel"):
        pipe.restore_frames(None, None)


# ------------------------------------------------------------------------------------------------ the configuration keys, header, binding
def test_plan_from_config_reads_the_detail_keys():
    from anyv2v_amd.config import OmegaConf
    from anyv2v_amd.prepare import PreparePlan, plan_from_config
    c = OmegaConf.create
    on = {"source_fit": "crop", "source_restore": True}
    # absent: the plan is what it was
    p = plan_from_config(c(on))
    assert p == PreparePlan("crop", restore=True) == PreparePlan("crop", 0.0, 0.0, "lanczos", None, True, "lanczos") and p.tag() == "_restored"
    assert (p.restore_detail, p.detail_lo, p.detail_hi, p.detail_radius) == (False, 8, 32, 2)
    assert plan_from_config(c(dict(on, source_restore_detail=False))) == p
    assert plan_from_config(c({"source_fit": "crop"})) == PreparePlan("crop")
    p = plan_from_config(c(dict(on, source_restore_detail=True)))
    assert p == PreparePlan("crop", restore=True, restore_detail=True) and p.tag() == "_restored_detail"
    p = plan_from_config(c(dict(on, source_restore_resample="bicubic", source_restore_detail=True, source_restore_detail_lo=4,
                                source_restore_detail_hi=16, source_restore_detail_radius=0)))
    assert (p.restore_detail, p.detail_lo, p.detail_hi, p.detail_radius) == (True, 4, 16, 0) and p.tag() == "_restored-bicubic_detail-4-16-0"
    assert plan_from_config(c(dict(on, source_restore_detail=True, source_restore_detail_radius=16))).tag() == "_restored_detail-8-32-16"
    assert plan_from_config(c(dict(on, source_restore_detail=True, source_restore_detail_lo=8, source_restore_detail_hi=32,
                                   source_restore_detail_radius=2))).tag() == "_restored_detail"
    assert PreparePlan("crop", restore_detail=True).tag() == ""                      # (the tag follows the switch of the way back)
    # ``api``: the fit in one configuration, the way back in the other
    p = plan_from_config(c({"source_fit": "crop"}), restore_config=c({"source_restore": True, "source_restore_detail": True,
                                                                      "source_restore_detail_hi": 64}))
    assert p.restore and p.restore_detail and p.detail_hi == 64
    assert plan_from_config(c({"source_fit": "crop"}), restore_config=c({"target_fps": 8})) == PreparePlan("crop")
    with pytest.raises(ValueError, match="source_restore_detail without source_restore"):
        plan_from_config(c({"source_fit": "crop", "source_restore": True}), restore_config=c({"source_restore_detail": True}))
    for bad, key in [({"source_fit": "crop", "source_restore_detail": True}, "source_restore_detail without source_restore"),
                     ({"source_fit": "crop", "source_restore": False, "source_restore_detail": True}, "source_restore_detail without source_restore"),
                     ({"source_restore_detail": True}, "source_restore_detail without source_restore"),
                     (dict(on, source_restore_detail_lo=4), "source_restore_detail_lo without source_restore_detail"),
                     (dict(on, source_restore_detail=False, source_restore_detail_hi=40), "source_restore_detail_hi without"),
                     (dict(on, source_restore_detail_radius=1), "source_restore_detail_radius without"),
                     ({"source_fit": "crop", "source_restore_detail_radius": 1}, "source_restore_detail_radius without"),
                     (dict(on, source_restore_detail="yes"), "source_restore_detail="), (dict(on, source_restore_detail=1), "source_restore_detail="),
                     (dict(on, source_restore_detail=True, source_restore_detail_lo=4.5), "source_restore_detail_lo="),
                     (dict(on, source_restore_detail=True, source_restore_detail_lo=True), "source_restore_detail_lo="),
                     (dict(on, source_restore_detail=True, source_restore_detail_hi="32"), "source_restore_detail_hi="),
                     (dict(on, source_restore_detail=True, source_restore_detail_radius=2.0), "source_restore_detail_radius="),
                     (dict(on, source_restore_detail=True, source_restore_detail_lo=-1), "lo < hi"),
                     (dict(on, source_restore_detail=True, source_restore_detail_hi=256), "lo < hi"),
                     (dict(on, source_restore_detail=True, source_restore_detail_lo=32), "lo < hi"),
                     (dict(on, source_restore_detail=True, source_restore_detail_lo=40, source_restore_detail_hi=39), "lo < hi"),
                     (dict(on, source_restore_detail=True, source_restore_detail_radius=17), "radius"),
                     (dict(on, source_restore_detail=True, source_restore_detail_radius=-1), "radius")]:
        with pytest.raises(ValueError, match=key):
            plan_from_config(c(bad))


def test_output_suffix_carries_the_detail_tag_only_with_the_switch():
    from anyv2v_amd.config import OmegaConf
    from anyv2v_amd.run_group_pnp_edit import output_suffix
    base = {"n_steps": 50, "cfg": 9.0, "pnp_f_t": 0.2, "pnp_spatial_attn_t": 0.2, "pnp_temp_attn_t": 0.5, "source_fit": "crop", "source_restore": True}
    plain = "ddim_init_latents_t_idx_0_nsteps_50_cfg_9.0_pnpf0.2_pnps0.2_pnpt0.5_restored"
    assert output_suffix(OmegaConf.create(base), 0) == plain
    assert output_suffix(OmegaConf.create(dict(base, source_restore_detail=True)), 0) == plain + "_detail"
    assert output_suffix(OmegaConf.create(dict(base, source_restore_detail=True, source_restore_detail_lo=0)), 0) == plain + "_detail-0-32-2"


def test_the_header_declares_the_entry_points_and_the_binding_mirrors_them():
    from anyv2v_amd import _lib
    assert _lib.ABI_VERSION == 105 and _lib.load().anyv2v_version() == 105
    with open(os.path.join(ROOT, "include", "anyv2v_hip.h")) as f:
        header = f.read()
    assert "#define ANYV2V_ABI_VERSION 105" in header and "#define ANYV2V_DETAIL_MAX_RADIUS 16" in header and _lib.DETAIL_MAX_RADIUS == 16
    ctype = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "const int32_t*": ctypes.c_void_p, "int32_t": ctypes.c_int32,
             "int64_t": ctypes.c_int64}
    for name, count in (("anyv2v_detail_gate_u8", 12), ("anyv2v_restore_detail_u8", 24)):
        m = re.search(r"\nint %s\(([^;]*)\);" % name, header)
        assert m, f"the header does not declare {name}"
        declared = [ctype[" ".join(a.split()[:-1])] for a in " ".join(m.group(1).split()).split(", ")]
        res, args = _lib.SYMBOLS[name]
        assert res is ctypes.c_int and args == declared and len(args) == count, name
        assert hasattr(_lib.load(), name)
    for line in ("wt = g + (g >> 7)", "add = ((d - p) * wt + 128) >> 8", "e2 = clamp(e + add, 0, 255)", "t = d * (255 - m) + e2 * m + 128",
                 "mean = (b + n / 2) / n", "G = (255 * (hi - mean) + (hi - lo) / 2) / (hi - lo)"):
        assert line in header, line
    assert re.search(r"anyv2v_detail_gate_u8 and anyv2v_restore_detail_u8 after them: new entry\s+\* points", header)
    with open(os.path.join(ROOT, "anyv2v_amd", "csrc", "Makefile")) as f:
        assert "restore_detail.hip" in f.read()


def test_the_entry_points_refuse_bad_arguments_before_any_launch():
    """Every refusal is decided on the host: no GPU is needed to see it."""
    from anyv2v_amd import _lib
    lib = _lib.load()
    M = 1 << 20
    good = dict(edit=1 * M, prepared=2 * M, gate_out=3 * M, F=2, h=12, w=10, lo=8, hi=32, radius=2, scratch=4 * M, scratch_bytes=480, stream=None)
    for change, word in [(dict(lo=32), "lo"), (dict(lo=-1), "lo"), (dict(hi=256), "hi"), (dict(lo=40, hi=39), "lo"), (dict(radius=17), "radius"),
                         (dict(radius=-1), "radius"), (dict(edit=None), "null"), (dict(scratch=None), "null"), (dict(F=0), "F ="),
                         (dict(h=0), "h x w"), (dict(w=16385), "h x w"), (dict(scratch_bytes=479), "scratch"), (dict(scratch=4 * M + 1), "aligned"),
                         (dict(gate_out=1 * M + 700), "overlap"), (dict(gate_out=4 * M + 100), "overlap"), (dict(scratch=2 * M - 2), "overlap")]:
        assert lib.anyv2v_detail_gate_u8(*dict(good, **change).values()) < 0, change
        msg = lib.anyv2v_last_error().decode()
        assert word in msg and "detail_gate" in msg, (change, msg)
    good = dict(source=4096, edit_h=1 * M, prep_h=2 * M, gate_h=3 * M, alpha_h=4 * M, out=5 * M, F=2, sh=12, sw=10, dx0=2, dy0=3, dx1=8, dy1=8,
                e_rows=4, e_bounds=6 * M, e_coeffs=7 * M, e_ksize=3, gate_frames=2, mask_frames=2, a_rows=4, a_bounds=8 * M, a_coeffs=9 * M, a_ksize=3,
                stream=None)
    for change, word in [(dict(dx1=11), "dest"), (dict(dx1=2), "dest"), (dict(dy0=8), "dest"), (dict(dy0=-1), "dest"),
                         (dict(out=4096 + 100), "overlap"), (dict(out=2 * M - 8), "overlap"), (dict(out=3 * M - 8), "overlap"),
                         (dict(out=4 * M - 8), "overlap"), (dict(out=7 * M - 8), "overlap"), (dict(out=8 * M), "overlap"),
                         (dict(mask_frames=3), "mask_frames"), (dict(gate_frames=3), "gate_frames"), (dict(gate_frames=0), "gate_frames"),
                         (dict(source=None), "null"), (dict(prep_h=None), "null"), (dict(gate_h=None), "null"), (dict(a_bounds=None), "null"),
                         (dict(e_coeffs=None), "null"), (dict(sh=0), "sh x sw"), (dict(F=65536), "F ="), (dict(e_ksize=0), "ksize"),
                         (dict(a_rows=-1), "rows"), (dict(a_coeffs=9 * M + 1), "aligned"), (dict(e_bounds=6 * M + 2), "aligned")]:
        assert lib.anyv2v_restore_detail_u8(*dict(good, **change).values()) < 0, change
        msg = lib.anyv2v_last_error().decode()
        assert word in msg and "restore_detail" in msg, (change, msg)


# ------------------------------------------------------------------------------------------------ the runner, on the op emulation
SRC_W, SRC_H, SIZE, N_FRAMES, N_STEPS = 96, 64, 32, 2, 2


def test_edit_runner_writes_a_detail_directory_and_the_plain_restore_is_unchanged(tmp_path, monkeypatch):
    """Inversion and edit of a 96 x 64 clip at 32 x 32: with ``source_restore_detail`` the PNGs land in ``.._restored_detail`` and equal the
    definition on what the same entry writes at the working size; without the key the entry writes the bytes it wrote before the key
    existed -- Pillow's paste of those frames."""
    import cpu_ops_emulation as oemu
    import test_runners_e2e as e2e
    oemu.install()
    demu.install(monkeypatch)
    monkeypatch.setenv("ANYV2V_NO_GRAPH", "1")
    from anyv2v_amd import prepare, run_group_ddim_inversion as s1, run_group_pnp_edit as s2
    from anyv2v_amd.utils import seed_everything, wait_for_pending_writes
    base = e2e._make_workspace(tmp_path)
    clip = os.path.join(base, "demo", "wide")
    os.makedirs(clip, exist_ok=True)
    rng = np.random.default_rng(17)
    frames = [rng.integers(0, 256, (SRC_H, SRC_W, 3), dtype=np.uint8) for _ in range(N_FRAMES)]
    for i, a in enumerate(frames):
        Image.fromarray(a).save(os.path.join(clip, f"{i:05d}.png"))
    torch.set_grad_enabled(False)
    log = logging.getLogger("restore-detail")
    inv, _, ed, ed_list = e2e._configs(base, "restore")
    for c in (inv, ed):
        c.device, c.image_size, c.n_frames = "cpu", [SIZE, SIZE], N_FRAMES
    inv.inverse_config.n_steps = ed.n_steps = N_STEPS
    fit = dict(source_fit="crop", source_x_offset=0.37)
    seed_everything(inv.seed)
    s1.main(inv, [dict({"active": True, "force_recompute_latents": False, "video_name": "wide", "recon_config": {"enable_recon": False}}, **fit)],
            torch.device("cpu"), log, synthetic_encoders=True)
    wait_for_pending_writes()
    entry = dict(ed_list[0], video_name="wide", **fit)
    # a gate that is open somewhere for the random mini checkpoint's output: the thresholds at the top of the range
    tuned = {"source_restore": True, "source_restore_detail": True, "source_restore_detail_lo": 200, "source_restore_detail_hi": 255,
             "source_restore_detail_radius": 1}
    for extra in ({}, {"source_restore": True}, {"source_restore": True, "source_restore_detail": True}, tuned):
        seed_everything(ed.seed)
        s2.main(ed, [dict(entry, **extra)], torch.device("cpu"), log, synthetic_encoders=True)
    root = os.path.join(base, "Results", "Prompt-Based-Editing", "mini-restore", "wide", "robot")
    plain, = [d for d in os.listdir(root) if "_restored" not in d]
    assert sorted(d[len(plain):] for d in os.listdir(root)) == ["", "_restored", "_restored_detail", "_restored_detail-200-255-1"]
    dest, box = prepare.restore_geometry((SRC_W, SRC_H), (SIZE, SIZE), "crop", 0.37, 0.0)
    P = prepare.prepare_frames(torch.from_numpy(np.stack(frames)), SIZE, SIZE, "crop", 0.37, 0.0, device="cpu").numpy()
    opened = 0
    for i in range(N_FRAMES):
        small = np.asarray(Image.open(os.path.join(root, plain, f"video_{i:05d}.png")))
        load = lambda tag: np.asarray(Image.open(os.path.join(root, plain + tag, f"video_{i:05d}.png")))
        assert small.shape == (SIZE, SIZE, 3)
        assert np.array_equal(load("_restored"), rs.pillow_restore(frames[i], small, dest, box, "lanczos")), f"_restored frame {i}"
        for tag, (lo, hi, radius) in (("_restored_detail", (8, 32, 2)), ("_restored_detail-200-255-1", (200, 255, 1))):
            G = ds.gate(small, P[i], lo, hi, radius)
            opened += int((G > 0).sum()) if lo == 200 else 0
            want = ds.restore_detail(frames[i], small, P[i], G, dest, box, "lanczos")
            got = load(tag)
            assert got.shape == (SRC_H, SRC_W, 3) and np.array_equal(got, want), f"{tag} frame {i}: {int((got != want).sum())} bytes differ"
    assert opened > 0, "the tuned gate never opened: the detail directory shows nothing the plain one does not"
    assert Image.open(os.path.join(root, plain + "_restored_detail", "video.gif")).size == (SRC_W, SRC_H)
