"""The way back to the source's own size on the CPU: the invariants of ``prepare.restore_geometry`` in exact fractions over a grid; the
paste formula against Pillow over all 256^3 values; the definition (``tests/restore_spec.py``) and the torch emulation of the kernel
(``tests/cpu_restore_emulation.py``) against Pillow's ``paste(resize(.., box), xy, mask=resize(..))`` byte for byte on the GPU test's
shapes; the configuration keys; the header and the binding; and the edit runner with ``source_restore`` on the op emulation.  No GPU."""
import ctypes
import logging
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch
from PIL import Image

import restore_spec as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTERS = ["box", "bilinear", "bicubic", "lanczos"]


# ------------------------------------------------------------------------------------------------ the geometry
def test_restore_geometry_invariants_over_a_grid():
    from anyv2v_amd.prepare import restore_geometry
    checked = refused = 0
    for w, h in [(16, 16), (24, 16), (16, 24)]:
        for sw in range(8, 41):
            for sh in range(8, 41):
                assert restore_geometry((sw, sh), (w, h), "stretch") == ((0, 0, sw, sh), (0.0, 0.0, float(w), float(h)))
                for xo in (-1, 0, 0.37, 1):
                    for yo in (-1, 0, 0.37, 1):
                        fx0, fy0, fx1, fy1 = rs.footprint((sw, sh), (w, h), "crop", xo, yo)
                        try:
                            (dx0, dy0, dx1, dy1), box = restore_geometry((sw, sh), (w, h), "crop", xo, yo)
                        except ValueError as e:   # only where no whole pixel lies inside the footprint, and the message names the sizes
                            assert math.ceil(fx0) >= math.floor(fx1) or math.ceil(fy0) >= math.floor(fy1)
                            assert f"{sw} x {sh}" in str(e) and f"{w} x {h}" in str(e)
                            refused += 1
                            continue
                        checked += 1
                        assert 0 <= dx0 < dx1 <= sw and 0 <= dy0 < dy1 <= sh                              # inside the frame, non-empty
                        assert fx0 <= dx0 and dx1 <= fx1 and fy0 <= dy0 and dy1 <= fy1                    # inside the footprint
                        assert dx0 - 1 < fx0 and dx1 + 1 > fx1 and dy0 - 1 < fy0 and dy1 + 1 > fy1        # and the largest such
                        assert all(isinstance(v, float) for v in box)
                        assert 0.0 <= box[0] < box[2] <= w and 0.0 <= box[1] < box[3] <= h
                        # the pre-image of dest: box = (d - f) * (w / footprint width), one rounding away at the most
                        sx, sy = Fraction(w) / (fx1 - fx0), Fraction(h) / (fy1 - fy0)
                        exact = ((dx0 - fx0) * sx, (dy0 - fy0) * sy, (dx1 - fx0) * sx, (dy1 - fy0) * sy)
                        assert all(abs(Fraction(b) - e) <= Fraction(1, 1 << 40) for b, e in zip(box, exact)), (box, exact)
    assert checked > 40000 and refused == 0      # (a source of at least 8 x 8 under a window of at most 24 always holds a whole pixel)
    # a tiny source blown up to the working size: the footprint [1.5, 2.5] x [0, 1] holds no whole pixel
    with pytest.raises(ValueError, match="3 x 1 source.*64 x 64"):
        restore_geometry((3, 1), (64, 64), "crop", 0.5, 0.0)


def test_restore_geometry_of_the_full_hd_case():
    from anyv2v_amd.prepare import restore_geometry
    assert restore_geometry((1920, 1080), (512, 512), "crop") == ((420, 0, 1500, 1080), (0.0625, 0.0, 511.9375, 512.0))
    for args in [((0, 10), (8, 8), "crop"), ((10, 10), (8, 8), "cover"), ((10, 10), (8, 8), "crop", 1.5)]:
        with pytest.raises(ValueError):
            restore_geometry(*args)


# ------------------------------------------------------------------------------------------------ the definition against Pillow
def test_paste_formula_equals_pillow_for_every_byte_triple():
    """All (d, e, m) in L mode: d down the rows, e along the columns, one paste per m."""
    d = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 256, axis=1)
    e = np.ascontiguousarray(d.T)
    d64, e64 = d.astype(np.int64), e.astype(np.int64)
    src, edit = Image.fromarray(d, mode="L"), Image.fromarray(e, mode="L")
    for m in range(256):
        out = src.copy()
        out.paste(edit, (0, 0), mask=Image.new("L", (256, 256), m))
        assert np.array_equal(np.asarray(out), rs.paste_byte(d64, e64, m)), m
    assert np.array_equal(rs.paste_byte(d64, e64, 0), d64) and np.array_equal(rs.paste_byte(d64, e64, 255), e64)


@pytest.mark.parametrize("case", list(rs.CASES))
def test_spec_and_emulation_equal_pillow(case):
    """The numpy restatement and the torch emulation of the kernel on every shape of the GPU test, every filter, with and without alpha."""
    import cpu_restore_emulation as emu
    _, (w, h), dest, box = rs.CASES[case]
    S, E = rs.operands(case)
    for name in FILTERS:
        for kind, frames in ((None, 1), ("random", 1), ("random", 2), ("step", 2)):
            want = rs.expected(case, name, kind, frames)
            A = None if kind is None else rs.alpha(kind, h, w, frames)
            spec = np.stack([rs.restore(S[f], E[f], dest, box, name, None if A is None else A[f % frames]) for f in range(2)])
            assert np.array_equal(spec, want), (name, kind, frames, int((spec != want).sum()))
            got = emu.restore_u8(torch.from_numpy(E.copy()), torch.from_numpy(S.copy()), dest, box, name,
                                 None if A is None else torch.from_numpy(A.copy()))
            assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), want), (name, kind, frames, int((got.numpy() != want).sum()))


def test_alpha_zero_keeps_the_source_and_alpha_full_is_the_plain_paste():
    import cpu_restore_emulation as emu
    _, (w, h), dest, box = rs.CASES["crop-right"]
    S, E = (torch.from_numpy(x.copy()) for x in rs.operands("crop-right"))
    zero, full = (torch.from_numpy(rs.alpha(k, h, w).copy()) for k in ("zero", "full"))
    assert torch.equal(emu.restore_u8(E, S, dest, box, "lanczos", zero), S)
    assert torch.equal(emu.restore_u8(E, S, dest, box, "lanczos", full), emu.restore_u8(E, S, dest, box, "lanczos"))
    assert not torch.equal(emu.restore_u8(E, S, dest, box, "lanczos"), S)


def test_a_box_is_taken_as_pillow_takes_it():
    """A box that is no float: Pillow rounds its numbers to C floats and forms the width in float; the passes are planned for that box, and
    a far end that then passes the side by a rounding is not refused."""
    from anyv2v_amd import ops
    box = rs.CASES["crop-right"][3]
    assert box[0] != float(np.float32(box[0]))
    x0, _, x1, _ = rs.pillow_box(box)
    assert x0 == float(np.float32(box[0])) and x1 - x0 == float(np.float32(np.float32(box[2]) - np.float32(box[0])))
    (row0, rows, hp, vp), _ = ops.restore_passes(16, 16, rs.CASES["crop-right"][2], box, "lanczos")
    ksize, bounds, coeffs = ops.resample_table(16, x0, x1, 38, "lanczos")
    assert hp[0] == ksize and torch.equal(hp[1], bounds) and torch.equal(hp[2], coeffs)
    with pytest.raises(ValueError):
        ops.resample_table(16, 0.0, 16.001, 38, "lanczos")


def test_identity_tables_where_pillow_skips_a_pass():
    from anyv2v_amd import ops
    (row0, rows, hp, vp), (_, _, ahp, avp) = ops.restore_passes(16, 24, (0, 0, 24, 16), (0.0, 0.0, 24.0, 16.0), "lanczos")
    assert (row0, rows, hp, ahp) == (0, 16, None, None)
    for t in (vp, avp):
        assert t[0] == 1 and t[1].tolist() == [[i, 1] for i in range(16)] and t[2].tolist() == [[1 << 22]] * 16
        assert t[1].dtype == torch.int32 and t[2].dtype == torch.int32


# ------------------------------------------------------------------------------------------------ the configuration keys, header, binding
def test_plan_from_config_reads_the_restore_keys():
    from anyv2v_amd.config import OmegaConf
    from anyv2v_amd.prepare import PreparePlan, plan_from_config
    c = OmegaConf.create
    assert plan_from_config(c({"source_fit": "crop"})) == PreparePlan("crop") and PreparePlan("crop").restore is False
    assert PreparePlan("crop").tag() == ""
    p = plan_from_config(c({"source_fit": "crop", "source_restore": True}))
    assert p == PreparePlan("crop", restore=True, restore_resample="lanczos") and p.tag() == "_restored"
    p = plan_from_config(c({"source_fit": "stretch", "source_restore": True, "source_restore_resample": "bicubic"}))
    assert p.restore and p.restore_resample == "bicubic" and p.tag() == "_restored-bicubic"
    assert plan_from_config(c({"source_fit": "crop", "source_restore": False})) == PreparePlan("crop")
    # ``api``: the fit in one configuration, the way back in the other
    p = plan_from_config(c({"source_fit": "crop"}), restore_config=c({"source_restore": True, "source_restore_resample": "box"}))
    assert p.restore and p.restore_resample == "box"
    assert plan_from_config(c({"source_fit": "crop"}), restore_config=c({"target_fps": 8})) == PreparePlan("crop")
    assert plan_from_config(c({}), restore_config=c({})) is None
    for bad, key in [({"source_restore": True}, "source_restore without source_fit"),
                     ({"source_fit": "crop", "source_restore_resample": "box"}, "source_restore_resample without source_restore"),
                     ({"source_fit": "crop", "source_restore": False, "source_restore_resample": "box"}, "source_restore_resample without"),
                     ({"source_fit": "crop", "source_restore": True, "source_restore_resample": "nearest"}, "source_restore_resample="),
                     ({"source_fit": "crop", "source_restore": "yes"}, "source_restore="), ({"source_fit": "crop", "source_restore": 1}, "source_restore=")]:
        with pytest.raises(ValueError, match=key):
            plan_from_config(c(bad))
    with pytest.raises(ValueError, match="source_restore without source_fit"):
        plan_from_config(c({}), restore_config=c({"source_restore": True}))


def test_output_suffix_is_unchanged_without_the_key():
    from anyv2v_amd.config import OmegaConf
    from anyv2v_amd.run_group_pnp_edit import output_suffix
    base = {"n_steps": 50, "cfg": 9.0, "pnp_f_t": 0.2, "pnp_spatial_attn_t": 0.2, "pnp_temp_attn_t": 0.5}
    plain = "ddim_init_latents_t_idx_0_nsteps_50_cfg_9.0_pnpf0.2_pnps0.2_pnpt0.5"
    assert output_suffix(OmegaConf.create(base), 0) == plain
    assert output_suffix(OmegaConf.create(dict(base, source_fit="crop")), 0) == plain
    assert output_suffix(OmegaConf.create(dict(base, source_fit="crop", source_restore=True)), 0) == plain + "_restored"
    both = dict(base, source_fit="crop", source_restore=True, source_restore_resample="bilinear")
    assert output_suffix(OmegaConf.create(both), 0) == plain + "_restored-bilinear"


def test_the_header_declares_the_entry_point_and_the_binding_mirrors_it():
    from anyv2v_amd import _lib
    assert _lib.ABI_VERSION == 105 and _lib.load().anyv2v_version() == 105
    with open(os.path.join(ROOT, "include", "anyv2v_hip.h")) as f:
        header = f.read()
    assert "#define ANYV2V_ABI_VERSION 105" in header
    m = re.search(r"\nint anyv2v_restore_paste_u8\(([^;]*)\);", header)
    assert m, "the header does not declare anyv2v_restore_paste_u8"
    ctype = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "const int32_t*": ctypes.c_void_p, "int32_t": ctypes.c_int32}
    declared = [ctype[" ".join(a.split()[:-1])] for a in " ".join(m.group(1).split()).split(", ")]
    res, args = _lib.SYMBOLS["anyv2v_restore_paste_u8"]
    assert res is ctypes.c_int and args == declared and len(args) == 21
    assert "t = d * (255 - m) + e * m + 128" in header and "((t >> 8) + t) >> 8" in header          # the paste formula is documented
    assert re.search(r"anyv2v_restore_paste_u8 were added under 105", header)
    assert hasattr(_lib.load(), "anyv2v_restore_paste_u8")


def test_the_entry_point_refuses_bad_arguments_before_any_launch():
    """Every refusal is decided on the host: no GPU is needed to see it."""
    from anyv2v_amd import _lib
    lib = _lib.load()
    good = dict(source=4096, edit_h=1 << 20, alpha_h=2 << 20, out=3 << 20, F=2, sh=12, sw=10, dx0=2, dy0=3, dx1=8, dy1=8, e_rows=4, e_bounds=4 << 20,
                e_coeffs=5 << 20, e_ksize=3, mask_frames=2, a_rows=4, a_bounds=6 << 20, a_coeffs=7 << 20, a_ksize=3, stream=None)
    for change, word in [(dict(dx1=11), "dest"), (dict(dx1=2), "dest"), (dict(dy0=8), "dest"), (dict(out=4096 + 100), "overlap"),
                         (dict(out=(2 << 20) - 8), "overlap"), (dict(mask_frames=3), "mask_frames"), (dict(source=None), "null"),
                         (dict(a_bounds=None), "null"), (dict(sh=0), "sh x sw"), (dict(e_ksize=0), "ksize"), (dict(a_rows=-1), "rows"),
                         (dict(a_coeffs=(7 << 20) + 1), "aligned")]:
        assert lib.anyv2v_restore_paste_u8(*dict(good, **change).values()) < 0, change
        assert word in lib.anyv2v_last_error().decode(), (change, lib.anyv2v_last_error())


# ------------------------------------------------------------------------------------------------ the public surface on the emulation
def test_restore_frames_and_the_plan_on_the_emulation(monkeypatch):
    import cpu_restore_emulation as emu
    emu.install(monkeypatch)
    from anyv2v_amd import prepare
    S, E = rs.operands("crop-right")
    dest, box = prepare.restore_geometry((53, 37), (16, 16), "crop", 1, -1)
    assert (dest, box) == rs.CASES["crop-right"][2:]
    alpha = torch.from_numpy(np.random.default_rng(3).random((2, 16, 16), dtype=np.float32))
    A = np.rint(alpha.numpy() * 255.0).astype(np.uint8)
    want = np.stack([rs.pillow_restore(S[f], E[f], dest, box, "lanczos", A[f]) for f in range(2)])
    pil_e, pil_s = [Image.fromarray(e) for e in E], [Image.fromarray(s) for s in S]
    got = prepare.restore_frames(pil_e, pil_s, "crop", 1, -1, alpha=alpha, device="cpu")
    assert np.array_equal(got.numpy(), want)
    assert np.array_equal(prepare.restore_frames(pil_e, pil_s, "crop", 1, -1, device="cpu").numpy(), rs.expected("crop-right"))

    class Pipe:   # what ``PreparePlan.restored`` uses of a pipeline
        def restore_frames(self, edited, source_frames, **kw):
            return prepare.restore_frames(edited, source_frames, device="cpu", **kw)
    plan = prepare.PreparePlan("crop", 1.0, -1.0, restore=True)
    out = plan.restored(Pipe(), pil_e, pil_s, alpha, prepared_from=(53, 37))
    assert [f.size for f in out] == [(53, 37)] * 2 and np.array_equal(np.stack([np.asarray(f) for f in out]), want)
    with pytest.raises(ValueError, match="prepared from"):
        plan.restored(Pipe(), pil_e, pil_s, alpha, prepared_from=(54, 37))
    with pytest.raises(ValueError, match="source frames"):
        prepare.restore_frames(pil_e, pil_s[:1], device="cpu")
    with pytest.raises(ValueError, match="alpha"):
        prepare.restore_frames(pil_e, pil_s, alpha=alpha[:, :8], device="cpu")


def test_composite_alpha_is_what_composite_over_source_builds(monkeypatch):
    """``composite_over_source`` calls ``composite_alpha``'s arithmetic: the alpha handed to ``ops.composite`` is the method's result."""
    import cpu_restore_emulation as emu
    emu.install(monkeypatch)      # (every op emulation down to ``latent_mask`` / ``pixel_alpha`` / ``composite``)
    from anyv2v_amd import ops
    from anyv2v_amd.masked_edit import MaskedEditMixin

    class Pipe(MaskedEditMixin):
        unet, vae_scale_factor, _execution_device = None, 8, torch.device("cpu")
    seen = {}
    real = ops.composite
    monkeypatch.setattr(ops, "composite", lambda video, src, alpha, match_color=False, out=None: seen.setdefault("alpha", alpha) is None or real(video, src, alpha, match_color))
    mask = torch.zeros(1, 64, 64, dtype=torch.bool)
    mask[:, 8:16, 8:16] = True
    video = torch.zeros(1, 3, 2, 64, 64)
    src = torch.zeros(2, 64, 64, 3, dtype=torch.uint8)
    pipe = Pipe()
    pipe.composite_over_source(video, src, mask, grow=0, feather=0.5, grow_px=2, feather_px=1.5)
    alpha = pipe.composite_alpha(mask, grow=0, feather=0.5, grow_px=2, feather_px=1.5)
    assert alpha.dtype == torch.float32 and tuple(alpha.shape) == (1, 64, 64) and torch.equal(alpha, seen["alpha"].float())
    assert float(alpha.min()) == 0.0 and float(alpha.max()) == 1.0
    with pytest.raises(ValueError, match="grow_px"):
        pipe.composite_alpha(mask, grow_px=1000)


# ------------------------------------------------------------------------------------------------ the runner, on the op emulation
SRC_W, SRC_H, SIZE, N_FRAMES, N_STEPS = 96, 64, 32, 2, 2


def restore_clip():
    rng = np.random.default_rng(17)
    return [rng.integers(0, 256, (SRC_H, SRC_W, 3), dtype=np.uint8) for _ in range(N_FRAMES)]


def check_runner_restores(tmp_path, device):
    """Inversion and edit of a 96 x 64 clip at 32 x 32 with ``source_restore``: the PNGs are 96 x 64 and equal Pillow's paste of what the same
    entry writes without the key."""
    import test_runners_e2e as e2e
    from anyv2v_amd import run_group_ddim_inversion as s1, run_group_pnp_edit as s2
    from anyv2v_amd.prepare import restore_geometry
    from anyv2v_amd.utils import seed_everything, wait_for_pending_writes
    base = e2e._make_workspace(tmp_path)
    clip = os.path.join(base, "demo", "wide")
    os.makedirs(clip, exist_ok=True)
    frames = restore_clip()
    for i, a in enumerate(frames):
        Image.fromarray(a).save(os.path.join(clip, f"{i:05d}.png"))
    torch.set_grad_enabled(False)
    log = logging.getLogger("restore")
    inv, _, ed, ed_list = e2e._configs(base, "restore")
    for c in (inv, ed):
        c.device, c.image_size, c.n_frames = device, [SIZE, SIZE], N_FRAMES
    inv.inverse_config.n_steps = ed.n_steps = N_STEPS
    fit = dict(source_fit="crop", source_x_offset=0.37)
    seed_everything(inv.seed)
    s1.main(inv, [dict({"active": True, "force_recompute_latents": False, "video_name": "wide", "recon_config": {"enable_recon": False}}, **fit)],
            torch.device(device), log, synthetic_encoders=True)
    wait_for_pending_writes()
    entry = dict(ed_list[0], video_name="wide", **fit)
    for extra in ({}, {"source_restore": True}, {"source_restore": True, "source_restore_resample": "bicubic"}):
        seed_everything(ed.seed)
        s2.main(ed, [dict(entry, **extra)], torch.device(device), log, synthetic_encoders=True)
    root = os.path.join(base, "Results", "Prompt-Based-Editing", "mini-restore", "wide", "robot")
    plain, = [d for d in os.listdir(root) if "_restored" not in d]
    assert sorted(d[len(plain):] for d in os.listdir(root)) == ["", "_restored", "_restored-bicubic"]
    dest, box = restore_geometry((SRC_W, SRC_H), (SIZE, SIZE), "crop", 0.37, 0.0)
    for tag, name in (("_restored", "lanczos"), ("_restored-bicubic", "bicubic")):
        for i in range(N_FRAMES):
            small = np.asarray(Image.open(os.path.join(root, plain, f"video_{i:05d}.png")))
            got = np.asarray(Image.open(os.path.join(root, plain + tag, f"video_{i:05d}.png")))
            assert small.shape == (SIZE, SIZE, 3) and got.shape == (SRC_H, SRC_W, 3)
            want = rs.pillow_restore(frames[i], small, dest, box, name)
            assert np.array_equal(got, want), f"{tag} frame {i}: {int((got != want).sum())} bytes differ"
            outside = np.ones((SRC_H, SRC_W), dtype=bool)
            outside[dest[1]:dest[3], dest[0]:dest[2]] = False
            assert np.array_equal(got[outside], frames[i][outside])
        assert Image.open(os.path.join(root, plain + tag, "video.gif")).size == (SRC_W, SRC_H)
    with pytest.raises(ValueError, match="source_restore without source_fit"):
        s2.main(ed, [dict(ed_list[0], video_name="wide", source_restore=True)], torch.device(device), log, synthetic_encoders=True)


def test_edit_runner_writes_the_source_size_with_source_restore(tmp_path, monkeypatch):
    import cpu_ops_emulation as oemu
    import cpu_restore_emulation as emu
    oemu.install()
    emu.install(monkeypatch)
    monkeypatch.setenv("ANYV2V_NO_GRAPH", "1")
    check_runner_restores(tmp_path, "cpu")
