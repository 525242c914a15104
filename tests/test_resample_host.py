"""Resampling on the CPU: the definition (``tests/resample_spec.py``) against Pillow's ``Image.resize`` itself, byte for byte and without
a tolerance (Pillow resamples 8-bit bands in fixed point); the host planner (``anyv2v_amd/csrc/resample_plan.cpp``), built with the host
compiler under the address and undefined-behaviour sanitizers next to ``tests/resample_plan_main.cpp`` and run once as its own process,
integer for integer against the spec's tables and against the built library; the geometry of ``anyv2v_amd.prepare`` against the
reference's arithmetic; the torch emulation against the spec; the configuration keys; and the inversion runner and the ``prepare_video``
tool on the CPU emulation with the mini checkpoint.  No GPU."""
import ctypes
import functools
import json
import logging
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

import resample_spec as spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "anyv2v_amd", "csrc")

FILTERS = ["box", "bilinear", "bicubic", "lanczos"]
PIL_FILTER = {"box": Image.Resampling.BOX, "bilinear": Image.Resampling.BILINEAR, "bicubic": Image.Resampling.BICUBIC,
              "lanczos": Image.Resampling.LANCZOS}
FILTER_ID = {"lanczos": 1, "bilinear": 2, "bicubic": 3, "box": 4}          # Pillow's numbers, ANYV2V_RESAMPLE_* of the header
# (H, W) -> (out_h, out_w), box: down, up, a large ratio, a side left unchanged each way, a fractional box, a tiny source, about 100 taps
CASES = [((37, 53), (16, 24), None), ((16, 24), (40, 72), None), ((270, 480), (64, 114), None), ((33, 47), (33, 20), None),
         ((61, 45), (24, 45), None), ((50, 70), (32, 32), (3.5, 2.25, 60.0, 47.5)), ((7, 5), (64, 64), None), ((135, 240), (8, 8), None)]
CASE_IDS = [f"{h}x{w}-{oh}x{ow}" + ("-box" if box else "") for (h, w), (oh, ow), box in CASES]


@functools.lru_cache(maxsize=None)
def source(H, W, C):
    """Seeded uint8 [H, W, C] (or [H, W] for C = 1) whose top-left quarter is pure 0 / 255, four flat blocks with a step between them: the
    negative lobes of bicubic and lanczos overshoot beside a step at any scale, so the clamp is hit."""
    rng = np.random.default_rng(H * 1000 + W * 10 + C)
    a = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
    qh, qw = (H + 1) // 2, (W + 1) // 2
    yy, xx = np.mgrid[0:qh, 0:qw]
    a[:qh, :qw] = ((((yy >= qh // 2).astype(int) + (xx >= qw // 2)) & 1) * 255).astype(np.uint8)[:, :, None]
    a.setflags(write=False)
    return a[:, :, 0] if C == 1 else a


def pillow(a, size, name, box=None):
    return np.asarray(Image.fromarray(np.ascontiguousarray(a)).resize(size, resample=PIL_FILTER[name], box=box))


@functools.lru_cache(maxsize=None)
def spec_result(i, C, name):
    (H, W), (oh, ow), box = CASES[i]
    stats = {}
    out = spec.resize(source(H, W, C), (ow, oh), name, box=box, stats=stats)
    out.setflags(write=False)
    return out, stats.get("clamped", 0)


# ------------------------------------------------------------------------------------------------ the definition against Pillow
@pytest.mark.parametrize("name", FILTERS)
@pytest.mark.parametrize("C", [3, 1], ids=["RGB", "L"])
@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_spec_equals_pillow(i, C, name):
    (H, W), (oh, ow), box = CASES[i]
    got, clamped = spec_result(i, C, name)
    want = pillow(source(H, W, C), (ow, oh), name, box)
    assert got.shape == want.shape and got.dtype == np.uint8
    assert np.array_equal(got, want), f"{int((got != want).sum())} bytes differ"
    if name in ("bicubic", "lanczos"):   # (box and bilinear have no negative weight: their accumulator cannot leave [0, 255])
        assert clamped > 0, "no accumulator left [0, 255]: the clamp was not exercised"


def test_window_equals_crop_of_the_whole():
    a = source(270, 480, 3)
    whole = spec.resize(a, (113, 64), "lanczos")
    assert np.array_equal(whole, pillow(a, (113, 64), "lanczos"))
    for wx, wy, ww, wh in [(0, 0, 40, 24), (73, 0, 40, 24), (0, 40, 40, 24), (73, 40, 40, 24), (36, 20, 41, 23)]:
        got = spec.resize(a, (113, 64), "lanczos", window=(wx, wy, ww, wh))
        assert np.array_equal(got, whole[wy:wy + wh, wx:wx + ww]), (wx, wy, ww, wh)


# ------------------------------------------------------------------------------------------------ the planner
def sides():
    """(in_size, in0, in1, out_size) of every pass of CASES, and a few single sides."""
    out = []
    for (H, W), (oh, ow), box in CASES:
        x0, y0, x1, y1 = box or (0, 0, W, H)
        out += [(W, float(x0), float(x1), ow), (H, float(y0), float(y1), oh)]
    out += [(1, 0.0, 1.0, 1), (1, 0.0, 1.0, 9), (16384, 0.0, 16384.0, 3), (5, 4.999, 5.0, 2), (9, 0.0, 0.001, 4), (1080, 0.0, 1080.0, 512),
            (1920, 0.0, 1920.0, 910)]
    return sorted(set(out))


SIDES = sides()
REFUSALS = [
    ("in_size_0", (0, 0.0, 1.0, 4, 1), "in_size"), ("in_size_big", (16385, 0.0, 8.0, 4, 1), "in_size"),
    ("out_size_0", (8, 0.0, 8.0, 0, 1), "out_size"), ("out_size_negative", (8, 0.0, 8.0, -3, 1), "out_size"),
    ("out_size_big", (8, 0.0, 8.0, 16385, 1), "out_size"),
    ("box_empty", (8, 3.0, 3.0, 4, 1), "box"), ("box_reversed", (8, 5.0, 3.0, 4, 1), "box"), ("box_negative", (8, -0.5, 8.0, 4, 1), "box"),
    ("box_past_the_end", (8, 0.0, 8.5, 4, 1), "box"), ("box_nan", (8, float("nan"), 8.0, 4, 1), "box"),
    ("box_nan_end", (8, 0.0, float("nan"), 4, 1), "box"), ("box_infinite", (8, 0.0, float("inf"), 4, 1), "box"),
    ("filter_nearest", (8, 0.0, 8.0, 4, 0), "filter"), ("filter_hamming", (8, 0.0, 8.0, 4, 5), "filter"),
    ("filter_unknown", (8, 0.0, 8.0, 4, -1), "filter"),
]


def _line(in_size, in0, in1, out_size, filt, fill):
    return f"{in_size} {in0!r} {in1!r} {out_size} {filt} {fill}\n"


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    """The stand-alone build's answers: {(side, filter name): object}, {(side, filter name, 'query'): object}, {refusal name: object}."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("resample_plan") / "resample_plan_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "resample_plan_main.cpp"),
                    os.path.join(CSRC, "resample_plan.cpp"), "-o", exe], check=True)
    keys, lines = [], []
    for side in SIDES:
        for name in FILTERS:
            for fill in (1, 0):
                keys.append((side, name) if fill else (side, name, "query"))
                lines.append(_line(*side, FILTER_ID[name], fill))
    for rname, args, _ in REFUSALS:
        for fill in (1, 0):
            keys.append((rname, fill))
            lines.append(_line(*args, fill))
    out = subprocess.run([exe], input="".join(lines), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    got = out.stdout.splitlines()
    assert len(got) == len(keys)
    return {k: json.loads(line) for k, line in zip(keys, got)}


def _library_table(side, name):
    from anyv2v_amd import _lib
    lib = _lib.load()
    in_size, in0, in1, out_size = side
    ksize = lib.anyv2v_resample_table(in_size, in0, in1, out_size, FILTER_ID[name], None, None)
    bounds, coeffs = (ctypes.c_int * (out_size * 2))(), (ctypes.c_int * (out_size * ksize))()
    assert lib.anyv2v_resample_table(in_size, in0, in1, out_size, FILTER_ID[name], bounds, coeffs) == ksize
    return ksize, list(bounds), list(coeffs)


@pytest.mark.parametrize("name", FILTERS)
def test_planner_tables_are_the_specs_and_the_librarys(planner, name):
    for side in SIDES:
        ksize, bounds, coeffs = spec.table(*side, name)
        got = planner[(side, name)]
        assert got["ksize"] == ksize and got["message"] == "", (side, got["ksize"], got["message"])
        assert got["bounds"] == [v for b in bounds for v in b], side
        assert got["coeffs"] == [v for k in coeffs for v in k], side
        assert planner[(side, name, "query")] == {"ksize": ksize, "message": ""}          # the null-pointer call only returns ksize
        assert _library_table(side, name) == (ksize, got["bounds"], got["coeffs"]), side
        # what the kernels rely on: the taps lie inside the side, the rows are zero past n, the bounds do not decrease, and the int32
        # accumulator has room: 255 * sum |k| + 2^21 < 2^31
        for (xmin, n), k in zip(bounds, coeffs):
            assert 0 <= xmin and 1 <= n <= ksize and xmin + n <= side[0] and k[n:] == [0] * (ksize - n)
            assert sum(abs(v) for v in k) < 2 << 22 and 255 * sum(abs(v) for v in k) + (1 << 21) < 1 << 31
            assert max(abs(v) for v in k) < 1 << 23                                           # a 24-bit multiply takes it
        assert all(b0[0] <= b1[0] and b0[0] + b0[1] <= b1[0] + b1[1] for b0, b1 in zip(bounds, bounds[1:]))


@pytest.mark.parametrize("rname,args,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_planner_refusals(planner, rname, args, word):
    from anyv2v_amd import _lib
    lib = _lib.load()
    for fill in (1, 0):
        got = planner[(rname, fill)]
        assert got["ksize"] < 0 and word in got["message"], got
    assert lib.anyv2v_resample_table(*args, None, None) < 0 and word in lib.anyv2v_last_error().decode()


def test_no_geometry_reaches_the_accumulator_bound():
    """The last refusal -- a row with sum |k| >= 2 * 2^22 -- guards the kernels' int32 accumulator; it holds for all four filters: the pixel
    under an output's centre always carries most of the weight.  Here: boxes a fraction of a pixel wide at every phase and at both ends of
    the side, where the taps are cut on one side and the negative lobes weigh most."""
    worst = 0.0
    for name in FILTERS:
        for in_size in (1, 2, 3, 4, 7):
            for phase in (0.0, 0.01, 0.25, 0.49, 0.5, 0.51, 0.75, 0.99):
                for base in range(in_size):
                    in0 = min(base + phase, in_size - 1e-6)
                    for width in (1e-6, 0.5, in_size - in0):
                        if width <= 0 or in0 + width > in_size:
                            continue
                        _, _, coeffs = spec.table(in_size, in0, in0 + width, 1, name)
                        worst = max(worst, sum(abs(v) for v in coeffs[0]) / (1 << 22))
    assert 1.0 <= worst < 1.7


# ------------------------------------------------------------------------------------------------ the geometry
def test_fit_geometry_is_the_references_arithmetic():
    from anyv2v_amd.prepare import fit_geometry
    for sw, sh in [(1920, 1080), (1080, 1920), (480, 270), (512, 512), (513, 511), (720, 406)]:
        for w, h in [(512, 512), (64, 64)]:
            for xo in (-1, -0.3, 0, 1):
                for yo in (-1, -0.3, 0, 1):
                    # prepare_video.py:50-77 (center_crop, not longest_to_width), restated
                    scale = min(sw / w, sh / h)
                    new_w, new_h = int(sw / scale), int(sh / scale)
                    ox = max(0, min(new_w - w, int(((xo + 1) / 2) * (new_w - w))))
                    oy = max(0, min(new_h - h, int(((yo + 1) / 2) * (new_h - h))))
                    got = fit_geometry((sw, sh), (w, h), "crop", xo, yo)
                    assert got == ((new_w, new_h), (ox, oy, w, h)) == spec.fit_geometry((sw, sh), (w, h), "crop", xo, yo)
                    (rw, rh), (x, y, ww, wh) = got
                    assert 0 <= x and 0 <= y and x + ww <= rw and y + wh <= rh and (ww, wh) == (w, h)
            assert fit_geometry((sw, sh), (w, h), "stretch") == ((w, h), (0, 0, w, h))
    assert fit_geometry((1920, 1080), (512, 512), "crop") == ((910, 512), (199, 0, 512, 512))
    assert fit_geometry((1920, 1080), (512, 512), "crop", -1)[1][0] == 0 and fit_geometry((1920, 1080), (512, 512), "crop", 1)[1][0] == 398


@pytest.mark.parametrize("kw", [dict(x_offset=1.01), dict(y_offset=-1.5), dict(x_offset=float("nan")), dict(x_offset="0"), dict(y_offset=True)])
def test_fit_geometry_refuses_offsets_outside_the_range(kw):
    from anyv2v_amd.prepare import fit_geometry
    with pytest.raises(ValueError, match="offset"):
        fit_geometry((1920, 1080), (512, 512), "crop", **kw)


def test_fit_geometry_refuses_bad_sizes_and_fits():
    from anyv2v_amd.prepare import fit_geometry
    for args in [((0, 10), (8, 8), "crop"), ((10, 10), (8, 0), "crop"), ((10, 10), (8.5, 8), "crop"), ((10, 10), (8, 8), "longest_to_width"),
                 ((10, 10, 3), (8, 8), "crop"), ((10, 10), (8, 20000), "stretch")]:
        with pytest.raises(ValueError):
            fit_geometry(*args)


# ------------------------------------------------------------------------------------------------ the emulation against the spec
@pytest.mark.parametrize("name", FILTERS)
@pytest.mark.parametrize("i", range(len(CASES)), ids=CASE_IDS)
def test_emulation_equals_spec(i, name):
    import cpu_resample_emulation as remu
    (H, W), (oh, ow), box = CASES[i]
    for C in (3, 1):
        a = np.asarray(source(H, W, C)).reshape(H, W, C)
        frames = torch.from_numpy(np.stack([a, a[::-1, ::-1]]).copy())
        got = remu.resample_u8(frames, (ow, oh), name, box=box)
        want = spec_result(i, C, name)[0].reshape(oh, ow, C)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (2, oh, ow, C)
        assert torch.equal(got[0], torch.from_numpy(want.copy()))
        assert torch.equal(got[1], torch.from_numpy(spec.resize(frames[1].numpy(), (ow, oh), name, box=box).reshape(oh, ow, C)))


def test_emulation_windows_and_refusals():
    import cpu_resample_emulation as remu
    a = torch.from_numpy(np.asarray(source(50, 70, 3)).copy())[None]
    box = (3.5, 2.25, 60.0, 47.5)
    whole = remu.resample_u8(a, (32, 31), "bicubic", box=box)
    for win in [(0, 0, 9, 7), (23, 24, 9, 7), (5, 6, 20, 21)]:
        wx, wy, ww, wh = win
        assert torch.equal(remu.resample_u8(a, (32, 31), "bicubic", box=box, window=win), whole[:, wy:wy + wh, wx:wx + ww])
    same = remu.resample_u8(a, (70, 50))                            # both passes skipped: a copy
    assert torch.equal(same, a) and same.data_ptr() != a.data_ptr()
    for kw in [dict(size=(32, 31), window=(0, 0, 33, 31)), dict(size=(32, 31), window=(-1, 0, 4, 4)), dict(size=(32, 31), window=(0, 0, 0, 4)),
               dict(size=(0, 31)), dict(size=(32, 20000)), dict(size=(32, 31), resample="nearest"), dict(size=(32, 31), box=(0, 0, 71, 50)),
               dict(size=(32, 31), box=(5, 0, 5, 50)), dict(size=(32.5, 31)), dict(size=(32, 31), window=(0, 0, 4))]:
        with pytest.raises(ValueError):
            remu.resample_u8(a, **kw)
    with pytest.raises(ValueError):
        remu.resample_u8(a.float(), (32, 31))


# ------------------------------------------------------------------------------------------------ the configuration keys and the ABI
def test_plan_from_config_resolves_every_key():
    from anyv2v_amd.config import OmegaConf
    from anyv2v_amd.prepare import PreparePlan, plan_from_config
    assert plan_from_config(OmegaConf.create({"image_size": [512, 512]})) is None
    assert plan_from_config(OmegaConf.create({"source_fit": None})) is None
    assert plan_from_config(OmegaConf.create({"source_fit": "crop"})) == PreparePlan("crop", 0.0, 0.0, "lanczos", None)
    full = {"source_fit": "crop", "source_x_offset": -0.3, "source_y_offset": 1, "source_resample": "bicubic", "source_size": [448, 256]}
    assert plan_from_config(OmegaConf.create(full)) == PreparePlan("crop", -0.3, 1.0, "bicubic", (448, 256))
    assert plan_from_config(OmegaConf.create({"source_fit": "stretch"})) == PreparePlan("stretch")
    import types
    assert plan_from_config(types.SimpleNamespace(source_fit="stretch", source_resample="box")) == PreparePlan("stretch", resample="box")
    for bad, key in [({"source_fit": "cover"}, "source_fit"), ({"source_fit": True}, "source_fit"),
                     ({"source_fit": "crop", "source_x_offset": 1.5}, "source_x_offset"),
                     ({"source_fit": "crop", "source_y_offset": "top"}, "source_y_offset"),
                     ({"source_fit": "crop", "source_resample": "nearest"}, "source_resample"),
                     ({"source_fit": "crop", "source_size": [512]}, "source_size"), ({"source_fit": "crop", "source_size": [500, 512]}, "source_size"),
                     ({"source_fit": "crop", "source_size": [0, 512]}, "source_size"),
                     ({"source_fit": "stretch", "source_x_offset": 0.5}, "source_x_offset"),
                     ({"source_x_offset": 0.5}, "source_x_offset"), ({"source_resample": "box"}, "source_resample"),
                     ({"source_size": [512, 512]}, "source_size")]:
        with pytest.raises(ValueError, match=key):
            plan_from_config(OmegaConf.create(bad))


def test_shipped_templates_do_not_set_the_key():
    from anyv2v_amd.config import OmegaConf
    from anyv2v_amd.prepare import plan_from_config
    for d in ("group_ddim_inversion", "group_pnp_edit"):
        assert plan_from_config(OmegaConf.load(os.path.join(ROOT, "configs", d, "template.yaml"))) is None
        for e in json.load(open(os.path.join(ROOT, "configs", d, "group_config.json"))):
            assert not any(k.startswith("source_") for k in e)


def test_abi_version_stays_and_the_header_declares_the_symbols():
    from anyv2v_amd import _lib
    assert _lib.ABI_VERSION == 105 and _lib.load().anyv2v_version() == 105
    with open(os.path.join(ROOT, "include", "anyv2v_hip.h")) as f:
        header = f.read()
    assert "#define ANYV2V_ABI_VERSION 105" in header
    for name in ("anyv2v_resample_table", "anyv2v_resample_h_u8", "anyv2v_resample_v_u8"):
        assert f"int {name}(" in header and name in _lib.SYMBOLS
    for name, number in FILTER_ID.items():
        assert f"#define ANYV2V_RESAMPLE_{name.upper()} {number}\n" in header and _lib.RESAMPLE_FILTERS[name] == number
        assert int(PIL_FILTER[name]) == number
    assert f"#define ANYV2V_RESAMPLE_MAX_SIDE {_lib.RESAMPLE_MAX_SIDE}\n" in header


def test_a_stale_library_is_a_clear_error(tmp_path, monkeypatch):
    """A library from before the symbols existed: ``load()`` says which symbol is missing and how to rebuild, as ``HipExtensionMissing``."""
    from anyv2v_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setitem(_lib.SYMBOLS, "anyv2v_resample_not_there_u8", (ctypes.c_int, []))
    with pytest.raises(_lib.HipExtensionMissing, match="anyv2v_resample_not_there_u8.*rebuild"):
        _lib.load()


# ------------------------------------------------------------------------------------------------ the runner and the tool, CPU emulation
SRC_H, SRC_W, N_FRAMES, SIZE, N_STEPS = 88, 120, 3, 64, 2


def wide_clip(n):
    yy, xx = np.mgrid[0:SRC_H, 0:SRC_W]
    rng = np.random.default_rng(5)
    noise = rng.integers(0, 256, (SRC_H, SRC_W, 3), dtype=np.uint8)
    out = []
    for i in range(n):
        a = np.stack([(xx * 3 + 17 * i) % 256, (yy * 5) % 256, ((xx + 2 * yy) + 40 * i) % 256], -1).astype(np.uint8)
        a[20:50, 30:80] = noise[20:50, 30:80]          # texture with hard edges: the lobes overshoot
        out.append(a)
    return out


def make_workspace(base):
    """The mini checkpoint of ``test_runners_e2e`` and a clip ``wide`` of 88 x 120 frames."""
    import test_runners_e2e as e2e
    base = e2e._make_workspace(base)
    clip = os.path.join(base, "demo", "wide")
    os.makedirs(clip, exist_ok=True)
    for i, a in enumerate(wide_clip(N_FRAMES)):
        Image.fromarray(a).save(os.path.join(clip, f"{i:05d}.png"))
    return base


def inversion_configs(base, tag, **entry):
    import test_runners_e2e as e2e
    inv, _, _, _ = e2e._configs(base, tag)
    inv.image_size, inv.n_frames = [SIZE, SIZE], N_FRAMES
    inv.inverse_config.n_steps = N_STEPS
    return inv, [dict({"active": True, "force_recompute_latents": False, "video_name": "wide", "recon_config": {"enable_recon": False}}, **entry)]


def expected_prepared(fit="crop", x_offset=0.0, y_offset=0.0):
    from anyv2v_amd.prepare import fit_geometry
    resize_to, (x, y, w, h) = fit_geometry((SRC_W, SRC_H), (SIZE, SIZE), fit, x_offset, y_offset)
    return [np.asarray(Image.fromarray(a).resize(resize_to, resample=Image.Resampling.LANCZOS).crop((x, y, x + w, y + h))) for a in wide_clip(N_FRAMES)]


def check_inversion_prepares_the_clip(tmp_path, device):
    base = make_workspace(tmp_path)
    torch.set_grad_enabled(False)
    from anyv2v_amd import run_group_ddim_inversion as s1
    from anyv2v_amd.utils import seed_everything, wait_for_pending_writes
    log = logging.getLogger("resample")
    inv, entries = inversion_configs(base, "prep", source_fit="crop", source_x_offset=-1)
    inv.device = device
    seed_everything(inv.seed)
    s1.main(inv, entries, torch.device(device), log, synthetic_encoders=True)
    wait_for_pending_writes()
    out_dir = os.path.join(base, "inversions", "mini-prep", "wide")
    want = expected_prepared(x_offset=-1)
    assert sorted(os.listdir(os.path.join(out_dir, "prepared_frames"))) == [f"{i:05d}.png" for i in range(N_FRAMES)]
    for i, w in enumerate(want):
        got = np.asarray(Image.open(os.path.join(out_dir, "prepared_frames", f"{i:05d}.png")))
        assert got.shape == (SIZE, SIZE, 3) and np.array_equal(got, w), f"frame {i}: {int((got != w).sum())} bytes differ"
    lat = [f for f in os.listdir(os.path.join(out_dir, "ddim_latents")) if f.startswith("ddim_latents_")]
    assert len(lat) == N_STEPS
    x = torch.load(os.path.join(out_dir, "ddim_latents", lat[0]))
    assert tuple(x.shape) == (1, 4, N_FRAMES, SIZE // 8, SIZE // 8) and bool(torch.isfinite(x.float()).all())
    # the same entry without the key: today's refusal (the runner then looks for the mp4, which is not there either)
    inv, entries = inversion_configs(base, "plain")
    inv.device = device
    from anyv2v_amd.utils import load_video_frames
    with pytest.raises(ValueError, match="does not match config.image_size"):
        load_video_frames(os.path.join(base, "demo", "wide"), N_FRAMES, (SIZE, SIZE))
    with pytest.raises(Exception):
        s1.main(inv, entries, torch.device(device), log, synthetic_encoders=True)
    assert not os.path.exists(os.path.join(base, "inversions", "mini-plain", "wide", "prepared_frames"))


def test_inversion_runner_prepares_a_clip_of_another_size(tmp_path, monkeypatch):
    import cpu_ops_emulation as emu
    import cpu_resample_emulation as remu
    emu.install()
    remu.install(monkeypatch)
    monkeypatch.setenv("ANYV2V_NO_GRAPH", "1")
    check_inversion_prepares_the_clip(tmp_path, "cpu")


def test_prepare_video_tool(tmp_path, monkeypatch, capsys):
    import cpu_resample_emulation as remu
    remu.install(monkeypatch)
    from anyv2v_amd import prepare_video
    from anyv2v_amd.prepare import fit_geometry
    clip = tmp_path / "in" / "walk"
    os.makedirs(clip)
    frames = wide_clip(7)
    for i, a in enumerate(frames):
        Image.fromarray(a).save(clip / f"{i:05d}.png")
    out = prepare_video.main(["--video_path", str(clip), "--output_folder", str(tmp_path / "out"), "--width", "64", "--height", "48",
                              "--n_frames", "3", "--center_crop", "--x_offset", "0.5", "--device", "cpu"])
    assert out == [str(tmp_path / "out" / "walk")] and sorted(os.listdir(out[0])) == ["00000.png", "00001.png", "00002.png"]
    resize_to, (x, y, w, h) = fit_geometry((SRC_W, SRC_H), (64, 48), "crop", 0.5, 0.0)
    for i, k in enumerate((0, 2, 4)):                     # (i * 7) // 3
        want = np.asarray(Image.fromarray(frames[k]).resize(resize_to, resample=Image.Resampling.LANCZOS).crop((x, y, x + w, y + h)))
        assert np.array_equal(np.asarray(Image.open(os.path.join(out[0], f"{i:05d}.png"))), want), i
    # without --center_crop: the plain resize; --input_folder finds the frame directory
    out = prepare_video.main(["--input_folder", str(tmp_path / "in"), "--output_folder", str(tmp_path / "out2"), "--width", "40", "--height",
                              "32", "--n_frames", "7", "--device", "cpu"])
    want = np.asarray(Image.fromarray(frames[6]).resize((40, 32), resample=Image.Resampling.LANCZOS))
    assert np.array_equal(np.asarray(Image.open(os.path.join(out[0], "00006.png"))), want)
    for flag in ("--start_time", "--end_time", "--clip_duration"):
        with pytest.raises(SystemExit):
            prepare_video.main(["--video_path", str(clip), "--output_folder", str(tmp_path / "out3"), flag, "1.5", "--device", "cpu"])
        assert "decoder" in capsys.readouterr().err
    with pytest.raises(ValueError, match="n_frames"):
        prepare_video.main(["--video_path", str(clip), "--output_folder", str(tmp_path / "out3"), "--n_frames", "8", "--device", "cpu"])
    assert not os.path.exists(tmp_path / "out3")


def test_pipeline_methods_on_the_emulation(monkeypatch):
    """``prepare_frames`` takes PIL frames or a tensor and refuses unequal sizes; ``prepare_mask`` keeps a half-plane's border in place."""
    import cpu_resample_emulation as remu
    remu.install(monkeypatch)
    from anyv2v_amd import prepare
    frames = wide_clip(2)
    pil = [Image.fromarray(a) for a in frames]
    want = torch.from_numpy(np.stack(expected_prepared()[:2]))
    assert torch.equal(prepare.prepare_frames(pil, SIZE, SIZE, device="cpu"), want)
    assert torch.equal(prepare.prepare_frames(torch.from_numpy(np.stack(frames)), SIZE, SIZE, device="cpu"), want)
    with pytest.raises(ValueError, match="unequal"):
        prepare.prepare_frames([pil[0], pil[1].crop((0, 0, 100, 88))], SIZE, SIZE, device="cpu")
    with pytest.raises(ValueError):
        prepare.prepare_frames(torch.zeros(2, 88, 120, 3), SIZE, SIZE, device="cpu")
    mask = torch.zeros(1, SRC_H, SRC_W, dtype=torch.bool)
    mask[:, :, 70:] = True                                                    # x >= 70 of 120
    (rw, rh), (x, y, w, h) = prepare.fit_geometry((SRC_W, SRC_H), (SIZE, SIZE), "crop")
    got = prepare.prepare_mask(mask, SIZE, SIZE, device="cpu")
    assert got.dtype == torch.uint8 and tuple(got.shape) == (1, SIZE, SIZE) and set(got.unique().tolist()) == {0, 255}
    edge = 70 * rw / SRC_W - x                                                # the border in the prepared frame
    cols = (got[0] == 255).int().argmax(dim=1)
    assert bool((got[0, :, :1] == 0).all()) and bool(((cols.float() - edge).abs() <= 1).all())
    assert torch.equal(got, prepare.prepare_mask(mask.to(torch.uint8) * 255, SIZE, SIZE, device="cpu"))
    want = spec.resize(mask[0].numpy().astype(np.uint8) * 255, (rw, rh), "bilinear", window=(x, y, w, h))
    assert np.array_equal(got[0].numpy(), (want >= 128).astype(np.uint8) * 255)
    assert math.isfinite(edge)
