"""Resampling on the GPU (``anyv2v_amd/csrc/resample.hip``): the kernels against Pillow's ``Image.resize`` itself, byte for byte -- the
whole computation is integer, so there is no tolerance; reads and writes at the operands' edges through the C ABI with framed operands
(``tests/track_edges.py``); windows; the pipeline's ``prepare_frames`` / ``prepare_mask``; the prepared tensor through the VAE; and the
inversion runner with ``source_fit``.  ``tests/test_resample_host.py`` holds the spec, the tables and the geometry on the CPU."""
import numpy as np
import pytest
import torch
from PIL import Image

import resample_spec as spec
import test_resample_host as host
import track_edges as te

pytestmark = pytest.mark.gpu

DEV = "cuda"


def differ(got, want):
    bad = (got != want)
    return f"{int(bad.sum())} of {bad.numel()} bytes differ, first at {bad.nonzero()[:4].tolist()}"


def check_against_pillow(a, size, name, box=None):
    """``a``: uint8 numpy [F, H, W, C] -> ``ops.resample_u8`` of all frames at once against Pillow frame by frame."""
    from anyv2v_amd import ops
    got = ops.resample_u8(torch.from_numpy(a.copy()).to(DEV), size, name, box=box).cpu()
    C = a.shape[3]
    want = torch.from_numpy(np.stack([host.pillow(f[:, :, 0] if C == 1 else f, size, name, box).reshape(size[1], size[0], C) for f in a]))
    assert got.dtype == torch.uint8 and got.shape == want.shape and torch.equal(got, want), differ(got, want)
    return got


@pytest.mark.parametrize("name", host.FILTERS)
@pytest.mark.parametrize("C", [3, 1], ids=["RGB", "L"])
@pytest.mark.parametrize("i", range(len(host.CASES)), ids=host.CASE_IDS)
def test_kernels_equal_pillow(i, C, name):
    (H, W), (oh, ow), box = host.CASES[i]
    a = np.asarray(host.source(H, W, C)).reshape(H, W, C)
    check_against_pillow(np.stack([a, a[::-1, ::-1]]), (ow, oh), name, box)      # F = 2: the frame stride


@pytest.mark.parametrize("name", host.FILTERS)
@pytest.mark.parametrize("C", [3, 1], ids=["RGB", "L"])
def test_ragged_rows(C, name):
    """40 x 71 -> 24 x 33: rows of 213 and 71 bytes, so every residue of the 4-byte grouping occurs in both passes, and an output width
    that is a multiple of no block."""
    a = np.asarray(host.source(40, 71, C)).reshape(40, 71, C)
    check_against_pillow(np.stack([a, a[::-1], a[:, ::-1]]), (33, 24), name)


@pytest.mark.parametrize("size", [(1, 1), (1, 9), (300, 1), (129, 5)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_frame_and_one_pixel_outputs(size):
    a = np.asarray(host.source(37, 53, 3))[None]
    for name in ("lanczos", "box"):
        check_against_pillow(a, size, name)


def test_a_span_as_wide_as_the_largest_side():
    """W = 16384 down to 40: the horizontal pass stages the whole row (its largest LDS request); 16384 rows down to 3 in the vertical."""
    rng = np.random.default_rng(3)
    check_against_pillow(rng.integers(0, 256, (1, 2, 16384, 3), dtype=np.uint8), (40, 2), "lanczos")
    check_against_pillow(rng.integers(0, 256, (1, 16384, 5, 1), dtype=np.uint8), (5, 3), "bicubic")


def test_both_passes_skipped_is_a_copy_and_refusals():
    from anyv2v_amd import ops
    a = torch.from_numpy(np.asarray(host.source(50, 70, 3)).copy())[None].to(DEV)
    same = ops.resample_u8(a, (70, 50))
    assert torch.equal(same, a) and same.data_ptr() != a.data_ptr()
    assert torch.equal(ops.resample_u8(a, (70, 50), window=(3, 4, 20, 10)), a[:, 4:14, 3:23])
    for kw in [dict(size=(32, 31), window=(0, 0, 33, 31)), dict(size=(32, 31), window=(-1, 0, 4, 4)), dict(size=(0, 31)),
               dict(size=(32, 20000)), dict(size=(32, 31), resample="nearest"), dict(size=(32, 31), box=(0, 0, 71, 50)),
               dict(size=(32, 31), box=(5, 0, 5, 50))]:
        with pytest.raises(ValueError):
            ops.resample_u8(a, **kw)
    for bad in (a.float(), a[0], a.cpu(), a[:, :, :, :2].contiguous(), a[:, ::2]):
        with pytest.raises(ValueError):
            ops.resample_u8(bad, (32, 31))


# ------------------------------------------------------------------------------------------------ edges, through the C ABI
def _tables(in_size, in0, in1, out_size, name):
    from anyv2v_amd import ops
    ksize, bounds, coeffs = ops.resample_table(in_size, in0, in1, out_size, name)
    return ksize, bounds.clone(), coeffs.clone()


def _as_i16(t):
    """An int32 table as the int16 elements ``track_edges.Frame`` frames (a window at byte offset 0 keeps the table 4-byte aligned)."""
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("off", [1, 2, 3])
def test_horizontal_pass_at_the_edges_of_framed_operands(off, C):
    """Source, destination and tables inside poisoned frames; the source ``off`` bytes and the destination ``4 - off`` bytes behind a 4-byte
    boundary; rows [row0, row0 + rows) with row0 > 0 and rows < H."""
    from anyv2v_amd import _lib, ops
    lib = _lib.load()
    F, H, W, out_w, row0, rows = 2, 9, 71, 33, 2, 5
    src = torch.from_numpy(np.stack([np.asarray(host.source(H, W, C)).reshape(H, W, C)] * F).copy())
    src[1] = src[1].flip(0)
    ksize, bounds, coeffs = _tables(W, 0.0, float(W), out_w, "lanczos")
    want = torch.from_numpy(np.stack([spec.resize(f.numpy(), (out_w, H), "lanczos").reshape(H, out_w, C)[row0:row0 + rows] for f in src]))

    def launch(s, b, k, d):
        assert b.data_ptr() % 4 == 0 and k.data_ptr() % 4 == 0
        _lib.check(lib.anyv2v_resample_h_u8(s.data_ptr(), d.data_ptr(), F, H, W, C, row0, rows, out_w, b.data_ptr(), k.data_ptr(), ksize,
                                            ops._stream()), "anyv2v_resample_h_u8")
        torch.cuda.synchronize()
    te.check_framed(launch, [(src, off), (_as_i16(bounds), 0), (_as_i16(coeffs), 0)], [((F, rows, out_w, C), torch.uint8, 4 - off)], [want],
                    device=DEV)


@pytest.mark.parametrize("C", [3, 1])
@pytest.mark.parametrize("off", [1, 2, 3])
def test_vertical_pass_at_the_edges_of_framed_operands(off, C):
    from anyv2v_amd import _lib, ops
    lib = _lib.load()
    F, H, W, out_h = 2, 40, 71, 24
    src = torch.from_numpy(np.stack([np.asarray(host.source(H, W, C)).reshape(H, W, C)] * F).copy())
    src[1] = src[1].flip(1)
    ksize, bounds, coeffs = _tables(H, 0.0, float(H), out_h, "lanczos")
    want = torch.from_numpy(np.stack([spec.resize(f.numpy(), (W, out_h), "lanczos").reshape(out_h, W, C) for f in src]))

    def launch(s, b, k, d):
        _lib.check(lib.anyv2v_resample_v_u8(s.data_ptr(), d.data_ptr(), F, H, W, C, out_h, b.data_ptr(), k.data_ptr(), ksize, ops._stream()),
                   "anyv2v_resample_v_u8")
        torch.cuda.synchronize()
    te.check_framed(launch, [(src, off), (_as_i16(bounds), 0), (_as_i16(coeffs), 0)], [((F, out_h, W, C), torch.uint8, 4 - off)], [want],
                    device=DEV)


def test_entry_points_refuse_bad_arguments():
    from anyv2v_amd import _lib
    lib = _lib.load()
    x = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    t = torch.zeros(1024, dtype=torch.int32, device=DEV)
    p, q = x.data_ptr(), x.data_ptr() + 2048
    good = dict(F=1, H=8, W=8, C=3, row0=0, rows=8, out_w=4, ksize=3)
    for change in [dict(C=2), dict(C=4), dict(F=0), dict(F=65536), dict(H=0), dict(W=16385), dict(out_w=0), dict(ksize=0), dict(row0=-1),
                   dict(row0=1), dict(rows=0), dict(rows=9)]:
        a = dict(good, **change)
        assert lib.anyv2v_resample_h_u8(p, q, a["F"], a["H"], a["W"], a["C"], a["row0"], a["rows"], a["out_w"], t.data_ptr(), t.data_ptr(),
                                        a["ksize"], None) == -1, change
        if not {"row0", "rows"} & set(change):
            assert lib.anyv2v_resample_v_u8(p, q, a["F"], a["H"], a["W"], a["C"], a["out_w"], t.data_ptr(), t.data_ptr(), a["ksize"], None) == -1
    assert lib.anyv2v_resample_v_u8(p, p + 100, 1, 8, 8, 3, 4, t.data_ptr(), t.data_ptr(), 3, None) == -1        # overlap
    assert lib.anyv2v_resample_v_u8(p, q, 1, 8, 8, 3, 4, t.data_ptr() + 2, t.data_ptr(), 3, None) == -1           # a misaligned table
    assert lib.anyv2v_resample_h_u8(None, q, 1, 8, 8, 3, 0, 8, 4, t.data_ptr(), t.data_ptr(), 3, None) == -1
    assert b"resample_h" in lib.anyv2v_last_error()


# ------------------------------------------------------------------------------------------------ windows
def test_windows_at_the_corners_and_with_a_fractional_box():
    from anyv2v_amd import ops
    a = np.asarray(host.source(270, 480, 3))
    dev = torch.from_numpy(a.copy())[None].to(DEV)
    whole = check_against_pillow(a[None], (113, 64), "lanczos")
    for win in [(0, 0, 40, 24), (73, 0, 40, 24), (0, 40, 40, 24), (73, 40, 40, 24), (36, 20, 41, 23)]:
        wx, wy, ww, wh = win
        got = ops.resample_u8(dev, (113, 64), "lanczos", window=win).cpu()
        assert torch.equal(got[0], torch.from_numpy(spec.resize(a, (113, 64), "lanczos", window=win))), win
        assert torch.equal(got, whole[:, wy:wy + wh, wx:wx + ww]), win
    b = np.asarray(host.source(50, 70, 3))
    box = (3.5, 2.25, 60.0, 47.5)
    whole = check_against_pillow(b[None], (32, 31), "bicubic", box)
    for win in [(0, 0, 9, 7), (23, 24, 9, 7), (5, 6, 20, 21)]:
        wx, wy, ww, wh = win
        got = ops.resample_u8(torch.from_numpy(b.copy())[None].to(DEV), (32, 31), "bicubic", box=box, window=win).cpu()
        assert torch.equal(got[0], torch.from_numpy(spec.resize(b, (32, 31), "bicubic", box=box, window=win))), win
        assert torch.equal(got, whole[:, wy:wy + wh, wx:wx + ww]), win


def test_two_calls_return_equal_tensors():
    from anyv2v_amd import ops
    a = torch.from_numpy(np.stack([np.asarray(host.source(270, 480, 3))] * 3).copy()).to(DEV)
    first = ops.resample_u8(a, (114, 64), "lanczos", window=(20, 0, 64, 64))
    assert torch.equal(first, ops.resample_u8(a, (114, 64), "lanczos", window=(20, 0, 64, 64)))


# ------------------------------------------------------------------------------------------------ the pipeline and the runner
@pytest.fixture(scope="module")
def pipe():
    """A pipeline on the GPU with the mini VAE (one down-sampling, random weights); the preparation needs none of the other parts."""
    from anyv2v_amd.encoders import NativeVAE
    from anyv2v_amd.pipeline import I2VGenXLPipeline
    from anyv2v_amd.vae import VAEConfig
    p = I2VGenXLPipeline(vae=NativeVAE(random_init_seed=1, cfg=VAEConfig.mini()).to(DEV))
    p._device = torch.device(DEV)
    return p


@pytest.mark.parametrize("fit,x_offset", [("crop", -1), ("crop", 0), ("crop", 1), ("stretch", 0)])
def test_prepare_frames_equals_pillow(pipe, fit, x_offset):
    frames = host.wide_clip(host.N_FRAMES)
    want = torch.from_numpy(np.stack(host.expected_prepared(fit, x_offset)))
    got = pipe.prepare_frames([Image.fromarray(a) for a in frames], host.SIZE, host.SIZE, fit=fit, x_offset=x_offset)
    assert got.is_cuda and got.dtype == torch.uint8 and torch.equal(got.cpu(), want), differ(got.cpu(), want)
    assert torch.equal(pipe.prepare_frames(torch.from_numpy(np.stack(frames)), host.SIZE, host.SIZE, fit=fit, x_offset=x_offset), got)


def test_prepare_mask_keeps_the_border_in_place(pipe):
    from anyv2v_amd.prepare import fit_geometry
    mask = torch.zeros(1, host.SRC_H, host.SRC_W, dtype=torch.bool)
    mask[:, :, 70:] = True
    (rw, rh), (x, y, w, h) = fit_geometry((host.SRC_W, host.SRC_H), (host.SIZE, host.SIZE), "crop")
    got = pipe.prepare_mask(mask, host.SIZE, host.SIZE).cpu()
    assert got.dtype == torch.uint8 and tuple(got.shape) == (1, host.SIZE, host.SIZE)
    cols = (got[0] == 255).int().argmax(dim=1)
    assert bool(((cols.float() - (70 * rw / host.SRC_W - x)).abs() <= 1).all())
    want = spec.resize(mask[0].numpy().astype(np.uint8) * 255, (rw, rh), "bilinear", window=(x, y, w, h))
    assert np.array_equal(got[0].numpy(), (want >= 128).astype(np.uint8) * 255)


def test_prepared_frames_go_through_the_vae_on_the_device(pipe):
    got = pipe.prepare_frames([Image.fromarray(a) for a in host.wide_clip(host.N_FRAMES)], host.SIZE, host.SIZE)
    torch.manual_seed(0)
    lat = pipe.encode_vae_video(got, device=torch.device(DEV), height=host.SIZE, width=host.SIZE)
    assert lat.is_cuda and tuple(lat.shape) == (1, 4, host.N_FRAMES, host.SIZE // 2, host.SIZE // 2) and bool(torch.isfinite(lat.float()).all())
    torch.manual_seed(0)
    pil = [Image.fromarray(f) for f in got.cpu().numpy()]
    assert torch.equal(lat, pipe.encode_vae_video(pil, device=torch.device(DEV), height=host.SIZE, width=host.SIZE))


def test_inversion_runner_prepares_a_clip_of_another_size_on_gpu(tmp_path):
    host.check_inversion_prepares_the_clip(tmp_path, DEV)
