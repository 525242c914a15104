"""The way back to the source's own size on the GPU (``anyv2v_amd/csrc/restore.hip``): ``anyv2v_restore_paste_u8`` behind the horizontal
passes against Pillow's ``S.paste(E.resize(dsize, filter, box), (dx0, dy0), mask=A.resize(dsize, BILINEAR, box))`` itself, byte for byte --
the whole computation is integer, so there is no tolerance.  Random bytes; every operand (source, edit, alpha, both intermediates, the
tables, the result) lies inside a poisoned frame (``tests/track_edges.py``) at an odd byte offset, and every frame must come back untouched.
``tests/test_restore_host.py`` holds the geometry, the definition and the emulation on the CPU; ``tests/restore_spec.py`` the shared cases."""
import numpy as np
import pytest
import torch
from PIL import Image

import restore_spec as rs
import track_edges as te

pytestmark = pytest.mark.gpu

DEV = "cuda"


def differ(got, want):
    bad = (got != want)
    return f"{int(bad.sum())} of {bad.numel()} bytes differ, first at {bad.nonzero()[:4].tolist()}"


def framed_restore(S, E, A, dest, box, name, which):
    """``ops.restore_u8``'s launches through the C ABI with every operand framed by poison ``which`` (0 / 1): the source 1 byte, the edit 3,
    alpha 1, the intermediates 2 and 3, the result 3 bytes behind a 4-byte boundary.  -> (result on the CPU, the frames)."""
    from anyv2v_amd import _lib, ops
    lib = _lib.load()
    poison, poison16 = te.POISON[torch.uint8][which], te.POISON[torch.int16][which]
    F, h, w, _ = E.shape
    dw = dest[2] - dest[0]
    fS, fE = te.framed(S, poison, 1, DEV), te.framed(E, poison, 3, DEV)
    fA = None if A is None else te.framed(A, poison, 1, DEV)
    frames = [fS, fE] + ([] if fA is None else [fA])

    def table(t):   # (ksize, bounds, coeffs) on the host -> framed on the device (int16 elements: a window at offset 0 stays 4-byte aligned)
        fb, fc = te.framed(t[1].contiguous().view(torch.int16), poison16, 0, DEV), te.framed(t[2].contiguous().view(torch.int16), poison16, 0, DEV)
        frames.extend([fb, fc])
        return t[0], fb.view.data_ptr(), fc.view.data_ptr()

    def horizontal(fx, N, C, p, off):
        row0, rows, hp, _ = p
        fy = te.Frame((N, rows, dw, C), torch.uint8, poison, off, DEV)
        frames.append(fy)
        if hp is None:
            fy.view.copy_(fx.view.view(N, h, w, C)[:, row0:row0 + rows])
        else:
            ksize, b, k = table(hp)
            _lib.check(lib.anyv2v_resample_h_u8(fx.view.data_ptr(), fy.view.data_ptr(), N, h, w, C, row0, rows, dw, b, k, ksize, ops._stream()),
                       "anyv2v_resample_h_u8")
        return fy
    pe, pa = ops.restore_passes(h, w, dest, box, name)
    f_eh = horizontal(fE, F, 3, pe, 2)
    ek, eb, ec = table(pe[3])
    a_args = (1, 1, None, None, 1)
    f_ah = None
    if fA is not None:
        f_ah = horizontal(fA, A.shape[0], 1, pa, 3)
        ak, ab, ac = table(pa[3])
        a_args = (A.shape[0], pa[1], ab, ac, ak)
    fO = te.Frame(S.shape, torch.uint8, poison, 3, DEV)
    frames.append(fO)
    _lib.check(lib.anyv2v_restore_paste_u8(fS.view.data_ptr(), f_eh.view.data_ptr(), None if f_ah is None else f_ah.view.data_ptr(), fO.view.data_ptr(),
                                           F, S.shape[1], S.shape[2], *dest, pe[1], eb, ec, ek, *a_args, ops._stream()), "anyv2v_restore_paste_u8")
    torch.cuda.synchronize()
    for i, f in enumerate(frames):
        assert f.intact(), f"poison {'AB'[which]}: the frame of operand {i} changed"
    assert torch.equal(fS.view.cpu(), S) and torch.equal(fE.view.cpu(), E) and (A is None or torch.equal(fA.view.cpu(), A)), "an input changed"
    return fO.view.cpu()


def check_case(case, name="lanczos", alpha_kind=None, alpha_frames=1, F=2):
    """One shared case: ``ops.restore_u8`` on plain tensors and the framed launches under both poisons, all equal to Pillow."""
    from anyv2v_amd import ops
    _, (w, h), dest, box = rs.CASES[case]
    S, E = (torch.from_numpy(x.copy()) for x in rs.operands(case, F))
    A = None if alpha_kind is None else torch.from_numpy(rs.alpha(alpha_kind, h, w, alpha_frames).copy())
    want = torch.from_numpy(rs.expected(case, name, alpha_kind, alpha_frames, F).copy())
    got = ops.restore_u8(E.to(DEV), S.to(DEV), dest, box, name, None if A is None else A.to(DEV)).cpu()
    assert got.dtype == torch.uint8 and got.shape == want.shape and torch.equal(got, want), differ(got, want)
    for which in (0, 1):
        framed = framed_restore(S, E, A, dest, box, name, which)
        assert torch.equal(framed, want), f"framed with poison {'AB'[which]}: {differ(framed, want)}"
    return S, got


@pytest.mark.parametrize("alpha_kind", [None, "random"])
@pytest.mark.parametrize("case", list(rs.CASES))
def test_restore_equals_pillow(case, alpha_kind):
    """Crops that touch an edge and start at an odd byte, stretch, a 3.75x upscale strictly inside the frame, a downscale, the identity (both
    passes skipped), each pass skipped alone, and a dest one pixel wide and one pixel high: plain paste and random alpha."""
    S, got = check_case(case, alpha_kind=alpha_kind)
    dx0, dy0, dx1, dy1 = rs.CASES[case][2]
    outside = torch.ones(S.shape[1:3], dtype=torch.bool)
    outside[dy0:dy1, dx0:dx1] = False
    assert torch.equal(got[:, outside], S[:, outside]), "a byte outside dest is not the source's"


@pytest.mark.parametrize("name", list(rs.FILTER_CASE))
def test_every_filter(name):
    check_case(rs.FILTER_CASE[name], name, "random", 2)


@pytest.mark.parametrize("alpha_frames", [1, 2])
@pytest.mark.parametrize("alpha_kind", rs.ALPHAS)
def test_alpha_content_and_frames(alpha_kind, alpha_frames):
    """All 0 (the result is the source, every byte), all 255 (the plain paste), random bytes, a 0 / 255 step; one alpha frame for the clip
    and one per frame."""
    S, got = check_case("crop-right", "lanczos", alpha_kind, alpha_frames)
    if alpha_kind == "zero":
        assert torch.equal(got, S)
    if alpha_kind == "full":
        assert torch.equal(got, torch.from_numpy(rs.expected("crop-right", "lanczos", None, 1).copy()))


def test_one_frame_without_alpha():
    check_case("crop-left", F=1)


def test_restore_frames_end_to_end():
    """PIL frames in, fp32 alpha in [0, 1], through the geometry: against Pillow with ``rint(255 alpha)``."""
    from anyv2v_amd import prepare
    (sw, sh), (w, h) = (53, 37), (16, 16)
    S, E = rs.operands("crop-right")
    alpha = torch.from_numpy(np.random.default_rng(11).random((1, h, w), dtype=np.float32))
    alpha[0, :4] = 0.0
    alpha[0, -4:] = 1.0
    dest, box = prepare.restore_geometry((sw, sh), (w, h), "crop", 1, -1)
    A = np.rint(alpha.numpy() * 255.0).astype(np.uint8)
    want = torch.from_numpy(np.stack([rs.pillow_restore(S[f], E[f], dest, box, "bicubic", A[0]) for f in range(2)]))
    got = prepare.restore_frames([Image.fromarray(e) for e in E], [Image.fromarray(s) for s in S], "crop", 1, -1, "bicubic", alpha, device=DEV)
    assert got.is_cuda and got.dtype == torch.uint8 and torch.equal(got.cpu(), want), differ(got.cpu(), want)
    assert torch.equal(prepare.restore_frames(torch.from_numpy(E.copy()), torch.from_numpy(S.copy()), "crop", 1, -1, "bicubic", alpha, device=DEV), got)
    for bad in (alpha * 2, alpha[0], alpha.to(torch.uint8), torch.zeros(3, h, w)):
        with pytest.raises(ValueError, match="alpha"):
            prepare.restore_frames(torch.from_numpy(E.copy()), torch.from_numpy(S.copy()), "crop", 1, -1, alpha=bad, device=DEV)


def test_entry_point_refuses_bad_arguments():
    from anyv2v_amd import _lib, ops
    lib = _lib.load()
    F, sh, sw, dw, dh, rows = 2, 12, 10, 6, 5, 4
    src = torch.zeros(F * sh * sw * 3, dtype=torch.uint8, device=DEV)
    out = torch.zeros_like(src)
    eh = torch.zeros(F * rows * dw * 3, dtype=torch.uint8, device=DEV)
    ah = torch.zeros(F * rows * dw, dtype=torch.uint8, device=DEV)
    t = torch.zeros(256, dtype=torch.int32, device=DEV)
    good = dict(source=src.data_ptr(), edit_h=eh.data_ptr(), alpha_h=ah.data_ptr(), out=out.data_ptr(), F=F, sh=sh, sw=sw, dx0=2, dy0=3, dx1=8,
                dy1=8, e_rows=rows, e_bounds=t.data_ptr(), e_coeffs=t.data_ptr(), e_ksize=3, mask_frames=F, a_rows=rows, a_bounds=t.data_ptr(),
                a_coeffs=t.data_ptr(), a_ksize=3, stream=None)
    assert lib.anyv2v_restore_paste_u8(*good.values()) == 0          # (tables of zeros: every tap count is 0, nothing is read)
    torch.cuda.synchronize()
    for change, word in [(dict(dx1=11), "dest"), (dict(dy0=-1), "dest"), (dict(dy1=13), "dest"),            # dest outside the frame
                         (dict(dx1=2), "dest"), (dict(dy0=8), "dest"),                                     # an empty dest
                         (dict(out=src.data_ptr()), "overlap"), (dict(out=src.data_ptr() + 100), "overlap"),  # out aliasing the source
                         (dict(out=eh.data_ptr()), "overlap"),
                         (dict(mask_frames=3), "mask_frames"),
                         (dict(source=None), "null"), (dict(e_bounds=None), "null"), (dict(a_coeffs=None), "null"),
                         (dict(F=0), "F ="), (dict(sw=16385), "sh x sw"), (dict(e_rows=0), "rows"), (dict(a_ksize=0), "ksize"),
                         (dict(e_coeffs=t.data_ptr() + 2), "aligned")]:
        a = dict(good, **change)
        assert lib.anyv2v_restore_paste_u8(*a.values()) < 0, change
        assert word in lib.anyv2v_last_error().decode() and "restore_paste" in lib.anyv2v_last_error().decode(), (change, lib.anyv2v_last_error())
    # the wrapper refuses the same as ValueErrors before anything is launched
    E, S = torch.zeros(2, 16, 16, 3, dtype=torch.uint8, device=DEV), torch.zeros(2, 37, 53, 3, dtype=torch.uint8, device=DEV)
    for kw in [dict(dest=(0, 0, 54, 37)), dict(dest=(5, 5, 5, 9)), dict(dest=(0, 0, 20.5, 9)), dict(box=(0, 0, 17, 16)), dict(box=(4, 0, 4, 16)),
               dict(resample="nearest"), dict(alpha_u8=torch.zeros(3, 16, 16, dtype=torch.uint8, device=DEV)),
               dict(alpha_u8=torch.zeros(1, 16, 16, device=DEV))]:
        with pytest.raises(ValueError):
            ops.restore_u8(E, S, **dict(dict(dest=(0, 0, 38, 37), box=(0.0, 0.0, 16.0, 16.0)), **kw))
    for e, s in [(E.cpu(), S), (E, S[:1]), (E.float(), S), (E, S[:, :, :, :2])]:
        with pytest.raises(ValueError):
            ops.restore_u8(e, s, (0, 0, 38, 37), (0.0, 0.0, 16.0, 16.0))
