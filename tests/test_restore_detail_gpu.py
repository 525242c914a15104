"""The detail-preserving restore on the GPU (``anyv2v_amd/csrc/restore_detail.hip``): ``anyv2v_detail_gate_u8`` and
``anyv2v_restore_detail_u8`` against the definition (``tests/detail_spec.py``) byte for byte -- the whole computation is integer, so there is
no tolerance.  Beside it: a gate of 0 gives ``ops.restore_u8`` (which ``test_restore_gpu`` holds against Pillow), and an edit that changes
nothing gives the source's own bytes.  Every operand of the framed launches (source, edit, prepared, gate, alpha, the four intermediates,
the uint16 scratch, the tables, the result) lies inside a poisoned frame (``tests/track_edges.py``) at an odd offset, and every frame must
come back untouched.  ``tests/test_restore_detail_host.py`` holds the definition and the emulation on the CPU."""
import numpy as np
import pytest
import torch
from PIL import Image

import detail_spec as ds
import restore_spec as rs
import track_edges as te

pytestmark = pytest.mark.gpu

DEV = "cuda"


def tt(a):
    return torch.from_numpy(np.array(a, copy=True))


def differ(got, want):
    bad = (got != want)
    return f"{int(bad.sum())} of {bad.numel()} bytes differ, first at {bad.nonzero()[:4].tolist()}"


def framed_gate(E, P, lo, hi, radius, which):
    """``anyv2v_detail_gate_u8`` through the C ABI under poison ``which``: the edit 3 bytes behind a 4-byte boundary, the prepared frames 1,
    the uint16 scratch 2 (an odd element), the result 3."""
    from anyv2v_amd import _lib, ops
    poison, poison16 = te.POISON[torch.uint8][which], te.POISON[torch.int16][which]
    F, h, w, _ = E.shape
    fE, fP = te.framed(E, poison, 3, DEV), te.framed(P, poison, 1, DEV)
    fW, fG = te.Frame((F, h, w), torch.int16, poison16, 2, DEV), te.Frame((F, h, w), torch.uint8, poison, 3, DEV)
    _lib.check(_lib.load().anyv2v_detail_gate_u8(fE.view.data_ptr(), fP.view.data_ptr(), fG.view.data_ptr(), F, h, w, lo, hi, radius,
                                                 fW.view.data_ptr(), 2 * F * h * w, ops._stream()), "anyv2v_detail_gate_u8")
    torch.cuda.synchronize()
    for i, f in enumerate((fE, fP, fW, fG)):
        assert f.intact(), f"poison {'AB'[which]}: the frame of operand {i} changed"
    assert torch.equal(fE.view.cpu(), E) and torch.equal(fP.view.cpu(), P), "an input changed"
    return fG.view.cpu()


def framed_restore(S, E, P, G, A, dest, box, name, which):
    """``ops.restore_detail_u8``'s launches through the C ABI with every operand framed by poison ``which`` (0 / 1): the source 1 byte, the
    edit 3, the prepared frames 1, the gate 3, alpha 1, the intermediates 2 / 3 / 1 / 3, the result 3 bytes behind a 4-byte boundary."""
    from anyv2v_amd import _lib, ops
    lib = _lib.load()
    poison, poison16 = te.POISON[torch.uint8][which], te.POISON[torch.int16][which]
    F, h, w, _ = E.shape
    dw = dest[2] - dest[0]
    ins = [(S, 1), (E, 3), (P, 1), (G, 3)] + ([] if A is None else [(A, 1)])
    fin = [te.framed(t, poison, off, DEV) for t, off in ins]
    frames = list(fin)
    fS, fE, fP, fG = fin[:4]
    tables = {}

    def table(t):   # (ksize, bounds, coeffs) on the host -> framed on the device, once per table (int16 elements: offset 0 stays 4-byte aligned)
        if id(t) not in tables:
            fb, fc = (te.framed(x.contiguous().view(torch.int16), poison16, 0, DEV) for x in t[1:])
            frames.extend([fb, fc])
            tables[id(t)] = (t[0], fb.view.data_ptr(), fc.view.data_ptr())
        return tables[id(t)]

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
    f_eh, f_ph = horizontal(fE, F, 3, pe, 2), horizontal(fP, F, 3, pe, 3)
    f_gh = horizontal(fG, G.shape[0], 1, pa, 1)
    f_ah = None if A is None else horizontal(fin[4], A.shape[0], 1, pa, 3)
    ek, eb, ec = table(pe[3])
    ak, ab, ac = table(pa[3])
    fO = te.Frame(S.shape, torch.uint8, poison, 3, DEV)
    frames.append(fO)
    _lib.check(lib.anyv2v_restore_detail_u8(fS.view.data_ptr(), f_eh.view.data_ptr(), f_ph.view.data_ptr(), f_gh.view.data_ptr(),
                                            None if f_ah is None else f_ah.view.data_ptr(), fO.view.data_ptr(), F, S.shape[1], S.shape[2], *dest,
                                            pe[1], eb, ec, ek, G.shape[0], 1 if A is None else A.shape[0], pa[1], ab, ac, ak, ops._stream()),
               "anyv2v_restore_detail_u8")
    torch.cuda.synchronize()
    for i, f in enumerate(frames):
        assert f.intact(), f"poison {'AB'[which]}: the frame of operand {i} changed"
    for f, (t, _) in zip(fin, ins):
        assert torch.equal(f.view.cpu(), t), "an input changed"
    return fO.view.cpu()


def check_case(case, name="lanczos", alpha_kind=None, alpha_frames=1, gate_frames=2):
    """One shared case, random operands under a random gate: ``ops.restore_detail_u8`` on plain tensors and the framed launches under both
    poisons, all equal to the definition."""
    from anyv2v_amd import ops
    _, (w, h), dest, box = rs.CASES[case]
    S, E = (tt(x) for x in rs.operands(case))
    P, G = tt(ds.prepared(case)), tt(ds.random_gate(case, gate_frames))
    A = None if alpha_kind is None else tt(rs.alpha(alpha_kind, h, w, alpha_frames))
    want = tt(ds.expected(case, name, alpha_kind, alpha_frames, gate_frames))
    got = ops.restore_detail_u8(E.to(DEV), P.to(DEV), G.to(DEV), S.to(DEV), dest, box, name, None if A is None else A.to(DEV)).cpu()
    assert got.dtype == torch.uint8 and got.shape == want.shape and torch.equal(got, want), differ(got, want)
    for which in (0, 1):
        framed = framed_restore(S, E, P, G, A, dest, box, name, which)
        assert torch.equal(framed, want), f"framed with poison {'AB'[which]}: {differ(framed, want)}"
    return S, got


# ------------------------------------------------------------------------------------------------ the gate
@pytest.mark.parametrize("kind", ds.SETS)
@pytest.mark.parametrize("case", ["crop-right", "down", "identity"])
def test_gate_equals_the_definition(case, kind):
    """Frames of 16 x 16, 64 x 64 and 24 x 16; every radius in {0, 1, 2, 16} (at 16 the window is wider than the 16 x 16 frame: every clamp
    fires) under every (lo, hi) in {(0, 1), (8, 32), (254, 255)}; the default parameters also framed, under both poisons."""
    from anyv2v_amd import ops
    E, P = (tt(x) for x in ds.structured(case, kind))
    e, p = E.to(DEV), P.to(DEV)
    for radius in ds.RADII:
        for lo, hi in ds.THRESHOLDS:
            want = tt(ds.expected_gate(case, kind, lo, hi, radius))
            got = ops.detail_gate_u8(e, p, lo, hi, radius).cpu()
            assert got.dtype == torch.uint8 and torch.equal(got, want), f"radius {radius}, ({lo}, {hi}): {differ(got, want)}"
    assert torch.equal(ops.detail_gate_u8(e, p).cpu(), tt(ds.expected_gate(case, kind)))           # the defaults are 8 / 32 / 2
    for which in (0, 1):
        for radius in (2, 16):
            framed = framed_gate(E, P, 8, 32, radius, which)
            assert torch.equal(framed, tt(ds.expected_gate(case, kind, 8, 32, radius))), f"framed, poison {'AB'[which]}, radius {radius}"


def test_gate_of_a_row_wider_than_one_block():
    """300 columns: two blocks a row, the halo of the second one read from the first one's pixels; 3 rows under radius 16.  The difference
    grows along the row (0 .. 49), so the means sweep through the ramp."""
    from anyv2v_amd import ops
    rng = np.random.default_rng(41)
    P = rng.integers(64, 192, (1, 3, 300, 3), dtype=np.uint8)
    E = (P.astype(np.int64) + rng.integers(-1, 2, P.shape) * (np.arange(300) // 6)[None, None, :, None]).astype(np.uint8)
    for radius in (1, 16):
        want = tt(ds.gate(E[0], P[0], 8, 32, radius)[None])
        assert len(np.unique(want.numpy())) > 8
        got = ops.detail_gate_u8(tt(E).to(DEV), tt(P).to(DEV), 8, 32, radius).cpu()
        assert torch.equal(got, want), differ(got, want)
        assert torch.equal(framed_gate(tt(E), tt(P), 8, 32, radius, 0), want)


# ------------------------------------------------------------------------------------------------ the paste
@pytest.mark.parametrize("alpha_kind", [None, "random"])
@pytest.mark.parametrize("case", list(rs.CASES))
def test_restore_detail_equals_the_definition(case, alpha_kind):
    S, got = check_case(case, alpha_kind=alpha_kind)
    dx0, dy0, dx1, dy1 = rs.CASES[case][2]
    outside = torch.ones(S.shape[1:3], dtype=torch.bool)
    outside[dy0:dy1, dx0:dx1] = False
    assert torch.equal(got[:, outside], S[:, outside]), "a byte outside dest is not the source's"


@pytest.mark.parametrize("name", list(rs.FILTER_CASE))
def test_every_filter(name):
    check_case(rs.FILTER_CASE[name], name, "random", 2)


@pytest.mark.parametrize("gate_frames", [1, 2])
@pytest.mark.parametrize("alpha_frames", [1, 2])
def test_gate_and_alpha_frames(alpha_frames, gate_frames):
    check_case("crop-right", "lanczos", "step", alpha_frames, gate_frames)


@pytest.mark.parametrize("kind", ["ramp", "clamp"])
@pytest.mark.parametrize("case", ["crop-left", "up-3.75", "down"])
def test_structured_operands_through_both_kernels(case, kind):
    """The gate the kernel makes from the structured sets, then the paste under it: interior ramp values, and ``e + add`` clamped at both
    ends (the clamp set under the thresholds (254, 255), which leave its gate open)."""
    from anyv2v_amd import ops
    _, _, dest, box = rs.CASES[case]
    S = rs.operands(case)[0]
    E, P = ds.structured(case, kind)
    lo, hi, radius = (254, 255, 1) if kind == "clamp" else (8, 32, 2)
    G = ds.expected_gate(case, kind, lo, hi, radius)
    want = tt(np.stack([ds.restore_detail(S[f], E[f], P[f], G[f], dest, box, "lanczos") for f in range(2)]))
    e, p = tt(E).to(DEV), tt(P).to(DEV)
    got = ops.restore_detail_u8(e, p, ops.detail_gate_u8(e, p, lo, hi, radius), tt(S).to(DEV), dest, box).cpu()
    assert torch.equal(got, want), differ(got, want)


@pytest.mark.parametrize("alpha_kind", [None, "random"])
@pytest.mark.parametrize("case", ["crop-right", "down", "identity"])
def test_gate_zero_is_restore_u8(case, alpha_kind):
    """... which ``restore_spec.expected`` says is Pillow."""
    from anyv2v_amd import ops
    _, (w, h), dest, box = rs.CASES[case]
    S, E = (tt(x).to(DEV) for x in rs.operands(case))
    P = tt(ds.prepared(case)).to(DEV)
    A = None if alpha_kind is None else tt(rs.alpha(alpha_kind, h, w, 1)).to(DEV)
    for frames in (1, 2):
        got = ops.restore_detail_u8(E, P, torch.zeros((frames, h, w), dtype=torch.uint8, device=DEV), S, dest, box, "lanczos", A)
        assert torch.equal(got, ops.restore_u8(E, S, dest, box, "lanczos", A))
        assert torch.equal(got.cpu(), tt(rs.expected(case, "lanczos", alpha_kind, 1)))


@pytest.mark.parametrize("case", list(rs.CASES))
def test_an_unchanged_edit_restores_the_source(case):
    """E == P, the gate from ``detail_gate_u8``: the source on every byte, for every filter, with and without alpha."""
    from anyv2v_amd import ops
    _, (w, h), dest, box = rs.CASES[case]
    S = tt(rs.operands(case)[0]).to(DEV)
    P = tt(ds.prepared(case)).to(DEV)
    G = ops.detail_gate_u8(P, P)
    assert bool((G == 255).all())
    A = tt(rs.alpha("random", h, w, 2)).to(DEV)
    for name in rs.FILTER_CASE:
        for a in (None, A):
            got = ops.restore_detail_u8(P, P, G, S, dest, box, name, a)
            assert torch.equal(got, S), (name, a is not None, differ(got, S))


# ------------------------------------------------------------------------------------------------ refusals, end to end
def test_entry_points_refuse_bad_arguments():
    from anyv2v_amd import _lib, ops
    lib = _lib.load()
    F, sh, sw, dw, dh, rows, h, w = 2, 12, 10, 6, 5, 4, 8, 8
    src = torch.zeros(F * sh * sw * 3, dtype=torch.uint8, device=DEV)
    out = torch.zeros_like(src)
    eh, ph = (torch.zeros(F * rows * dw * 3, dtype=torch.uint8, device=DEV) for _ in range(2))
    gh, ah = (torch.zeros(F * rows * dw, dtype=torch.uint8, device=DEV) for _ in range(2))
    t = torch.zeros(256, dtype=torch.int32, device=DEV)
    good = dict(source=src.data_ptr(), edit_h=eh.data_ptr(), prep_h=ph.data_ptr(), gate_h=gh.data_ptr(), alpha_h=ah.data_ptr(), out=out.data_ptr(),
                F=F, sh=sh, sw=sw, dx0=2, dy0=3, dx1=8, dy1=8, e_rows=rows, e_bounds=t.data_ptr(), e_coeffs=t.data_ptr(), e_ksize=3, gate_frames=F,
                mask_frames=F, a_rows=rows, a_bounds=t.data_ptr(), a_coeffs=t.data_ptr(), a_ksize=3, stream=None)
    assert lib.anyv2v_restore_detail_u8(*good.values()) == 0          # (tables of zeros: every tap count is 0, nothing is read)
    torch.cuda.synchronize()
    for change, word in [(dict(dx1=11), "dest"), (dict(dy0=-1), "dest"), (dict(dy1=13), "dest"), (dict(dx1=2), "dest"), (dict(dy0=8), "dest"),
                         (dict(out=src.data_ptr()), "overlap"), (dict(out=src.data_ptr() + 100), "overlap"), (dict(out=eh.data_ptr()), "overlap"),
                         (dict(out=ph.data_ptr()), "overlap"), (dict(out=gh.data_ptr()), "overlap"), (dict(out=ah.data_ptr()), "overlap"),
                         (dict(mask_frames=3), "mask_frames"), (dict(gate_frames=3), "gate_frames"),
                         (dict(source=None), "null"), (dict(prep_h=None), "null"), (dict(gate_h=None), "null"), (dict(e_bounds=None), "null"),
                         (dict(a_coeffs=None), "null"), (dict(F=0), "F ="), (dict(sw=16385), "sh x sw"), (dict(e_rows=0), "rows"),
                         (dict(a_ksize=0), "ksize"), (dict(e_coeffs=t.data_ptr() + 2), "aligned")]:
        assert lib.anyv2v_restore_detail_u8(*dict(good, **change).values()) < 0, change
        msg = lib.anyv2v_last_error().decode()
        assert word in msg and "restore_detail" in msg, (change, msg)
    e, p = (torch.zeros(F * h * w * 3, dtype=torch.uint8, device=DEV) for _ in range(2))
    g = torch.zeros(F * h * w, dtype=torch.uint8, device=DEV)
    ws = torch.zeros(F * h * w, dtype=torch.int16, device=DEV)
    good = dict(edit=e.data_ptr(), prepared=p.data_ptr(), gate_out=g.data_ptr(), F=F, h=h, w=w, lo=8, hi=32, radius=2, scratch=ws.data_ptr(),
                scratch_bytes=2 * F * h * w, stream=None)
    assert lib.anyv2v_detail_gate_u8(*good.values()) == 0
    torch.cuda.synchronize()
    assert bool((g == 255).all())
    for change, word in [(dict(lo=32), "lo"), (dict(lo=-1), "lo"), (dict(hi=256), "hi"), (dict(radius=17), "radius"), (dict(radius=-1), "radius"),
                         (dict(edit=None), "null"), (dict(gate_out=None), "null"), (dict(scratch=None), "null"), (dict(F=0), "F ="),
                         (dict(w=0), "h x w"), (dict(scratch_bytes=2 * F * h * w - 1), "scratch"), (dict(scratch=ws.data_ptr() + 1), "aligned"),
                         (dict(gate_out=e.data_ptr() + 5), "overlap"), (dict(gate_out=ws.data_ptr()), "overlap"), (dict(scratch=p.data_ptr()), "overlap")]:
        assert lib.anyv2v_detail_gate_u8(*dict(good, **change).values()) < 0, change
        msg = lib.anyv2v_last_error().decode()
        assert word in msg and "detail_gate" in msg, (change, msg)
    # the wrappers refuse the same as ValueErrors before anything is launched
    E, S = torch.zeros(2, 16, 16, 3, dtype=torch.uint8, device=DEV), torch.zeros(2, 37, 53, 3, dtype=torch.uint8, device=DEV)
    G = torch.zeros(2, 16, 16, dtype=torch.uint8, device=DEV)
    ok = dict(dest=(0, 0, 38, 37), box=(0.0, 0.0, 16.0, 16.0))
    ops.restore_detail_u8(E, E, G, S, **ok)
    for kw in [dict(dest=(0, 0, 54, 37)), dict(dest=(5, 5, 5, 9)), dict(dest=(0, 0, 20.5, 9)), dict(box=(0, 0, 17, 16)), dict(box=(4, 0, 4, 16)),
               dict(resample="nearest"), dict(alpha_u8=torch.zeros(3, 16, 16, dtype=torch.uint8, device=DEV)),
               dict(alpha_u8=torch.zeros(1, 16, 16, device=DEV))]:
        with pytest.raises(ValueError):
            ops.restore_detail_u8(E, E, G, S, **dict(ok, **kw))
    for e_, p_, g_, s_ in [(E.cpu(), E, G, S), (E, E[:1], G, S), (E, E[:, :8], G, S), (E, E.cpu(), G, S), (E, E, G[:, :8], S), (E, E, G.float(), S),
                           (E, E, torch.zeros(3, 16, 16, dtype=torch.uint8, device=DEV), S), (E, E, G.cpu(), S), (E, E, G, S[:1]),
                           (E.float(), E, G, S), (E, E, G, S[:, :, :, :2])]:
        with pytest.raises(ValueError):
            ops.restore_detail_u8(e_, p_, g_, s_, **ok)
    for args in [(E, E, 32, 32, 2), (E, E, -1, 32, 2), (E, E, 8, 256, 2), (E, E, 8.5, 32, 2), (E, E, 8, 32, 17), (E, E, 8, 32, -1), (E, E, True, 32, 2),
                 (E, E[:1], 8, 32, 2), (E.cpu(), E, 8, 32, 2), (E, E[..., :2], 8, 32, 2), (E, E.float(), 8, 32, 2)]:
        with pytest.raises(ValueError):
            ops.detail_gate_u8(*args)


def test_restore_frames_detail_end_to_end():
    """PIL frames in, fp32 alpha in [0, 1], through the geometry: against the definition with ``rint(255 alpha)``, the prepared frames given
    and made on the spot."""
    from anyv2v_amd import prepare
    (sw, sh), (w, h) = (53, 37), (16, 16)
    S = rs.operands("crop-right")[0]
    P = prepare.prepare_frames(tt(S), h, w, "crop", 1, -1, "bicubic", device=DEV).cpu().numpy()
    E = P.copy()
    E[:, :, 8:] = ds.structured("crop-right", "ramp")[0][:, :, 8:]           # the left half unchanged, the right half not
    alpha = torch.from_numpy(np.random.default_rng(11).random((1, h, w), dtype=np.float32))
    alpha[0, :4] = 0.0
    alpha[0, -4:] = 1.0
    dest, box = prepare.restore_geometry((sw, sh), (w, h), "crop", 1, -1)
    A = np.rint(alpha.numpy() * 255.0).astype(np.uint8)
    gates = [ds.gate(E[f], P[f], 6, 40, 1) for f in range(2)]
    assert len({int(v) for g in gates for v in np.unique(g)}) > 4
    want = tt(np.stack([ds.restore_detail(S[f], E[f], P[f], gates[f], dest, box, "bilinear", A[0]) for f in range(2)]))
    kw = dict(fit="crop", x_offset=1, y_offset=-1, resample="bilinear", alpha=alpha, source_resample="bicubic", gate_lo=6, gate_hi=40, gate_radius=1,
              device=DEV)
    pil = lambda x: [Image.fromarray(f) for f in x]
    got = prepare.restore_frames_detail(pil(E), pil(S), pil(P), **kw)
    assert got.is_cuda and got.dtype == torch.uint8 and torch.equal(got.cpu(), want), differ(got.cpu(), want)
    assert torch.equal(prepare.restore_frames_detail(tt(E), tt(S), **kw), got)                     # prepared on the spot: the same frames
    assert torch.equal(prepare.restore_frames_detail(tt(P), tt(S), **kw).cpu(), tt(S))             # an edit that changes nothing
    for bad, word in [(dict(prepared=tt(P)[:, :8]), "prepared"), (dict(alpha=alpha * 2), "alpha"), (dict(gate_lo=40), "lo"), (dict(gate_radius=17), "radius")]:
        with pytest.raises(ValueError, match=word):
            prepare.restore_frames_detail(tt(E), tt(S), **dict(kw, **bad))
