"""The mask-tracking kernels (``anyv2v_amd/csrc/track.hip``) at their edges, through the C ABI: every operand inside poisoned frames at
every byte offset the entry points accept, ``block_match`` at every radius and on inputs made of ties, the luma on all 2^24 inputs, the
median network on all 512 zero-one inputs, the 64-lane count of ``first_frame_mask`` on cells that change in their upper lanes only, and
every refusal of the five entry points with live device buffers.  Every result is integer and compared with ``torch.equal`` against
``tests/track_spec.py``; no case expects a fault: a framed operand lies inside one allocation (``tests/track_edges.py``), so a stray
access shows as a failing assertion."""
import functools

import pytest
import torch

import track_edges as te
import track_spec as spec

pytestmark = pytest.mark.gpu

U8, I16 = torch.uint8, torch.int16


# ------------------------------------------------------------------------------------------------ the C ABI
def _lib():
    from anyv2v_amd import _lib as lib
    return lib, lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t if isinstance(t, int) else t.data_ptr()


def c_luma(rgb, y, dims=None):
    mod, lib = _lib()
    F, H, W = dims or rgb.shape[:3]
    return lib.anyv2v_luma_u8(_ptr(rgb), _ptr(y), F, H, W, _stream())


def c_block_match(y, flow, R, dims=None):
    mod, lib = _lib()
    F, H, W = dims or y.shape
    return lib.anyv2v_block_match_u8(_ptr(y), _ptr(flow), F, H, W, R, _stream())


def c_flow_median(flow, out, dims=None):
    mod, lib = _lib()
    F, h, w = dims or flow.shape[:3]
    return lib.anyv2v_flow_median_i16(_ptr(flow), _ptr(out), F, h, w, _stream())


def c_mask_propagate(mask0, flow, out, dims=None):
    mod, lib = _lib()
    F, H, W = dims or out.shape
    return lib.anyv2v_mask_propagate_u8(_ptr(mask0), _ptr(flow), _ptr(out), F, H, W, _stream())


def c_first_frame_mask(src, ed, mask, thr, cnt, dims=None):
    mod, lib = _lib()
    H, W = dims or mask.shape
    return lib.anyv2v_first_frame_mask_u8(_ptr(src), _ptr(ed), _ptr(mask), H, W, thr, cnt, _stream())


def _ok(rc, what):
    _lib()[0].check(rc, what)


def _match(y, R):
    """``block_match`` on fresh tensors -> the field on the host."""
    F, H, W = y.shape
    flow = torch.full((F, H // 8, W // 8, 2), 0x7E5A, dtype=I16, device="cuda")
    _ok(c_block_match(y.cuda(), flow, R), "anyv2v_block_match_u8")
    return flow.cpu()


def _same(got, want):
    bad = (got != want).reshape(-1)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert torch.equal(got, want), f"{int(bad.sum())} of {bad.numel()} elements differ, first at flat index {bad.nonzero()[:4].reshape(-1).tolist()}"


# ------------------------------------------------------------------------------------------------ 1 .. 5: framed operands
@functools.lru_cache(maxsize=None)
def _luma_case():
    rgb = te.rgb_frames(2, 40, 72, seed=2)
    return rgb, spec.luma(rgb)


@pytest.mark.parametrize("out_offset", [0, 1, 2, 3])
@pytest.mark.parametrize("in_offset", [0, 1, 2, 3])
def test_luma_framed_at_every_byte_offset(in_offset, out_offset):
    """F = 2, 40 x 72: 1440 threads of the four-pixel kernel (a partial last block) at offsets (0, 0), the one-pixel kernel at the other 15."""
    rgb, want = _luma_case()
    te.check_framed(lambda x, y: _ok(c_luma(x, y), "anyv2v_luma_u8"), [(rgb, in_offset)], [(want.shape, U8, out_offset)], [want], "cuda")


@functools.lru_cache(maxsize=None)
def _framed_match_case(R):
    y = te.radius_clip(3, 40, 72, R)
    return y, spec.block_match(y, R)


@pytest.mark.parametrize("offset", [0, 1, 3])
@pytest.mark.parametrize("R", [1, 16, 32])
def test_block_match_framed(R, offset):
    """F = 3, 40 x 72 (5 x 9 cells: partial tiles in both axes, every window clamps somewhere): the luma at three byte offsets, the field
    (4-byte aligned, as the entry point requires) in a frame of its own."""
    y, want = _framed_match_case(R)
    assert te.moves_in_more_than_one_way(want[1]) and not bool(want[0].any())
    te.check_framed(lambda a, f: _ok(c_block_match(a, f, R), "anyv2v_block_match_u8"), [(y, offset)], [(want.shape, I16, 0)], [want], "cuda")


@pytest.mark.parametrize("offset", [0, 2])
@pytest.mark.parametrize("F,h,w", [(2, 5, 9), (2, 1, 7), (2, 6, 1)])
def test_flow_median_framed(F, h, w, offset):
    """5 x 9 cells, then the degenerate grids where every neighbour clamps; int16 extremes among the values."""
    g = torch.Generator().manual_seed(17 + h)
    flow = torch.randint(-32768, 32768, (F, h, w, 2), generator=g).to(I16)
    flow[0].view(-1)[:2] = torch.tensor([-32768, 32767], dtype=I16)
    want = spec.flow_median(flow)
    te.check_framed(lambda a, b: _ok(c_flow_median(a, b), "anyv2v_flow_median_i16"), [(flow, offset)], [(flow.shape, I16, offset)], [want], "cuda")


@pytest.mark.parametrize("offset", [0, 1])
def test_mask_propagate_framed(offset):
    """F = 5, 40 x 72, displacements from {-32768, -33, -1, 0, 1, 33, 32767}: every step clamps somewhere, and a coordinate plus a
    displacement needs more than 16 bits.  The mask (0 / 1 / 255) and the output at ``offset``, the field in a frame of its own."""
    mask0, flow = te.propagate_inputs()
    want = spec.propagate(mask0, flow)
    assert torch.equal(want, spec.propagate_chain(mask0, flow))
    want = want.to(U8)
    te.check_framed(lambda m, f, o: _ok(c_mask_propagate(m, f, o), "anyv2v_mask_propagate_u8"), [(mask0, offset), (flow, 0)],
                    [(want.shape, U8, offset)], [want], "cuda")


@pytest.mark.parametrize("offsets", [(0, 0, 0), (1, 1, 1), (0, 1, 0), (1, 0, 1)], ids=lambda o: "".join(map(str, o)))
def test_first_frame_mask_framed(offsets):
    """24 x 40: 15 cells, a partial last block of four waves."""
    src, ed = te.first_frame_pair(24, 40, seed=8)
    want = spec.first_frame_mask(src, ed, 24, 8)[0].to(U8)
    te.check_framed(lambda a, b, m: _ok(c_first_frame_mask(a, b, m, 24, 8), "anyv2v_first_frame_mask_u8"),
                    [(src, offsets[0]), (ed, offsets[1])], [(want.shape, U8, offsets[2])], [want], "cuda")


# ------------------------------------------------------------------------------------------------ 6: every radius
@pytest.mark.parametrize("R", range(33))
def test_block_match_at_every_radius(R):
    """Every ``groups = R / 2 + 1``, every row pitch ``40 + 4 groups``, every mask ``dx + s <= R`` on the last group of four: F = 2, 24 x 40."""
    y = te.radius_clip(2, 24, 40, R)
    want = spec.block_match(y, R)
    assert R < 2 or te.moves_in_more_than_one_way(want[1])
    _same(_match(y, R), want)


@pytest.mark.parametrize("R", range(1, 33))
def test_block_match_reaches_the_rim_of_the_search_range(R):
    """The winners at dy = -R, dx = R (the last candidate the mask ``dx + s <= R`` lets through) and at dy = R, dx = -R, on a pair where
    one candidate more would win and one fewer would lose (``track_edges.range_end_pair``)."""
    pair = te.range_end_pair()
    got = _match(pair, R)
    _same(got, spec.block_match(pair, R))
    assert got[1, -1, 0].tolist() == [-R, R] and got[1, 0, -1].tolist() == [R, -R]


def test_block_match_default_radius_many_tiles():
    """R = 16 on F = 3, 136 x 72: 17 x 9 cells, a tail tile of one cell in both axes, ``blockIdx.z`` = 2."""
    y = te.radius_clip(3, 136, 72, 16)
    want = spec.block_match(y, 16)
    assert te.moves_in_more_than_one_way(want[1]) and te.moves_in_more_than_one_way(want[2])
    _same(_match(y, 16), want)


# ------------------------------------------------------------------------------------------------ 7, 8: ties and the cost range
@pytest.mark.parametrize("swapped", [False, True], ids=["pair", "swapped"])
@pytest.mark.parametrize("R", [1, 3])
def test_block_match_tie_order_on_a_checkerboard(R, swapped):
    """A one-pixel checkerboard against its inverse, 40 x 48: every displacement of odd parity costs nothing inside the frame, so
    (-1, 0), (0, -1), (0, 1) and (1, 0) tie in cost and in length and the order of (dy, dx) decides: (-1, 0)."""
    pair = te.checkerboard_pair(40, 48, 1, swapped)
    got = _match(pair, R)
    _same(got, spec.block_match(pair, R))
    inner = got[1, 1:-1]
    assert torch.equal(inner, torch.tensor([-1, 0], dtype=I16).expand_as(inner)), "not the first of the four shortest zero-cost vectors"


def test_block_match_tie_order_on_two_pixel_squares():
    pair = te.checkerboard_pair(40, 48, 2)
    _same(_match(pair, 4), spec.block_match(pair, 4))


def test_block_match_largest_cost_next_to_zero_cost():
    """One cell finds a zero-cost window at (5, -6); cells of the same tile that cannot reach it cost 65 280 whatever they try."""
    pair = te.cost_range_pair()
    got = _match(pair, te.COST_R)
    _same(got, spec.block_match(pair, te.COST_R))
    assert got[1][te.COST_CELL].tolist() == list(te.COST_D)
    far = te.cost_out_of_reach()
    assert not bool(got[1][far].any()) and not bool(got[0].any())


# ------------------------------------------------------------------------------------------------ 9: the luma on every input
def test_luma_on_every_input():
    """All 2^24 (R, G, B) in one launch of the four-pixel kernel; the same tensor one byte further on takes the one-pixel kernel."""
    rgb = te.all_rgb("cuda")
    want = spec.luma(rgb.cpu())
    out = torch.zeros(rgb.shape[:3], dtype=U8, device="cuda")
    assert rgb.data_ptr() % 4 == 0 and out.data_ptr() % 4 == 0
    _ok(c_luma(rgb, out), "anyv2v_luma_u8")
    _same(out.cpu(), want)
    odd = torch.zeros(rgb.numel() + 1, dtype=U8, device="cuda")[1:].view(rgb.shape)
    odd.copy_(rgb)
    out.zero_()
    assert odd.data_ptr() % 4 == 1
    _ok(c_luma(odd, out), "anyv2v_luma_u8")
    _same(out.cpu(), want)


# ------------------------------------------------------------------------------------------------ 10: the median network
def test_median_network_on_every_zero_one_input():
    """A selection network is right if and only if it is right on every zero-one input: 512 frames of 3 x 3 cells."""
    flow = te.zero_one_flow()
    out = torch.zeros_like(flow, device="cuda")
    _ok(c_flow_median(flow.cuda(), out), "anyv2v_flow_median_i16")
    got = out.cpu()
    _same(got, spec.flow_median(flow))
    _same(got[:, 1, 1], te.zero_one_majority())


# ------------------------------------------------------------------------------------------------ 11: the count over 64 lanes
@functools.lru_cache(maxsize=None)
def _ballot_case():
    src, ed, lanes = te.ballot_frames()
    return src.cuda(), ed.cuda(), src, ed, lanes.sum(dim=1)


@pytest.mark.parametrize("threshold", [0, 24, 254, 255])
@pytest.mark.parametrize("min_count", [1, 2, 31, 32, 33, 63, 64])
def test_first_frame_mask_counts_all_64_lanes(min_count, threshold):
    """64 x 72: cell c <= 64 changes in exactly c pixels; cells 65 .. 71 change in rows 4 .. 7 only, rows 0 .. 3 only, the last row, the
    first row, and in 7 or 8 pixels of the upper 32 lanes beside 0, 1 and 24 of the lower."""
    dsrc, ded, src, ed, count = _ballot_case()
    H, W = te.BALLOT_HW
    mask = torch.full((H, W), 0xA5, dtype=U8, device="cuda")
    _ok(c_first_frame_mask(dsrc, ded, mask, threshold, min_count), "anyv2v_first_frame_mask_u8")
    got = mask.cpu()
    _same(got, spec.first_frame_mask(src, ed, threshold, min_count)[0].to(U8))
    if threshold == 24:
        cells = got.view(H // 8, 8, W // 8, 8).permute(0, 2, 1, 3).reshape(72, 64)
        assert torch.equal(cells, (count >= min_count).to(U8)[:, None].expand(72, 64)), "a cell is set if and only if its count reaches min_count"
        assert cells[:65, 0].tolist() == [int(c >= min_count) for c in range(65)]


# ------------------------------------------------------------------------------------------------ 12: refusals
def _refused(name, call, outs):
    """``call()`` returns non-zero, the message names the entry point, and after a synchronise the pre-filled outputs are untouched."""
    mod, lib = _lib()
    rc = call()
    msg = lib.anyv2v_last_error()
    assert rc != 0 and name.encode() in msg, (name, rc, msg)
    torch.cuda.current_stream().synchronize()
    for o in outs:
        assert bool((o == 0xA5 if o.dtype == U8 else o == 0x7E5A).all()), f"{name}: a refused call wrote its output ({msg})"
    return msg


BAD_HW = ((12, 24), (16, 20), (0, 24), (16, -8))
BIG = (1 << 10, 1 << 10, 1 << 10)      # 3 F H W = 3 * 2^30: refused before anything reads the (small) buffers


def test_luma_refusals():
    rgb = te.rgb_frames(2, 16, 24, seed=1)
    x, y = rgb.cuda(), torch.full((2, 16, 24), 0xA5, dtype=U8, device="cuda")
    for call, word in [(lambda: c_luma(None, y, (2, 16, 24)), b"null"), (lambda: c_luma(x, None, (2, 16, 24)), b"null"),
                       (lambda: c_luma(x, y, (0, 16, 24)), b"F = "), (lambda: c_luma(x, y, (-1, 16, 24)), b"F = "),
                       (lambda: c_luma(x, y, BIG), b"fit an int")] + [(lambda hw=hw: c_luma(x, y, (2,) + hw), b"multiples of 8") for hw in BAD_HW]:
        assert word in _refused("luma", call, [y])
    _ok(c_luma(x, y), "anyv2v_luma_u8")
    _same(y.cpu(), spec.luma(rgb))


def test_block_match_refusals():
    y = te.radius_clip(2, 16, 24, 4)
    x = y.cuda()
    buf = torch.full((2 * 2 * 3 * 2 + 2,), 0x7E5A, dtype=I16, device="cuda")
    flow, dims = buf[:-2].view(2, 2, 3, 2), (2, 16, 24)
    for call, word in [(lambda: c_block_match(None, flow, 4, dims), b"null"), (lambda: c_block_match(x, None, 4, dims), b"null"),
                       (lambda: c_block_match(x, flow, 4, (0, 16, 24)), b"F = "), (lambda: c_block_match(x, flow, 4, BIG), b"fit an int"),
                       (lambda: c_block_match(x, flow, -1, dims), b"radius"), (lambda: c_block_match(x, flow, 33, dims), b"radius"),
                       (lambda: c_block_match(x, buf[1:-1], 4, dims), b"4-byte aligned"),
                       (lambda: c_block_match(x, flow, 4, (65536, 8, 8)), b"65535")] \
            + [(lambda hw=hw: c_block_match(x, flow, 4, (2,) + hw), b"multiples of 8") for hw in BAD_HW]:
        assert word in _refused("block_match", call, [buf])
    assert buf[1:-1].data_ptr() % 4 == 2
    _ok(c_block_match(x, flow, 4), "anyv2v_block_match_u8")
    _same(flow.cpu(), spec.block_match(y, 4))
    assert bool((buf[-2:] == 0x7E5A).all())


def test_flow_median_refusals():
    g = torch.Generator().manual_seed(4)
    flow = torch.randint(-32, 33, (2, 2, 3, 2), generator=g).to(I16)
    x, out, dims = flow.cuda(), torch.full((2, 2, 3, 2), 0x7E5A, dtype=I16, device="cuda"), (2, 2, 3)
    for call, word in [(lambda: c_flow_median(None, out, dims), b"null"), (lambda: c_flow_median(x, None, dims), b"null"),
                       (lambda: c_flow_median(x, out, (0, 2, 3)), b"F = "), (lambda: c_flow_median(x, out, (2, 0, 3)), b"at least 1"),
                       (lambda: c_flow_median(x, out, (2, 2, -1)), b"at least 1"),
                       (lambda: c_flow_median(x, out, (1 << 12, 1 << 10, 1 << 10)), b"fit an int"),
                       (lambda: c_flow_median(out, out, dims), b"may not alias")]:
        assert word in _refused("flow_median", call, [out])
    _ok(c_flow_median(x, out), "anyv2v_flow_median_i16")
    _same(out.cpu(), spec.flow_median(flow))


def test_mask_propagate_refusals():
    mask0, flow = te.propagate_inputs(2, 16, 24, seed=6)
    m, f, dims = mask0.cuda(), flow.cuda(), (2, 16, 24)
    out = torch.full(dims, 0xA5, dtype=U8, device="cuda")
    as_flow = torch.full((2, 2, 3, 2), 0x7E5A, dtype=I16, device="cuda")      # an output that is also the field argument
    for call, word in [(lambda: c_mask_propagate(None, f, out, dims), b"null"), (lambda: c_mask_propagate(m, None, out, dims), b"null"),
                       (lambda: c_mask_propagate(m, f, None, dims), b"null"), (lambda: c_mask_propagate(m, f, out, (0, 16, 24)), b"F = "),
                       (lambda: c_mask_propagate(m, f, out, BIG), b"fit an int"), (lambda: c_mask_propagate(out, f, out, dims), b"may not alias"),
                       (lambda: c_mask_propagate(m, as_flow, as_flow, dims), b"may not alias")] \
            + [(lambda hw=hw: c_mask_propagate(m, f, out, (2,) + hw), b"multiples of 8") for hw in BAD_HW]:
        assert word in _refused("mask_propagate", call, [out, as_flow])
    _ok(c_mask_propagate(m, f, out), "anyv2v_mask_propagate_u8")
    _same(out.cpu(), spec.propagate(mask0, flow).to(U8))


def test_first_frame_mask_refusals():
    src, ed = te.first_frame_pair(16, 24, seed=3)
    a, b, dims = src.cuda(), ed.cuda(), (16, 24)
    mask = torch.full(dims, 0xA5, dtype=U8, device="cuda")
    as_input = torch.full((16, 24, 3), 0xA5, dtype=U8, device="cuda")          # an output that is also an input argument
    call = lambda s=a, e=b, m=mask, thr=24, cnt=8, d=dims: c_first_frame_mask(s, e, m, thr, cnt, d)
    for kw, word in [(dict(s=None), b"null"), (dict(e=None), b"null"), (dict(m=None), b"null"), (dict(d=(1 << 15, 1 << 15)), b"fit an int"),
                     (dict(thr=-1), b"threshold"), (dict(thr=256), b"threshold"), (dict(cnt=0), b"min_count"), (dict(cnt=65), b"min_count"),
                     (dict(s=as_input, m=as_input), b"may not alias"), (dict(e=as_input, m=as_input), b"may not alias")] \
            + [(dict(d=hw), b"multiples of 8") for hw in BAD_HW]:
        assert word in _refused("first_frame_mask", lambda kw=kw: call(**kw), [mask, as_input])
    _ok(call(), "anyv2v_first_frame_mask_u8")
    _same(mask.cpu(), spec.first_frame_mask(src, ed, 24, 8)[0].to(U8))
