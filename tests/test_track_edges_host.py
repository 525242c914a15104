"""The helpers of the mask-tracking edge tests (``tests/track_edges.py``) without a GPU: the frames report what they are there to
report, ``check_framed`` fails on every kind of wrong launch, and the seeded inputs of ``tests/test_track_edges_gpu.py`` meet the
conditions their tests lean on, evaluated on the definition (``tests/track_spec.py``)."""
import pytest
import torch

import track_edges as te
import track_spec as spec

U8, I16 = torch.uint8, torch.int16


# ------------------------------------------------------------------------------------------------ frames
@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("dtype", [U8, I16], ids=["uint8", "int16"])
def test_frame_reports_a_flipped_element_next_to_the_window(dtype, offset):
    for poison in te.POISON[dtype]:
        f = te.Frame((3, 5), dtype, poison, offset)
        item, lo, hi = f.item, f.lo, f.lo + f.nbytes
        assert f.raw.dtype == U8 and f.raw.dim() == 1 and lo % 4 == offset and f.nbytes == 15 * item
        assert lo >= te.PAD * item and f.raw.numel() - hi >= te.PAD * item, "fewer than PAD poison elements on a side"
        assert f.intact()
        before = f.raw[lo - item:lo].clone().view(dtype)
        after = f.raw[hi:hi + item].clone().view(dtype)
        assert int(before) == int(after) == poison, "the elements next to the window are not whole poison elements"
        f.raw[lo:hi] = 0x33                                          # inside the window anything may change
        assert f.intact()
        for where in (slice(lo - item, lo), slice(hi, hi + item), slice(0, item), slice(f.raw.numel() - item, f.raw.numel())):
            keep = f.raw[where].clone()
            f.raw[where] = keep ^ 0xFF                               # the element flipped
            assert not f.intact(), where
            f.raw[where] = keep
            assert f.intact()
        for at in (lo - 1, hi):                                      # one bit of the nearest byte
            f.raw[at] ^= 0x10
            assert not f.intact(), at
            f.raw[at] ^= 0x10
        if offset % item:
            with pytest.raises(ValueError, match="cannot start"):
                f.view
        else:
            v = f.view
            assert v.dtype == dtype and tuple(v.shape) == (3, 5) and v.is_contiguous() and v.data_ptr() % 4 == offset


def test_framed_copies_the_operand_and_the_poisons_differ_in_every_byte():
    for dtype, (a, b) in te.POISON.items():
        item = torch.empty(0, dtype=dtype).element_size()
        assert all(((a >> (8 * k)) & 0xFF) != ((b >> (8 * k)) & 0xFF) for k in range(item))
        t = torch.arange(24).to(dtype).view(2, 3, 4)
        f = te.framed(t, a, 2)
        assert torch.equal(f.view, t) and f.intact() and f.view.data_ptr() % 4 == 2
        f.view.add_(1)
        assert f.intact() and torch.equal(f.view, t + 1)
    assert (te.POISON[U8], te.POISON[I16]) == ((0xA5, 0x5A), (0x7E5A, -0x7E5A))


def _outside(t, delta):
    """The element ``delta`` places from the start of ``t`` in its storage (a frame's poison when ``t`` is a framed window), or None."""
    at = t.storage_offset() + delta
    whole = torch.empty(0, dtype=t.dtype).set_(t.untyped_storage())
    return whole[at:at + 1] if 0 <= at < whole.numel() else None


def test_check_framed_fails_on_every_kind_of_wrong_launch():
    rgb = te.rgb_frames(1, 8, 8, seed=1)
    want = spec.luma(rgb)
    case = lambda launch, offs=(0, 0): te.check_framed(launch, [(rgb, offs[0])], [(want.shape, U8, offs[1])], [want])

    def right(x, y):
        y.copy_(spec.luma(x))

    for offs in ((0, 0), (1, 3), (2, 1)):
        assert torch.equal(case(right, offs)[0], want)

    def wrong(x, y):
        right(x, y)
        y[0, 0, 0] ^= 1
    with pytest.raises(AssertionError, match="on fresh tensors"):
        case(wrong)

    def reads_before(x, y):                                         # right on a fresh tensor, one element of the frame mixed in otherwise
        right(x, y)
        stray = _outside(x, -1)
        if stray is not None:
            y[0, 0, 0] ^= stray[0]
    with pytest.raises(AssertionError, match="framed with poison A"):
        case(reads_before, (1, 0))

    def reads_after(x, y):
        right(x, y)
        stray = _outside(x, x.numel())
        if stray is not None:
            y[0, -1, -1] ^= stray[0]
    with pytest.raises(AssertionError, match="framed with poison A"):
        case(reads_after)

    def skips_one(x, y):                                            # an element never written keeps the poison
        last = y[0, -1, -1].clone()
        right(x, y)
        if y.storage_offset():
            y[0, -1, -1] = last
    with pytest.raises(AssertionError, match="framed with poison A"):
        case(skips_one)

    for delta, name in ((-1, "before"), (want.numel(), "after")):
        def stores_outside(x, y, delta=delta):
            right(x, y)
            stray = _outside(y, delta)
            if stray is not None:
                stray[0] = 7
        with pytest.raises(AssertionError, match="a store left the window of output 0"):
            case(stores_outside, (0, 2))

    def spoils_input(x, y):
        right(x, y)
        if x.storage_offset():
            x[0, 0, 0, 0] ^= 1
    with pytest.raises(AssertionError, match="input 0 changed"):
        case(spoils_input)

    def spoils_input_frame(x, y):
        right(x, y)
        stray = _outside(x, -3)
        if stray is not None:
            stray[0] = 0
    with pytest.raises(AssertionError, match="the frame of input 0 changed"):
        case(spoils_input_frame)

    flow = torch.randint(-32768, 32768, (2, 3, 4, 2), generator=torch.Generator().manual_seed(1)).to(I16)
    med = spec.flow_median(flow)
    te.check_framed(lambda a, b: b.copy_(spec.flow_median(a)), [(flow, 2)], [(flow.shape, I16, 0)], [med])

    def only_right_under_a(a, b):                                   # what the second poison is for: a value that happens to agree with the first
        b.copy_(spec.flow_median(a))
        stray = _outside(a, -1)
        if stray is not None and int(stray[0]) != te.POISON[I16][0]:
            b.view(-1)[0] += 1
    with pytest.raises(AssertionError, match="framed with poison B"):
        te.check_framed(only_right_under_a, [(flow, 0)], [(flow.shape, I16, 0)], [med])


# ------------------------------------------------------------------------------------------------ the inputs' conditions
def test_radius_clips_move_in_more_than_one_way():
    """For every R >= 2 the definition's field for frame 1 holds two distinct vectors at least, one of them non-zero -- so does every
    clip of the framed and of the many-tile case."""
    for R in range(2, 33):
        field = spec.block_match(te.radius_clip(2, 24, 40, R), R)[1]
        assert te.moves_in_more_than_one_way(field), R
        assert int(field.abs().max()) <= R
    assert not te.moves_in_more_than_one_way(torch.zeros(3, 5, 2, dtype=I16))
    assert not te.moves_in_more_than_one_way(torch.ones(3, 5, 2, dtype=I16))


@pytest.mark.parametrize("R", range(1, 33))
def test_range_end_pair_wins_on_the_rim(R):
    """At every radius the bottom-left cell goes to (-R, R) and the top-right cell to (R, -R) -- and, searched one pixel further, one
    pixel further: a kernel that lost the candidates at the rim, or let one more through, would differ from the definition."""
    pair = te.range_end_pair()
    assert int(pair[0].max()) < 255 and int(pair[0].min()) > 0
    field = spec.block_match(pair, R)[1]
    assert field[-1, 0].tolist() == [-R, R] and field[0, -1].tolist() == [R, -R]
    assert len({tuple(v) for v in field.reshape(-1, 2).tolist()}) >= 3      # (the case R + 1 is the "one pixel further" of the case R)


def test_framed_and_many_tile_clips_move_in_more_than_one_way():
    for R in (1, 16, 32):
        assert te.moves_in_more_than_one_way(spec.block_match(te.radius_clip(3, 40, 72, R), R)[1]), R
    many = spec.block_match(te.radius_clip(3, 136, 72, 16), 16)
    assert te.moves_in_more_than_one_way(many[1]) and te.moves_in_more_than_one_way(many[2])


def test_checkerboards_tie_as_the_tie_tests_assume():
    vec, border = lambda *d: torch.tensor(d, dtype=I16), set()
    for R in (1, 3):
        pair = te.checkerboard_pair(40, 48, 1)
        assert torch.equal(pair[0], 255 - pair[1]) and set(pair.unique().tolist()) == {0, 255}
        assert int(pair[1, 0, 0]) == 0 and int(pair[1, 0, 1]) == 255 and int(pair[1, 1, 0]) == 255
        field = spec.block_match(pair, R)
        assert torch.equal(field[1, 1:-1], vec(-1, 0).expand(3, 6, 2)), "the four vectors of length 1 tie; (-1, 0) is the first in order"
        assert torch.equal(spec.block_match(te.checkerboard_pair(40, 48, 1, swapped=True), R), field)
        border |= {tuple(v) for v in torch.cat([field[1, 0], field[1, -1]]).tolist()}
    assert border == {(0, 1), (0, -1), (-3, 0), (0, 3), (0, -3), (-1, 0)}, "the clamped border rows: other winners, the definition covers them"
    two = te.checkerboard_pair(40, 48, 2)
    assert torch.equal(two[1, :4, :4], torch.tensor([[0, 0, 255, 255]] * 2 + [[255, 255, 0, 0]] * 2, dtype=U8))
    inner = {tuple(v) for v in spec.block_match(two, 4)[1, 1:-1].reshape(-1, 2).tolist()}
    assert inner == {(-2, 0)}, inner


def test_cost_range_pair_holds_both_ends_in_one_tile():
    pair, far = te.cost_range_pair(), te.cost_out_of_reach()
    field = spec.block_match(pair, te.COST_R)
    assert field[1][te.COST_CELL].tolist() == list(te.COST_D) and not bool(field[0].any())
    assert not bool(field[1][far].any()) and int(far.sum()) >= 8
    ty, tx = te.COST_CELL[0] // 4 * 4, te.COST_CELL[1] // 4 * 4
    assert bool(far[ty:ty + 4, tx:tx + 4].any()), "no cell of the tile costs 65 280 throughout"
    near = field[1][~far]
    assert bool(near.any()), "cells that reach the square in part move too: the comparison with the definition covers them"
    # the two costs themselves, from the definition's formula: 0 at COST_D for COST_CELL, 255 * 256 for a cell out of reach
    top, left = 8 * te.COST_CELL[0] - 4, 8 * te.COST_CELL[1] - 4
    win = pair[1, top:top + 16, left:left + 16].long()
    assert int((win - pair[0, top + te.COST_D[0]:top + te.COST_D[0] + 16, left + te.COST_D[1]:left + te.COST_D[1] + 16].long()).abs().sum()) == 0
    assert int((pair[1, :16, :16].long() - pair[0, :16, :16].long()).abs().sum()) == 65280 and bool(far[0, 0])


def test_all_rgb_holds_every_triple_once():
    rgb = te.all_rgb()
    assert rgb.dtype == U8 and tuple(rgb.shape) == (1, 4096, 4096, 3)
    v = rgb.view(-1, 3).long()
    code = (v[:, 0] << 16) | (v[:, 1] << 8) | v[:, 2]
    assert bool((torch.bincount(code, minlength=1 << 24) == 1).all())
    assert bool((v[1:] != v[:-1]).all(dim=1).float().mean() > 0.98), "neighbouring pixels share channels: a mixed-up byte could go unseen"
    assert tuple(spec.luma(rgb[:, :1]).shape) == (1, 1, 4096)


def test_zero_one_flow_and_its_majority():
    flow, major = te.zero_one_flow(), te.zero_one_majority()
    assert flow.dtype == I16 and tuple(flow.shape) == (512, 3, 3, 2)
    assert len({tuple(f.reshape(-1).tolist()) for f in flow[..., 0]}) == 512, "every zero-one input once"
    for i in (0, 1, 0b101010101, 0b000010000, 511):
        bits = [(i >> j) & 1 for j in range(9)]
        assert flow[i, :, :, 0].reshape(-1).tolist() == [9 if b else -7 for b in bits]
        assert flow[i, :, :, 1].reshape(-1).tolist() == [-32768 if b else 32767 for b in bits], "component 1: the complement pattern"
        assert major[i].tolist() == [9 if sum(bits) >= 5 else -7, 32767 if 9 - sum(bits) >= 5 else -32768]
    assert torch.equal(spec.flow_median(flow)[:, 1, 1], major)


def test_propagate_inputs_clamp_and_overflow_16_bits():
    mask0, flow = te.propagate_inputs()
    assert tuple(flow.shape) == (5, 5, 9, 2) and set(mask0.unique().tolist()) == {0, 1, 255}
    for k in range(1, 5):
        for c in range(2):
            assert set(flow[k, ..., c].unique().tolist()) == set(te.PROPAGATE_VALUES), (k, c)
    # every step of the chain clamps somewhere, and somewhere a coordinate plus a displacement leaves the int16 range
    H, W = 40, 72
    py, px = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    for k in range(4, 0, -1):
        qy, qx = py.clone(), px.clone()
        for j in range(k, 0, -1):
            d = flow[j].long()[qy // 8, qx // 8]
            ny, nx = qy + d[..., 0], qx + d[..., 1]
            assert bool(((ny < 0) | (ny >= H) | (nx < 0) | (nx >= W)).any()), (k, j)
            if j == k:
                assert int(ny.max()) > 32767 and int(nx.max()) > 32767 and int(ny.min()) <= -32768
            qy, qx = ny.clamp(0, H - 1), nx.clamp(0, W - 1)
    want = spec.propagate(mask0, flow)
    assert torch.equal(want, spec.propagate_chain(mask0, flow))
    for k in range(5):
        assert 0 < int(want[k].sum()) < H * W, k
    assert not torch.equal(want[4], want[0])


def test_first_frame_pair_gives_a_mixed_mask():
    for hw, seed in (((24, 40), 8), ((16, 24), 3)):
        m = spec.first_frame_mask(*te.first_frame_pair(*hw, seed=seed), 24, 8)
        assert 0 < int(m.sum()) < m.numel(), hw


def test_ballot_frames_hold_the_counts_they_name():
    src, ed, lanes = te.ballot_frames()
    H, W = te.BALLOT_HW
    assert tuple(src.shape) == (H, W, 3) and tuple(lanes.shape) == (72, 64)
    count = lanes.sum(dim=1)
    assert count[:65].tolist() == list(range(65))
    upper, lower = lanes[:, 32:].sum(dim=1), lanes[:, :32].sum(dim=1)
    assert list(zip(upper[65:].tolist(), lower[65:].tolist())) == [(8, 0), (0, 8), (8, 0), (0, 8), (7, 0), (7, 1), (8, 24)]
    assert bool(lanes[67, 56:].all()) and bool(lanes[68, :8].all()) and bool(lanes[67, 63]) and bool(lanes[68, 0])
    assert int((lanes[:65, 32:].sum(dim=1) > 0).sum()) >= 60
    diff = (ed.long() - src.long()).abs().amax(dim=-1)
    cells = lambda plane: plane.view(H // 8, 8, W // 8, 8).permute(0, 2, 1, 3).reshape(72, 64)
    assert torch.equal(cells(diff == 255), lanes) and set(diff.unique().tolist()) == {0, 24, 255}
    assert bool((ed[cells_to_pixels(lanes, H, W)] != src[cells_to_pixels(lanes, H, W)]).sum(dim=-1).eq(1).all()), "one channel per changed pixel"
    for thr, over in ((0, cells(diff > 0)), (24, lanes), (254, lanes), (255, torch.zeros_like(lanes))):
        for cnt in (1, 2, 31, 32, 33, 63, 64):
            want = cells(spec.first_frame_mask(src, ed, thr, cnt)[0])
            assert torch.equal(want, (over.sum(dim=1) >= cnt)[:, None].expand(72, 64)), (thr, cnt)
    # a count over the lower 32 lanes alone would differ from the definition at every min_count of the test
    for cnt in (1, 2, 31, 32, 33, 63, 64):
        assert not torch.equal(lower >= cnt, count >= cnt), cnt


def cells_to_pixels(lanes, H, W):
    return lanes.view(H // 8, W // 8, 8, 8).permute(0, 2, 1, 3).reshape(H, W)
