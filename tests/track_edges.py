"""TEST-ONLY helpers of the mask-tracking edge tests (``tests/test_track_edges_host.py`` proves them on the CPU,
``tests/test_track_edges_gpu.py`` uses them on the kernels of ``anyv2v_amd/csrc/track.hip``): operands of one or two bytes per element
inside poisoned frames, the three-run check built on them, and the seeded inputs whose conditions the host file asserts.  Nothing here
knows a kernel: a launch is any callable that takes the input tensors followed by the output tensors."""
from __future__ import annotations

import torch

PAD = 4096                                                                     # poison elements before and after every window, at least
POISON = {torch.uint8: (0xA5, 0x5A), torch.int16: (0x7E5A, -0x7E5A)}           # A, B: no byte of A equals the byte of B in its place


class Frame:
    """A contiguous window of ``numel`` elements of ``dtype`` inside one larger 1-D byte buffer ``raw``.  Every element outside the window
    holds ``poison``, counted from the window's two ends (so the element directly before and the one directly after it are whole poison
    elements at any offset); at least ``PAD`` of them on either side.  The window starts ``offset`` bytes (0 .. 3) behind a 4-byte
    boundary.  ``intact()`` compares every byte outside the window with what was put there."""

    def __init__(self, shape, dtype, poison, offset=0, device="cpu"):
        assert dtype in POISON and 0 <= offset <= 3 and -(1 << 15) <= poison < (1 << 16), (dtype, offset, poison)
        self.shape, self.dtype, self.offset = tuple(shape), dtype, offset
        self.item = torch.empty(0, dtype=dtype).element_size()
        self.nbytes = self.item * int(torch.Size(self.shape).numel())
        self.lo = PAD * self.item + offset                                         # PAD * item is a multiple of 4
        total = self.lo + self.nbytes + PAD * self.item + (4 - offset)
        pattern = torch.tensor([(poison >> (8 * b)) & 0xFF for b in range(self.item)], dtype=torch.uint8)       # little-endian
        self.expected = pattern[(torch.arange(total) - self.lo) % self.item].to(device)
        self.raw = self.expected.clone()
        assert self.raw.data_ptr() % 4 == 0, "the allocation itself is not 4-byte aligned"

    @property
    def view(self):
        """The window as a tensor of the operand's dtype and shape (pre-filled with the poison until something is copied in)."""
        if self.offset % self.item:
            raise ValueError(f"a window of {self.dtype} cannot start {self.offset} bytes behind a 4-byte boundary")
        v = self.raw[self.lo:self.lo + self.nbytes].view(self.dtype).view(self.shape)
        assert v.data_ptr() % 4 == self.offset
        return v

    def intact(self):
        hi = self.lo + self.nbytes
        return bool(torch.equal(self.raw[:self.lo], self.expected[:self.lo]) and torch.equal(self.raw[hi:], self.expected[hi:]))


def framed(t, poison, offset=0, device=None):
    """``t`` (uint8 or int16) copied into a frame on ``device`` (default: its own)."""
    f = Frame(t.shape, t.dtype, poison, offset, t.device if device is None else device)
    f.view.copy_(t)
    return f


def check_framed(launch, ins, outs, want, device="cpu"):
    """One framed case, three runs with the same arguments: on fresh tensors, then framed with poison A, then framed with poison B.
    ``ins``: (host tensor, byte offset) each; ``outs``: (shape, dtype, byte offset) each; ``want``: the definition's results;
    ``launch(*inputs, *outputs)``.  Framed outputs start as poison.  Asserted: both framed results equal the definition, both equal the
    plain result, every frame (inputs' included) is intact, no input changed.  A read that reached poison cannot give the same answer
    under A and B unless it was discarded.  Returns the plain results."""
    fresh_in = [t.to(device) for t, _ in ins]
    fresh_out = [torch.zeros(shape, dtype=dtype, device=device) for shape, dtype, _ in outs]
    launch(*fresh_in, *fresh_out)
    plain = [o.cpu() for o in fresh_out]
    for i, (p, w) in enumerate(zip(plain, want)):
        assert p.dtype == w.dtype and torch.equal(p, w), f"output {i} on fresh tensors: {_differ(p, w)}"
    for which, name in enumerate("AB"):
        fin = [framed(t, POISON[t.dtype][which], off, device) for t, off in ins]
        fout = [Frame(shape, dtype, POISON[dtype][which], off, device) for shape, dtype, off in outs]
        launch(*[f.view for f in fin], *[f.view for f in fout])
        got = [f.view.cpu() for f in fout]
        for i, (g, w, p) in enumerate(zip(got, want, plain)):
            assert torch.equal(g, w), f"output {i} framed with poison {name}: {_differ(g, w)}"
            assert torch.equal(g, p), f"output {i} framed with poison {name} is not the result on fresh tensors: {_differ(g, p)}"
        for i, f in enumerate(fin):
            assert f.intact(), f"poison {name}: the frame of input {i} changed"
            assert torch.equal(f.view.cpu(), ins[i][0]), f"poison {name}: input {i} changed"
        for i, f in enumerate(fout):
            assert f.intact(), f"poison {name}: a store left the window of output {i}"
    return plain


def _differ(got, want):
    bad = (got != want).reshape(-1)
    return f"{int(bad.sum())} of {bad.numel()} elements differ from the expected, first at flat index {bad.nonzero()[:4].reshape(-1).tolist()}"


# ------------------------------------------------------------------------------------------------ seeded inputs
def rgb_frames(F, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    rgb = torch.randint(0, 256, (F, H, W, 3), generator=g, dtype=torch.uint8)
    rgb[0, 0, :4] = torch.tensor([[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 0, 255]], dtype=torch.uint8)
    return rgb


RADIUS_SEED = 3      # (tests/test_track_edges_host.py asserts what the radius tests need of the clips of this seed)


def radius_clip(F, H, W, R):
    """The clip of the every-radius tests: a global drift of (2, -3) per frame, (1, -1) in the right half, one texture per radius."""
    from test_track_host import moving_clip
    return moving_clip(F, H, W, seed=RADIUS_SEED + R, smooth=1)


def moves_in_more_than_one_way(field):
    """What the radius tests need of the definition's field for frame 1: two distinct vectors at least, one of them non-zero."""
    return bool(field.any()) and len({tuple(v) for v in field.reshape(-1, 2).tolist()}) >= 2


RANGE_END_HW = (32, 40)


def range_end_pair():
    """A pair whose best displacements lie on the rim of every search range R <= 32 (the clips above drift by a few pixels whatever R is,
    so a candidate lost or gained at dx = R would not show on them).  Y_0 brightens to the right and to the top; Y_1 is 255 in its left
    half and 0 in its right half, so a left cell's cost falls with every step right and up, a right cell's with every step left and
    down, as long as one pixel of the displaced window is not clamped: the bottom-left cell goes to (-R, R), the top-right cell to
    (R, -R), and a search that reached one candidate further would go further."""
    H, W = RANGE_END_HW
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    y0 = (2 * xx + 3 * (H - 1 - yy) + 10).to(torch.uint8)
    y1 = torch.zeros(H, W, dtype=torch.uint8)
    y1[:, :W // 2] = 255
    return torch.stack([y0, y1])


def checkerboard_pair(H, W, size=1, swapped=False):
    """Y_1 = a checkerboard of ``size``-pixel squares (0 / 255), Y_0 = its inverse (``swapped``: the other way round) -> uint8 [2, H, W].
    Every displacement with (dy // size + dx // size) odd costs nothing where no window clamps."""
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    y1 = (((yy // size + xx // size) & 1) * 255).to(torch.uint8)
    y0 = 255 - y1
    return torch.stack([y1, y0] if swapped else [y0, y1])


COST_CELL, COST_D, COST_R, COST_HW = (3, 4), (5, -6), 8, (64, 64)


def cost_range_pair():
    """Y_1 all 0; Y_0 all 255 but for a 16 x 16 square of zeros at ``COST_D`` from the window of cell ``COST_CELL``.  At ``COST_D`` that
    cell costs 0; a cell whose search cannot reach the square costs 65 280 at every displacement (-> the zero vector), and the tile of
    ``COST_CELL`` holds such cells.  (Y_0 is the frame that carries the square: the cost compares Y_1[p] with Y_0[p + d], so against a
    constant Y_0 no displacement would change any cost.)"""
    H, W = COST_HW
    y0 = torch.full((H, W), 255, dtype=torch.uint8)
    top, left = 8 * COST_CELL[0] - 4 + COST_D[0], 8 * COST_CELL[1] - 4 + COST_D[1]
    assert 0 <= top and top + 16 <= H and 0 <= left and left + 16 <= W
    y0[top:top + 16, left:left + 16] = 0
    return torch.stack([y0, torch.zeros(H, W, dtype=torch.uint8)])


def cost_out_of_reach():
    """bool [h, w]: cells none of whose candidate windows touches the square of ``cost_range_pair``."""
    H, W = COST_HW
    cy, cx = torch.arange(H // 8), torch.arange(W // 8)
    oy, ox = COST_D[0] - 8 * (cy - COST_CELL[0]), COST_D[1] - 8 * (cx - COST_CELL[1])      # the square seen from each cell's window
    return ((oy.abs() - COST_R >= 16)[:, None]) | ((ox.abs() - COST_R >= 16)[None, :])


ALL_RGB_STEP = 0x9E3779      # odd: i -> i * step mod 2^24 is a bijection, and neighbouring pixels differ in all three channels


def all_rgb(device="cpu"):
    """uint8 [1, 4096, 4096, 3] holding every (R, G, B) exactly once, pixel i the triple number ``i * ALL_RGB_STEP mod 2^24``."""
    v = (torch.arange(1 << 24, dtype=torch.int64, device=device) * ALL_RGB_STEP) & 0xFFFFFF
    return torch.stack([v >> 16, (v >> 8) & 255, v & 255], dim=-1).to(torch.uint8).view(1, 4096, 4096, 3)


MEDIAN_VALUES = ((-7, 9), (32767, -32768))      # (value of a 0 bit, value of a 1 bit) per component: component 1 carries the complement


def zero_one_flow():
    """int16 [512, 3, 3, 2]: frame i carries bit j of i at cell j (row j // 3, column j % 3)."""
    bits = (torch.arange(512)[:, None] >> torch.arange(9)[None, :]) & 1
    comps = [torch.where(bits == 1, hi, lo) for lo, hi in MEDIAN_VALUES]
    return torch.stack(comps, dim=-1).to(torch.int16).view(512, 3, 3, 2)


def zero_one_majority():
    """int16 [512, 2]: what the centre cell of each frame of ``zero_one_flow`` must become, from the count of its bits alone."""
    ones = ((torch.arange(512)[:, None] >> torch.arange(9)[None, :]) & 1).sum(dim=1)
    return torch.stack([torch.where(ones >= 5, hi, lo) for lo, hi in MEDIAN_VALUES], dim=-1).to(torch.int16)


PROPAGATE_VALUES = (-32768, -33, -1, 0, 1, 33, 32767)


def propagate_inputs(F=5, H=40, W=72, seed=13):
    """(mask0 uint8 [H, W] of 0 / 1 / 255, flow int16 [F, h, w, 2] drawn from ``PROPAGATE_VALUES``)."""
    g = torch.Generator().manual_seed(seed)
    values = torch.tensor(PROPAGATE_VALUES, dtype=torch.int16)
    flow = values[torch.randint(0, len(values), (F, H // 8, W // 8, 2), generator=g)]
    mask0 = (torch.rand(H, W, generator=g) < 0.4).to(torch.uint8) * torch.where(torch.rand(H, W, generator=g) < 0.5, 1, 255).to(torch.uint8)
    return mask0, flow


def first_frame_pair(H, W, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
    b = torch.where(torch.rand(H, W, 1, generator=g) < 0.12, torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8), a)
    return a, b


BALLOT_HW = (64, 72)
# cells 65 .. 71 as (lanes to draw from, how many): 8 in rows 4 .. 7 only; 8 in rows 0 .. 3 only; the last row (lanes 56 .. 63); the first
# row (lanes 0 .. 7); 7 in the upper lanes and nothing else; 7 there and 1 below; 8 there and 24 below
BALLOT_EXTRA = (((range(32, 64), 8),), ((range(0, 32), 8),), ((range(56, 64), 8),), ((range(0, 8), 8),), ((range(32, 64), 7),),
                ((range(32, 64), 7), (range(0, 32), 1)), ((range(32, 64), 8), (range(0, 32), 24)))


def ballot_lanes(seed=21):
    """bool [72, 64]: the lanes (row * 8 + column of the cell's pixels) that change, per cell: cell c <= 64 has c of them at seeded places."""
    g = torch.Generator().manual_seed(seed)
    lanes = torch.zeros(72, 64, dtype=torch.bool)
    for c in range(65):
        lanes[c, torch.randperm(64, generator=g)[:c]] = True
    for c, parts in enumerate(BALLOT_EXTRA, start=65):
        for pool, count in parts:
            pool = torch.tensor(list(pool))
            lanes[c, pool[torch.randperm(len(pool), generator=g)[:count]]] = True
    return lanes


def ballot_frames(seed=21):
    """(source, edited uint8 [64, 72, 3], lanes): a changed pixel differs by 255 in one seeded channel (upwards or downwards), every other
    pixel by 0 or by exactly 24 -- over a threshold of 0 only."""
    H, W = BALLOT_HW
    lanes = ballot_lanes(seed)
    g = torch.Generator().manual_seed(seed + 1)
    changed = lanes.view(H // 8, W // 8, 8, 8).permute(0, 2, 1, 3).reshape(H, W)
    channel = torch.nn.functional.one_hot(torch.randint(0, 3, (H, W), generator=g), 3).bool()
    up = torch.rand(H, W, generator=g) < 0.5
    quiet = torch.randint(0, 232, (H, W, 3), generator=g)                                # both frames where nothing happens
    near = torch.where(torch.rand(H, W, generator=g) < 0.5, 24, 0)                      # 0 or 24 in the seeded channel
    src = torch.where(changed[..., None] & channel, torch.where(up, 0, 255)[..., None], quiet)
    ed = torch.where(changed[..., None] & channel, torch.where(up, 255, 0)[..., None], quiet + near[..., None] * channel)
    return src.to(torch.uint8), ed.to(torch.uint8), lanes
