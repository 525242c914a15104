"""Cost of taking a 16-frame 512 x 512 edit back to its 1920 x 1080 source (``fit="crop"``, lanczos) for profiles/restore_cost.md: the
horizontal passes of the edit and of alpha and the paste launch of ``ops.restore_u8`` separately and together, with and without alpha
(device events, warm-up, median of 20), beside a plain device copy of the same 16 x 1080 x 1920 x 3 bytes; the result of frame 0 is
compared with Pillow's byte for byte.  Needs a GPU.

    python tools/restore_cost.py [--out FILE.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from anyv2v_amd import _lib, ops, prepare  # noqa: E402
from tools.prepare_cost import med_ms  # noqa: E402


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument("--out", default=None)
    args = parser.parse_args()
    assert torch.cuda.is_available(), "restore_cost.py measures on the GPU"
    lib = _lib.load()
    F, h, w, sh, sw = 16, 512, 512, 1080, 1920
    dest, box = prepare.restore_geometry((sw, sh), (w, h), "crop")
    dw = dest[2] - dest[0]
    res = {"device": torch.cuda.get_device_name(0), "geometry": [list(dest), list(box)]}
    rng = np.random.default_rng(0)
    S = torch.from_numpy(rng.integers(0, 256, (F, sh, sw, 3), dtype=np.uint8)).cuda()
    E = torch.from_numpy(rng.integers(0, 256, (F, h, w, 3), dtype=np.uint8)).cuda()
    A = torch.from_numpy(rng.integers(0, 256, (F, h, w), dtype=np.uint8)).cuda()
    pe, pa = (tuple(None if t is None else (t if not isinstance(t, tuple) else (t[0], t[1].cuda(), t[2].cuda())) for t in p)
              for p in ops.restore_passes(h, w, dest, box, "lanczos"))
    res["passes"] = {"edit": {"rows": pe[1], "ksize_h": pe[2][0] if pe[2] else None, "ksize_v": pe[3][0]},
                     "alpha": {"rows": pa[1], "ksize_h": pa[2][0] if pa[2] else None, "ksize_v": pa[3][0]}}

    def horizontal(x, p, y):
        _lib.check(lib.anyv2v_resample_h_u8(x.data_ptr(), y.data_ptr(), x.shape[0], h, w, x.shape[3], p[0], p[1], dw, p[2][1].data_ptr(),
                                            p[2][2].data_ptr(), p[2][0], ops._stream()), "anyv2v_resample_h_u8")
    eh = torch.empty((F, pe[1], dw, 3), dtype=torch.uint8, device="cuda")
    ah = torch.empty((F, pa[1], dw, 1), dtype=torch.uint8, device="cuda")
    out = torch.empty_like(S)
    res["h_edit_ms"] = med_ms(lambda: horizontal(E, pe, eh), 20)
    res["h_alpha_ms"] = med_ms(lambda: horizontal(A[..., None], pa, ah), 20)
    res["paste_no_alpha_ms"] = med_ms(lambda: ops.restore_paste_u8(S, eh, None, dest, pe[3], out=out), 20)
    res["paste_alpha_ms"] = med_ms(lambda: ops.restore_paste_u8(S, eh, ah[..., 0], dest, pe[3], pa[3], out=out), 20)
    res["restore_u8_no_alpha_ms"] = med_ms(lambda: ops.restore_u8(E, S, dest, box, "lanczos"), 20)
    res["restore_u8_alpha_ms"] = med_ms(lambda: ops.restore_u8(E, S, dest, box, "lanczos", A), 20)
    res["device_copy_ms"] = med_ms(lambda: out.copy_(S), 20)
    res["bytes_frame"] = int(S.numel())
    res["bytes_intermediates"] = [int(eh.numel()), int(ah.numel())]
    for name, a in (("no_alpha", None), ("alpha", A)):
        got = ops.restore_u8(E, S, dest, box, "lanczos", a)[0].cpu().numpy()
        want = Image.fromarray(S[0].cpu().numpy())
        e = Image.fromarray(E[0].cpu().numpy()).resize((dw, dest[3] - dest[1]), Image.Resampling.LANCZOS, box=box)
        m = None if a is None else Image.fromarray(a[0].cpu().numpy(), mode="L").resize((dw, dest[3] - dest[1]), Image.Resampling.BILINEAR, box=box)
        want.paste(e, (dest[0], dest[1]), mask=m)
        res[f"equal_to_pillow_{name}"] = bool(np.array_equal(got, np.asarray(want)))
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
