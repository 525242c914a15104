"""TEST-ONLY restatement of FreeU (arXiv 2309.11497) as ``I2VGenXLUNet.enable_freeu`` means it -- a helper, not a test file.

In the decoder, before every ``torch.cat([hidden, skip], 1)`` that feeds a ResNet of ``up_blocks[r]``, r = 0 ((b, s) = (b1, s1)) and
r = 1 ((b2, s2)) only:  ``hidden[:, : C_hidden // 2] *= b``;  ``skip = fourier_filter(skip, threshold=1, scale=s)`` per 4-D image
[N, C, H, W] in fp32 -- fftn over (H, W), fftshift, the box ``[H//2-1 : H//2+1, W//2-1 : W//2+1]`` times s, ifftshift, ifftn, real part.

Here: that definition with ``torch.fft`` (CPU only); its closed form in plain torch (the box holds the frequencies {0, -1} of each
axis, {0} on an axis of size 1, where the Python slice wraps); a CPU emulation of ``ops.freeu`` on top of ``cpu_ops_emulation``; and
``hook_oracle``, which gives the oracle UNet FreeU through forward pre-hooks without editing ``oracle/``.
"""
from __future__ import annotations

import math

import torch


def fourier_filter_fft(x: torch.Tensor, scale: float, threshold: int = 1) -> torch.Tensor:
    """The definition, [N, C, H, W] in the dtype of ``x`` (fp32 / fp64)."""
    H, W = x.shape[-2:]
    xf = torch.fft.fftshift(torch.fft.fftn(x, dim=(-2, -1)), dim=(-2, -1))
    mask = torch.ones(x.shape[-2:], dtype=x.dtype)
    mask[H // 2 - threshold: H // 2 + threshold, W // 2 - threshold: W // 2 + threshold] = scale
    return torch.fft.ifftn(torch.fft.ifftshift(xf * mask, dim=(-2, -1)), dim=(-2, -1)).real


def fourier_filter_closed(x: torch.Tensor, scale: float) -> torch.Tensor:
    """y = x + (s - 1) / (H W) sum_{k in Kh x Kw} [(sum x cos phi_k) cos phi_k + (sum x sin phi_k) sin phi_k],
    phi_k(h, w) = 2 pi (k_h h / H + k_w w / W), Kh = {0, -1} if H >= 2 else {0}, Kw likewise.  Plain torch, any device, dtype of ``x``."""
    H, W = x.shape[-2:]
    a = (2 * math.pi / H) * torch.arange(H, dtype=x.dtype, device=x.device)[:, None]
    b = (2 * math.pi / W) * torch.arange(W, dtype=x.dtype, device=x.device)[None, :]
    corr = torch.zeros_like(x)
    for kh in ((0, -1) if H >= 2 else (0,)):
        for kw in ((0, -1) if W >= 2 else (0,)):
            phi = kh * a + kw * b
            c, s = torch.cos(phi), torch.sin(phi)
            corr = corr + (x * c).sum((-2, -1), keepdim=True) * c + (x * s).sum((-2, -1), keepdim=True) * s
    return x + ((scale - 1.0) / (H * W)) * corr


def freeu_pair(hidden: torch.Tensor, skip: torch.Tensor, b: float, s: float, fourier=None):
    """The definition on NCHW tensors of any float dtype: fp32 arithmetic, cast back.  ``fourier``: the filter, by default
    ``torch.fft`` on the CPU and the closed form elsewhere (torch.fft is called on the CPU only)."""
    if fourier is None:
        fourier = fourier_filter_closed if skip.is_cuda else fourier_filter_fft
    half = hidden.shape[1] // 2
    hidden = torch.cat([(hidden[:, :half].float() * b).to(hidden.dtype), hidden[:, half:]], 1)
    return hidden, fourier(skip.float(), s).to(skip.dtype)


def freeu_tokens_reference(hidden: torch.Tensor, skip: torch.Tensor, n_img: int, H: int, W: int, b: float, s: float, dtype=torch.float64):
    """``ops.freeu``'s contract on token matrices [n_img H W, C] (CPU): (hidden' in fp16, exact; skip' un-rounded in ``dtype``)."""
    half = hidden.shape[1] // 2
    ho = hidden.clone()
    ho[:, :half] = (hidden[:, :half].float() * b).half()
    xs = skip.to(dtype).view(n_img, H, W, skip.shape[1]).permute(0, 3, 1, 2)
    return ho, fourier_filter_fft(xs, s).permute(0, 2, 3, 1).reshape(skip.shape)


def emulated_freeu(hidden, skip, n_img, H, W, b, s, out=None):
    """CPU emulation of ``anyv2v_amd.ops.freeu``: the torch.fft definition in fp32, one fp16 rounding."""
    ho, so = freeu_tokens_reference(hidden, skip, n_img, H, W, b, s, dtype=torch.float32)
    so = so.half()
    if out is not None:
        out[0].copy_(ho)
        out[1].copy_(so)
        return out
    return ho, so


def install(monkeypatch=None):
    """``cpu_ops_emulation.install`` plus ``ops.freeu`` (tests only)."""
    import cpu_ops_emulation as emu
    from anyv2v_amd import ops
    emu.install(monkeypatch)
    if monkeypatch is not None:
        monkeypatch.setattr(ops, "freeu", emulated_freeu, raising=False)
    else:
        ops.freeu = emulated_freeu


def hook_oracle(oracle_unet, s1, s2, b1, b2):
    """FreeU on the oracle UNet: forward pre-hooks on ``up_blocks[0 / 1].resnets[i]`` split the already concatenated input at
    in_channels - skip_channels (the backbone's channels: the previous block's output for i = 0, this block's for i > 0) and
    apply the definition.  Returns the hook handles (``h.remove()`` undoes it)."""
    handles = []
    prev_out = oracle_unet.mid_block.resnets[-1].conv2.out_channels
    for r, (b, s) in enumerate(((b1, s1), (b2, s2))):
        blk = oracle_unet.up_blocks[r]
        for i, res in enumerate(blk.resnets):
            c_hidden = prev_out if i == 0 else res.conv2.out_channels

            def pre(mod, args, c_hidden=c_hidden, b=b, s=s):
                x = args[0]
                assert 0 < c_hidden < x.shape[1]
                hidden, skip = freeu_pair(x[:, :c_hidden], x[:, c_hidden:], b, s)
                return (torch.cat([hidden, skip], 1),) + tuple(args[1:])
            handles.append(res.register_forward_pre_hook(pre))
        prev_out = blk.resnets[-1].conv2.out_channels
    return handles
