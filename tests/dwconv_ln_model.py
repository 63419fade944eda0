"""fp64 model of the training ResBlock front (include/paella_hip.h "Training ResBlock front"): [cat with the skip ->] depthwise 3x3 with zero padding + bias ->
LayerNorm over the channels, NHWC, forward and the closed-form backward.  The convolution is written as explicit sums over shifted slices -- no F.conv2d, no autograd.
Plain torch on whatever device the inputs live on; shared by tests/test_dwconv_train.py (against torch's own autograd) and tests/test_gpu_dwconv_train.py (against
the HIP op)."""
import torch

EPS = 1e-6


def _cat(x, skip):
    """x, skip [B, H, W, C] -> xcat [B, H, W, J C] in fp64"""
    return x.double() if skip is None else torch.cat([x.double(), skip.double()], dim=-1)


def _shifted(t, oy, ox):
    """s[b, y, x] = t[b, y + oy, x + ox], 0 outside the image; t [B, H, W, ...]"""
    B, H, W = t.shape[:3]
    s = torch.zeros_like(t)
    y0, y1 = max(0, -oy), min(H, H - oy)
    x0, x1 = max(0, -ox), min(W, W - ox)
    if y0 < y1 and x0 < x1:
        s[:, y0:y1, x0:x1] = t[:, y0 + oy:y1 + oy, x0 + ox:x1 + ox]
    return s


def forward(x, skip, w, bias, eps=EPS):
    """x, skip (or None) [B, H, W, C]; w [C, J, 3, 3]; bias [C] -> (y [B, H, W, C], rstd [B, H, W]) in fp64"""
    xc = _cat(x, skip)
    C, J = w.size(0), w.size(1)
    assert xc.size(-1) == J * C
    w = w.double()
    a = bias.double().view(1, 1, 1, C).expand(*xc.shape[:3], C).clone()
    for ky in range(3):
        for kx in range(3):
            s = _shifted(xc, ky - 1, kx - 1)
            for j in range(J):
                a = a + s[..., j::J] * w[:, j, ky, kx]     # output channel g reads concatenated channel J g + j
    mean = a.mean(dim=-1, keepdim=True)
    var = (a - mean).pow(2).mean(dim=-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    return (a - mean) * rstd, rstd.squeeze(-1)


def backward(x, skip, w, bias, dy, eps=EPS):
    """-> (dx [B, H, W, C], dskip [B, H, W, C] or None, dw [C, J, 3, 3], dbias [C]) in fp64 for the gradient dy arriving at y"""
    y, rstd = forward(x, skip, w, bias, eps)
    xc = _cat(x, skip)
    C, J = w.size(0), w.size(1)
    w = w.double()
    dy = dy.double()
    c1 = dy.mean(dim=-1, keepdim=True)
    c2 = (dy * y).mean(dim=-1, keepdim=True)
    da = rstd.unsqueeze(-1) * (dy - c1 - y * c2)
    dbias = da.sum(dim=(0, 1, 2))
    dw = torch.zeros_like(w)
    dxc = torch.zeros_like(xc)
    for ky in range(3):
        for kx in range(3):
            s = _shifted(xc, ky - 1, kx - 1)             # xcat[pos + (ky - 1, kx - 1)]
            g = _shifted(da, 1 - ky, 1 - kx)             # da[pos - (ky - 1, kx - 1)]
            for j in range(J):
                dw[:, j, ky, kx] = (da * s[..., j::J]).sum(dim=(0, 1, 2))
                dxc[..., j::J] += g * w[:, j, ky, kx]
    if skip is None:
        return dxc, None, dw, dbias
    return dxc[..., :C], dxc[..., C:], dw, dbias
