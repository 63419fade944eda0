"""fp64 model of the training token stem (include/paella_hip.h "Training token stem"): the rows the op returns and the gradient it writes for the table, made by
torch fp64 autograd through F.embedding -> layer_norm -> pixel_unshuffle on the CPU -- the chain the network runs by default, and nothing of the kernel's
algorithm (no sum per label, no LayerNorm backward by hand).  Tokens outside [0, num_labels) are clamped first, as the inference kernel clamps them."""
import torch
import torch.nn.functional as F


def clamp_tokens(x, num_labels):
    return x.clamp(0, num_labels - 1)


def chain(x, weight, patch=1, eps=1e-6):
    """the torch chain in the dtype of `weight`, on its device: rows [B, H/p, W/p, c_in p^2] (differentiable in weight)"""
    c_in = weight.size(1)
    h = F.layer_norm(F.embedding(clamp_tokens(x, weight.size(0)), weight), (c_in,), None, None, eps).permute(0, 3, 1, 2)
    return F.pixel_unshuffle(h, patch).permute(0, 2, 3, 1).contiguous()


def model(x, weight, d_rows=None, patch=1, eps=1e-6):
    """fp64 on the CPU: (rows, dweight or None without d_rows)"""
    w = weight.detach().double().cpu().requires_grad_(d_rows is not None)
    rows = chain(x.cpu(), w, patch, eps)
    if d_rows is None:
        return rows.detach(), None
    rows.backward(d_rows.detach().double().cpu())
    return rows.detach(), w.grad


def inputs(B, H, W, patch, c_in, num_labels, seed=0, tokens=None):
    """(x int64 [B, H, W], weight fp32 [num_labels, c_in], d_rows fp32 [B, H/p, W/p, c_in p^2]) from a seeded CPU generator; tokens: a value every position holds"""
    g = torch.Generator().manual_seed(1000 + seed)
    x = torch.randint(0, num_labels, (B, H, W), generator=g) if tokens is None else torch.full((B, H, W), int(tokens), dtype=torch.int64)
    weight = torch.randn(num_labels, c_in, generator=g) * 0.7 + 0.1 * torch.randn(num_labels, 1, generator=g)
    d_rows = torch.randn(B, H // patch, W // patch, c_in * patch * patch, generator=g)
    return x, weight, d_rows
