"""fp64 model of the training timestep modulation (include/paella_hip.h "Training timestep modulation"): the residual add, x (1 + a) + b with (a, b) the halves of
ab [B, 2C], and the LayerNorm over the channels, NHWC with the positions of a sample flattened, forward and the closed-form backward -- explicit sums, no
F.layer_norm, no autograd.  Plain torch on whatever device the inputs live on; shared by tests/test_mod_train.py (against torch's own autograd) and
tests/test_gpu_mod_train.py (against the HIP op)."""
import torch

EPS = 1e-6


def _parts(x, ab, residual):
    """x, residual (or None) [B, P, C]; ab [B, 2C] -> (u, 1 + a, b) in fp64, the last two as [B, 1, C]"""
    C = x.size(-1)
    u = x.double() if residual is None else x.double() + residual.double()
    ab = ab.double()
    return u, (1.0 + ab[:, :C]).unsqueeze(1), ab[:, C:].unsqueeze(1)


def forward(x, ab, residual=None, eps=EPS):
    """-> (x' [B, P, C], z [B, P, C], rstd [B, P]) in fp64"""
    u, s, b = _parts(x, ab, residual)
    xp = u * s + b
    C = x.size(-1)
    mean = xp.sum(dim=-1, keepdim=True) / C
    var = ((xp - mean) ** 2).sum(dim=-1, keepdim=True) / C
    rstd = 1.0 / torch.sqrt(var + eps)
    return xp, (xp - mean) * rstd, rstd.squeeze(-1)


def backward(x, ab, residual=None, dxp=None, dz=None, eps=EPS):
    """-> (dx [B, P, C], which is dresidual as well, dab [B, 2C]) in fp64 for the gradients dxp arriving at x' and dz at z (None: none arrived)"""
    u, s, _ = _parts(x, ab, residual)
    C = x.size(-1)
    g = torch.zeros_like(u) if dxp is None else dxp.double().clone()
    if dz is not None:
        _, z, rstd = forward(x, ab, residual, eps)
        dz = dz.double()
        c1 = dz.sum(dim=-1, keepdim=True) / C
        c2 = (dz * z).sum(dim=-1, keepdim=True) / C
        g = g + rstd.unsqueeze(-1) * (dz - c1 - z * c2)
    return g * s, torch.cat([(g * u).sum(dim=1), g.sum(dim=1)], dim=1)
