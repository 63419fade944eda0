"""fp64 model of the training MLP activation (include/paella_hip.h "Training MLP activation"): GELU -> GlobalResponseNorm -> Dropout of a [B, P, C] pre-activation,
forward and the closed-form backward, and the dropout keep mask from the independent CPU Philox of tests/counter_noise.py.  Plain torch on whatever device the inputs
live on; shared by tests/test_grn_act.py (against torch's own autograd) and tests/test_gpu_grn_act.py (against the HIP op)."""
import math

import numpy as np
import torch

from tests import counter_noise as CN

DROPOUT_SALT = 0xA0761D6478BD642F
EPS = 1e-6


def keep_mask(shape, p, seed):
    """[B, P, C] bool numpy: element e (flat index) takes word e & 3 of philox4x32(seed ^ DROPOUT_SALT, e >> 2, 0) and is kept iff u01_half_open(word) >= fp32(p)"""
    n = int(np.prod(shape))
    assert n % 4 == 0
    w = CN.philox4x32((int(seed) ^ DROPOUT_SALT) & CN.M64, np.arange(n // 4, dtype=np.uint64), 0)
    words = np.stack(w, axis=-1).reshape(n)
    return (CN.u01_half_open(words) >= float(np.float32(p))).reshape(shape)


def scale_of(p):
    """the kernels' one fp32 division"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def _keep64(keep, like):
    if keep is None:
        return torch.ones_like(like)
    return torch.as_tensor(keep, device=like.device).to(like.dtype)


def _parts(u, gamma):
    u = u.double()
    h = 0.5 * u * (1.0 + torch.erf(u / math.sqrt(2.0)))
    G = h.pow(2).sum(dim=1).sqrt()                       # [B, C]
    Mp = G.mean(dim=1, keepdim=True) + EPS               # [B, 1]
    n = G / Mp
    a = 1.0 + gamma.double().view(1, -1) * n             # [B, C]
    return u, h, G, Mp, n, a


def forward(u, gamma, beta, keep=None, p=0.0):
    """-> (z [B, P, C], G [B, C]) in fp64; keep: bool [B, P, C] or None (everything kept)"""
    u, h, G, Mp, n, a = _parts(u, gamma)
    y = h * a[:, None, :] + beta.double().view(1, 1, -1)
    return _keep64(keep, y) * y * scale_of(p), G


def backward(u, gamma, dz, keep=None, p=0.0):
    """-> (du [B, P, C], dgamma [C], dbeta [C]) in fp64 for the gradient dz arriving at z"""
    u, h, G, Mp, n, a = _parts(u, gamma)
    C = u.size(-1)
    g = gamma.double().view(1, -1)
    dy = _keep64(keep, u) * dz.double() * scale_of(p)
    dbeta = dy.sum(dim=(0, 1))
    S = (dy * h).sum(dim=1)                              # [B, C]
    dgamma = (n * S).sum(dim=0)
    dn = g * S
    dG = dn / Mp - (dn * G).sum(dim=1, keepdim=True) / (C * Mp * Mp)
    k = torch.where(G > 0, dG / torch.where(G > 0, G, torch.ones_like(G)), torch.zeros_like(G))
    dh = dy * a[:, None, :] + k[:, None, :] * h
    cdf = 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)
    return dh * (cdf + u * pdf), dgamma, dbeta
