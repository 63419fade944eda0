"""fp64 model of the training attention op (paella_amd/csrc/attn_train.hip, include/paella_hip.h "Training attention"), written independently of the kernels: the
forward and the closed-form backward with explicit exp / sum (no softmax, no scaled_dot_product_attention), and the dropout mask from the CPU Philox model of
tests/counter_noise.py."""
import math

import numpy as np
import torch

from tests import counter_noise as CN

ATTN_DROPOUT_SALT = 0xE7037ED1A0B428DB


def keep_mask(shape, p, seed):
    """[B, nhead, P, L] bool numpy: element e, the flat index in [B, nhead, P, L4] with L4 = 4 ceil(L / 4) (a quad never straddles a row), takes word e & 3 of
    philox4x32(seed ^ ATTN_DROPOUT_SALT, e >> 2, 0) and is kept iff u01_half_open(word) >= fp32(p)"""
    B, nhead, P, L = shape
    L4 = 4 * ((L + 3) // 4)
    rows = B * nhead * P
    w = CN.philox4x32((int(seed) ^ ATTN_DROPOUT_SALT) & CN.M64, np.arange(rows * (L4 // 4), dtype=np.uint64), 0)
    words = np.stack(w, axis=-1).reshape(rows, L4)[:, :L]
    return (CN.u01_half_open(words) >= float(np.float32(p))).reshape(shape)


def scale_of(p):
    """the kernels' one fp32 division"""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def heads(t, nhead):
    """[B, N, nhead * D] -> [B, nhead, N, D] in fp64"""
    B, N, C = t.shape
    return t.double().view(B, N, nhead, C // nhead).permute(0, 2, 1, 3)


def unheads(t):
    """[B, nhead, N, D] -> [B, N, nhead * D]"""
    B, nhead, N, D = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, N, nhead * D)


def _keep64(keep, like):
    if keep is None:
        return torch.ones_like(like)
    return torch.as_tensor(keep, device=like.device).to(like.dtype)


def _probs(q, k, nhead):
    qh, kh = heads(q, nhead), heads(k, nhead)
    s = (qh.unsqueeze(3) * kh.unsqueeze(2)).sum(-1) / math.sqrt(qh.size(-1))   # [B, nhead, P, L]
    m = s.max(dim=-1, keepdim=True).values
    lse = m + torch.log(torch.exp(s - m).sum(dim=-1, keepdim=True))
    return qh, kh, s, lse, torch.exp(s - lse)


def forward(q, k, v, nhead, keep=None, p=0.0):
    """q [B, P, C], k and v [B, L, C] -> (o [B, P, C], lse [B, nhead, P]) in fp64; keep: bool [B, nhead, P, L] or None (everything kept)"""
    qh, kh, s, lse, pr = _probs(q, k, nhead)
    pd = _keep64(keep, pr) * pr * scale_of(p)
    o = (pd.unsqueeze(-1) * heads(v, nhead).unsqueeze(2)).sum(3)
    return unheads(o), lse.squeeze(-1)


def backward(q, k, v, do, nhead, keep=None, p=0.0):
    """-> (dq [B, P, C], dk [B, L, C], dv [B, L, C]) in fp64 for the gradient do arriving at o"""
    qh, kh, s, lse, pr = _probs(q, k, nhead)
    vh, gh = heads(v, nhead), heads(do, nhead)
    kp = _keep64(keep, pr) * scale_of(p)
    pd = kp * pr
    o = (pd.unsqueeze(-1) * vh.unsqueeze(2)).sum(3)
    delta = (gh * o).sum(-1, keepdim=True)                                     # [B, nhead, P, 1]
    dpd = (gh.unsqueeze(3) * vh.unsqueeze(2)).sum(-1)                          # [B, nhead, P, L]
    ds = pr * (kp * dpd - delta)
    r = 1.0 / math.sqrt(qh.size(-1))
    dq = (ds.unsqueeze(-1) * kh.unsqueeze(2)).sum(3) * r
    dk = (ds.unsqueeze(-1) * qh.unsqueeze(3)).sum(2) * r
    dv = (pd.unsqueeze(-1) * gh.unsqueeze(3)).sum(2)
    return unheads(dq), unheads(dk), unheads(dv)
