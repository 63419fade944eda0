"""CPU model of confidence-ordered renoise and of the per-row statistics (DESIGN.md 4 "Confidence-ordered renoise") in numpy -- a restatement of the contract, not
of the kernels.

Statistics of one row of fp32 z_i = fp32(mix_i * inv_t), fp64 throughout:
  A = {i : z_i >= the top_k-th largest z} (ties kept; every label when top_k is off), m = max z, S = sum_A exp(z - m), E = sum_A (z - m) exp(z - m)
  logprob_i = (z_i - m) - log S for i in A,   entropy = log S - E / S;   a row with a NaN or without a finite maximum: logprob = -inf, entropy = NaN
Error bounds of the kernel's fp32 values, from tests/truncation_model.py's own model (U, gamma, delta_e: nothing fitted): with x = z - m, p = softmax over A,
Delta = sum_A p_i delta_e(x_i) and gamma = gamma(L), the kernel's S' = S (1 + d), |d| <= Delta + gamma, so log S' is off by (Delta + gamma)(1 + 2^-10); the
logarithm itself by at most 2 ulp of log S; x_t = fl(z_t - m) by |x_t| U; the final subtraction by one ulp of the result:
  eps_logp = |x_t| U + (Delta + gamma)(1 + 2^-10) + 2 ulp32(log S) + ulp32(logprob)
  eps_H    = eps_c + 2 ulp32(log S) + ulp32(H)                    eps_c: the error of c = E / S, as defined there

Renoise stage, per sample: free = the positions the pin does not own;
  count       n = clamp(rint(fp32(t_next) * fp32(|free|)), 0, |free|): an fp32 product rounded to nearest, ties to even; a negative or NaN t_next gives 0
  key(score)  the ascending order-preserving 32-bit key of the fp32 score: -0 == +0, NaN -> 0 (before -inf: the least confident)
  selection   the n free positions smallest in (key, position index)
  score       logprob when g == 0, else fp32 fma(-(g * t_next), log(-log u01_open(w1)), logprob), w1 = word 1 of philox4x32(seed ^ RENOISE_SALT, ctr_row, step) --
              the call whose word 0 is the random policy's coin
The selection is pure integer and fp32 arithmetic, hence exact; `score64` is the fp64 value of the score with the bound the device may differ by."""
import math

import numpy as np

from tests import counter_noise as C
from tests import truncation_model as TM


# ---------------------------------------------------------------------------------------------------------------- statistics
def row_stats(z, top_k=0):
    """One row.  z: fp32 [L].  -> dict(filtered, logprob fp64 [L] (-inf outside A), entropy, eps_logp fp64 [L], eps_H)."""
    z32 = np.asarray(z, dtype=np.float32)
    L = z32.size
    zz = z32.astype(np.float64)
    out = dict(filtered=False, logprob=np.full(L, -np.inf), entropy=math.nan, eps_logp=np.zeros(L), eps_H=0.0)
    if np.isnan(zz).any() or not np.isfinite(zz.max()):
        return out
    top_k = 0 if top_k is None else int(top_k)
    A = np.ones(L, bool)
    if 1 <= top_k < L:
        A = zz >= np.sort(zz)[::-1][top_k - 1]
    m = zz.max()
    with np.errstate(invalid="ignore"):
        x = np.where(A, zz - m, -np.inf)
    e = np.exp(x)
    S = e.sum()
    p = e / S
    ls = math.log(S)
    logp = x - ls
    c = (p * np.where(p > 0, x, 0.0)).sum()
    H = ls - c
    ax = np.where(A & np.isfinite(x), np.abs(x), 0.0)
    Delta = (p * TM.delta_e(ax)).sum()
    g = TM.gamma(L)
    eps_c = ((p * ax * (TM.delta_e(ax) + 2.0 * TM.U + g)).sum() + abs(c) * (Delta + g + TM.U)) * TM.SECOND_ORDER
    u_ls = float(C.ulp32(ls))
    with np.errstate(invalid="ignore"):
        eps_logp = ax * TM.U + (Delta + g) * TM.SECOND_ORDER + 2.0 * u_ls + C.ulp32(np.where(np.isfinite(logp), logp, 0.0))
    out.update(filtered=True, logprob=logp, entropy=H, eps_logp=eps_logp, eps_H=eps_c + 2.0 * u_ls + float(C.ulp32(H)))
    return out


# ---------------------------------------------------------------------------------------------------------------- selection
def score_key(scores):
    """uint32 keys of fp32 scores, ascending with the score: -0 == +0, NaN -> 0"""
    s = np.asarray(scores, dtype=np.float32).copy()
    nan = np.isnan(s)
    s[s == 0] = np.float32(0.0)
    b = s.view(np.uint32)
    neg = (b & np.uint32(0x80000000)) != 0
    key = np.where(neg, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    key[nan] = 0
    return key


def renoise_count(t_next, n_free):
    """n = clamp(rint(fp32(t_next) * fp32(n_free)), 0, n_free), the product in fp32, ties to even; NaN -> 0"""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.float32(t_next) * np.float32(n_free)
    if np.isnan(v):
        return 0
    return int(min(max(np.rint(np.float64(v)), 0.0), float(n_free)))


def select(scores_fp32, free, t_next):
    """bool [HW]: the renoised positions of one sample -- the n free positions smallest in (key(score), index)"""
    key = score_key(scores_fp32)
    free = np.asarray(free, dtype=bool)
    idx = np.nonzero(free)[0]
    n = renoise_count(t_next, idx.size)
    order = idx[np.lexsort((idx, key[idx]))]   # (last key is the primary one)
    out = np.zeros(key.size, bool)
    out[order[:n]] = True
    return out


# ---------------------------------------------------------------------------------------------------------------- scores
def renoise_words(seed, ctr_rows, step):
    """(w0, w1) of the renoise stage's one Philox call per position: key seed ^ RENOISE_SALT, counter (ctr_row, step)"""
    w = C.philox4x32(C.renoise_key(seed), np.asarray(ctr_rows, dtype=np.uint64), int(step))
    return w[0], w[1]


def score64(logprob, g, t_next, bits):
    """(score fp64, bound): logprob - fp32(g * t_next) * log(-log u01_open(bits)) and what the device's fp32 score may differ from it by -- the logarithm's
    stated bound scaled by g * t_next plus one ulp of the score (its single rounding, and the slack of a non-finite bound being none)"""
    lp = np.asarray(logprob, dtype=np.float32).astype(np.float64)
    if g == 0:
        return lp, np.zeros_like(lp)
    gt = float(np.float32(g) * np.float32(t_next))
    le = C.log_exp1(bits)
    with np.errstate(invalid="ignore"):
        s = lp - gt * le
    return s, abs(gt) * C.gumbel_bound(le) + C.ulp32(np.where(np.isfinite(s), s, 0.0))
