"""CPU model of truncated sampling (top-k, nucleus, typical filtering) in fp64 -- a restatement of the contract, not of the kernel -- plus the BAND of every row: the
labels whose membership could differ under the fp32 arithmetic of `sample_tail_filter_kernel`.  A GPU test uses a row only when its band is empty and then demands
the kernel's kept set to equal the model's exactly.

Contract (DESIGN.md 4 "Truncated sampling"), for one row of fp32 z_i = fp32(mix_i * inv_t):
  stage A   top_k = k, 1 <= k < L: A = {i : z_i >= the k-th largest z} (ties kept); otherwise A = every label
  p         p_i = exp(z_i - m) / sum_A exp(z_j - m), m = max z; a label with p_i = 0 adds 0 to the entropy H = -sum_A p log p
  stage B   top_p = P in (0, 1):        kept = {i in A : z_i >= v*}, v* the largest value with sum_{z_j >= v*} p_j >= P
            typical_mass = M in (0, 1): kept = {i in A : d_i <= d*}, d_i = |-log p_i - H|, d* the smallest value with sum_{d_j <= d*} p_j >= M
            neither: kept = A; both: ValueError
  min_tokens = n >= 1: with a mass filter the n first labels of A in stage B's order (descending z / ascending d) stay as well, ties at the n-th value kept
  a mass target never reached (rounding): kept = A;  a row with a NaN or without a finite maximum: not filtered (kept = every label)

Error model of the kernel (u = 2^-24, the unit roundoff of fp32).  Nothing here is fitted to the kernel's output.
  * exp: the kernel forms x' = fl(z - m) (relative error u, so |x' - x| <= |x| u) and e' = v_exp_f32(fl(x' * fl(log2 e))): the constant and the product each
    carry a relative error u, so the exponent y = x log2(e) is off by at most |y| 2u, which is a RELATIVE error |x| 2u ln2 log2(e) = |x| 2u of 2^y; the
    instruction itself is accurate to 1 ulp = 2u (CDNA ISA: v_exp_f32).  With the error of x' (relative |x| u of e):
        delta_e(x) = (3 |x| + 2) u                                  (results below 2^-126 flush to 0: an absolute error of 2^-126 per label, ignored against u)
  * sums: every sum is one fixed-order reduction -- n_seq = ceil(L / 256) sequential terms per thread, then a tree (6 shuffle levels in the wave, 2 levels across
    the 4 waves; the bound below allows 10 levels).  A sum of non-negative terms evaluated in ANY such order has relative error <= gamma = (n_seq - 1 + 10) u.
  * mass: the kernel compares W' = sum'(e'_i over a candidate set) with T' = fl(fl32(P) * S'), S' = sum'(e' over A).  Normalised by the exact S:
        |W'/S - W/S| <= Delta + gamma,  Delta = sum_A p_i delta_e(x_i);        |T'/S - P| <= P (Delta + gamma + 2u)
    so the kernel's decision equals the model's whenever the exact cumulative mass differs from P by more than
        eps_mass = ((1 + P) (Delta + gamma) + 2 u P) (1 + 2^-10)             (the last factor covers the second-order terms)
  * keys: the z keys of top-k and top-p are the fp32 inputs themselves -- exact, eps_key = 0.  The typical key is d'_i = fl|c' - x'_i| with c' = fl(E'/S'),
    E' = sum'(fl(x'_i e'_i)): each term of E carries delta_e + 2u, the sum gamma, the quotient S's error and one rounding:
        eps_c = (sum_A p_i |x_i| (delta_e(x_i) + 2u + gamma) + |c| (Delta + gamma + u)) (1 + 2^-10)
        eps_key(i) = eps_c + |x_i| u + (d_i + eps_c + |x_i| u) u
    Two labels of equal z have equal keys in the kernel as in the model.  Labels i outside the threshold group {d_j = d*} with |d_i - d*| <= eps_key(i) + eps_key(*)
    could change sides of the cut; so could a threshold group that holds two different z (equal d only in exact arithmetic).
Band of a row = the labels flagged by the key condition, plus the threshold group (and its predecessor) when the exact cumulative mass just below or at the cut lies
within eps_mass of the target.  With an empty band the kernel's order separates the same two sets as the model's and, the fixed-order sums being monotone in the
set, its bisection stops at the same cut."""
import math

import numpy as np

U = 2.0 ** -24
TREE_LEVELS = 10
SECOND_ORDER = 1.0 + 2.0 ** -10


def z_of(logits_c, logits_u, cfg, omc, temperature):
    """fp32 z exactly as the tail forms it: mix = l_c * cfg + l_u * omc (two products, one sum, each rounded), inv_t = fp32(1 / T), z = fp32(mix * inv_t)"""
    lc = np.asarray(logits_c, dtype=np.float32)
    if logits_u is None:
        mix = lc
    else:
        mix = (lc * np.float32(cfg)).astype(np.float32) + (np.asarray(logits_u, dtype=np.float32) * np.float32(omc)).astype(np.float32)
        mix = mix.astype(np.float32)
    inv_t = np.float32(1.0) / np.float32(temperature)
    with np.errstate(invalid="ignore", over="ignore"):
        return (mix * inv_t).astype(np.float32)


def gamma(L):
    return (math.ceil(L / 256) - 1 + TREE_LEVELS) * U


def delta_e(x):
    return (3.0 * np.abs(x) + 2.0) * U


def _groups(keys):
    """ascending distinct keys, and for every label the index of its group"""
    vals, inv = np.unique(keys, return_inverse=True)
    return vals, inv


def truncate_row(z, top_k=0, top_p=1.0, typical_mass=1.0, min_tokens=1):
    """One row.  z: fp32 [L].  Returns dict(kept bool [L], band bool [L], filtered, m, logsum, H, threshold)."""
    z32 = np.asarray(z, dtype=np.float32)
    L = z32.size
    top_k = 0 if top_k is None else int(top_k)
    top_p = 1.0 if top_p is None else float(top_p)
    typical_mass = 1.0 if typical_mass is None else float(typical_mass)
    k_on = 1 <= top_k < L
    p_on = 0.0 < top_p < 1.0
    t_on = 0.0 < typical_mass < 1.0
    if p_on and t_on:
        raise ValueError("top_p and typical_mass are mutually exclusive")
    if min_tokens < 1:
        raise ValueError("min_tokens must be >= 1")
    out = dict(kept=np.ones(L, bool), band=np.zeros(L, bool), filtered=False, m=math.nan, logsum=math.nan, H=math.nan, threshold=math.nan)
    zz = z32.astype(np.float64)
    if np.isnan(zz).any() or not np.isfinite(zz.max()):
        return out
    out["filtered"] = True
    m = zz.max()
    A = np.ones(L, bool)
    if k_on:
        kth = np.sort(zz)[::-1][top_k - 1]
        A = zz >= kth
        out["threshold"] = kth
    with np.errstate(invalid="ignore"):
        x = np.where(A, zz - m, -np.inf)
    e = np.exp(x)
    S = e.sum()
    p = e / S
    logp = x - math.log(S)
    H = -np.where(p > 0, p * np.where(p > 0, logp, 0.0), 0.0).sum()
    out.update(m=m, logsum=math.log(S), H=H, kept=A.copy())
    if not (p_on or t_on):
        return out
    target = top_p if p_on else typical_mass
    ax = np.where(A & np.isfinite(x), np.abs(x), 0.0)
    Delta = (p * delta_e(ax)).sum()
    g = gamma(L)
    eps_mass = ((1.0 + target) * (Delta + g) + 2.0 * U * target) * SECOND_ORDER
    if p_on:
        key = -zz                                   # ascending key = stage B's order
        eps_key = np.zeros(L)
    else:
        with np.errstate(invalid="ignore"):
            key = np.where(A, np.abs(-logp - H), np.inf)
        c = (p * np.where(p > 0, x, 0.0)).sum()
        eps_c = ((p * ax * (delta_e(ax) + 2.0 * U + g)).sum() + abs(c) * (Delta + g + U)) * SECOND_ORDER
        eps_key = np.where(np.isfinite(key), eps_c + ax * U + (np.where(np.isfinite(key), key, 0.0) + eps_c + ax * U) * U, 0.0)
    key = np.where(A, key, np.inf)
    band = np.zeros(L, bool)

    def near(cut_key, cut_eps):
        """labels outside the group {key == cut_key} that the kernel's rounding could move across it; the group itself when it mixes different z"""
        grp = A & (key == cut_key)
        b = A & ~grp & np.isfinite(key) & (np.abs(key - cut_key) <= eps_key + cut_eps)
        if np.unique(zz[grp]).size > 1 and not p_on:
            b |= grp
        return b

    vals, inv = _groups(key[A])
    mass = np.bincount(inv, weights=p[A], minlength=vals.size)
    cum = np.cumsum(mass)
    hit = np.nonzero(cum >= target)[0]
    if hit.size == 0:                               # the target is never reached: kept = A
        band |= A & (abs(cum[-1] - target) <= eps_mass)
        out["band"] = band
        return out
    j = int(hit[0])
    cut = vals[j]
    below = cum[j - 1] if j > 0 else 0.0
    if abs(cum[j] - target) <= eps_mass:
        band |= A & (key == cut)
        if j + 1 < vals.size:
            band |= A & (key == vals[j + 1])
    if j > 0 and abs(below - target) <= eps_mass:
        band |= A & ((key == cut) | (key == vals[j - 1]))
    band |= near(cut, eps_key[A & (key == cut)].max())
    if min_tokens > 1:
        nA = int(A.sum())
        if min_tokens >= nA:
            cut_n = np.inf
        else:
            cut_n = np.sort(key[A])[min_tokens - 1]
            band |= near(cut_n, eps_key[A & (key == cut_n)].max())
        cut = max(cut, cut_n)
    out["kept"] = A & (key <= cut)
    out["band"] = band
    out["threshold"] = (-cut if p_on else cut) if np.isfinite(cut) else math.nan
    return out


def truncate_rows(z, **kw):
    """every row of z [rows, L] -> (kept bool [rows, L], band bool [rows, L])"""
    res = [truncate_row(r, **kw) for r in np.asarray(z)]
    return np.stack([r["kept"] for r in res]), np.stack([r["band"] for r in res])


# ---------------------------------------------------------------------------------------------------------------- inputs of the GPU tests
# (L, filter, logit scale) of every kernel-level GPU case; tests/test_truncated_sampling.py asserts that at most half of the candidate rows of each are rejected
GPU_SHAPES = (64, 1036, 8192)
GPU_FILTERS = {
    "top_k": dict(top_k=50),
    "top_k=1": dict(top_k=1),
    "top_p": dict(top_p=0.6),
    "typical": dict(typical_mass=0.5),
    "top_k+top_p": dict(top_k=40, top_p=0.8),
    "top_k+typical": dict(top_k=40, typical_mass=0.3),
    "min_tokens": dict(top_p=0.1, min_tokens=12),
    "typical+min_tokens": dict(typical_mass=0.05, min_tokens=9),
}
GPU_SCALE = 1.5
CANDIDATES = 160  # candidate rows per case; the GPU tests use the first rows with an empty band


def candidate_logits(L, name, with_u, n=CANDIDATES, seed=1234):
    """fixed candidate rows of one case: (logits_c, logits_u or None, cfg, omc, temperature), fp32"""
    rng = np.random.default_rng([seed, L, sorted(GPU_FILTERS).index(name), int(with_u)])
    lc = (rng.standard_normal((n, L)) * GPU_SCALE).astype(np.float32)
    if not with_u:
        return lc, None, 1.0, 0.0, 0.8
    lu = (rng.standard_normal((n, L)) * GPU_SCALE).astype(np.float32)
    return lc, lu, 1.5, -0.5, 0.8


def select_rows(L, name, with_u, rows):
    """the first `rows` candidate rows with an empty band -> (logits_c, logits_u, cfg, omc, T, kept [rows, L], rejected fraction over ALL candidates)"""
    lc, lu, cfg, omc, T = candidate_logits(L, name, with_u)
    kept, band = truncate_rows(z_of(lc, lu, cfg, omc, T), **GPU_FILTERS[name])
    ok = ~band.any(axis=1)
    idx = np.nonzero(ok)[0][:rows]
    return lc[idx], (None if lu is None else lu[idx]), cfg, omc, T, kept[idx], 1.0 - ok.mean()
