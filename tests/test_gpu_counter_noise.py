"""GPU: the counter-based noise (`noise="philox"`) against the independent numpy model in tests/counter_noise.py.

Every random number of that mode -- start tokens, inpainting's random_x, the categorical draw (tail kernel and the head GEMM's
fused epilogue), the renoise mask, paella_add_noise's Philox branch -- is compared with the model: integers and the exact
uniform grids bit for bit, the fp32 Gumbel transform against fp64 within a stated bound (tokens may then differ only where the
model's own top-1 / top-2 score margin is below twice that bound; such rows are counted and printed).  The sampler is checked in
closed loop against the CPU oracle's UNet with the model supplying every draw."""
import types

import numpy as np
import pytest
import torch

import paella_amd
from oracle import golden_configs as G
from oracle import paella_oracle as O
from paella_amd import _lib, sampling
from tests import counter_noise as C
from tests.helpers import cond_for, to_dev, weights_for

pytestmark = pytest.mark.gpu
DEV = "cuda"

SEED_HI = 0xC3A5C85C97CB3127          # bit 63 set
# the largest |device log_exp1 - fp64| the bound allows anywhere on the u grid (|log E| <= 24 ln 2 = 16.64)
DELTA = float(C.gumbel_bound(np.array([24 * np.log(2.0)]))[0])


def _signed(w):
    w &= C.M64
    return w - (1 << 64) if w >= 1 << 63 else w


def _word(v):
    return None if v is None else torch.tensor([_signed(v)], dtype=torch.int64, device=DEV)


def _stream():
    return _lib.stream_ptr(torch.device(DEV))


def _tail_ex(lc, lu, L, cfg, omc, temperature, mode, seed, step, out, sampled=None, seed_word=None, row_offset=0, row_word=None,
             init=None, t_next=0.0):
    lib = _lib.load()
    sw, rw = _word(seed_word), _word(row_word)
    _lib.check(lib.paella_sample_tail_ex(_lib.ptr(lc), _lib.ptr(lu), lc.size(0), L, cfg, omc, temperature, mode, None, seed, _lib.ptr(sw), step,
                                         row_offset, _lib.ptr(rw), _lib.ptr(init), None, t_next, _lib.ptr(out), _lib.ptr(sampled), _stream()))
    torch.cuda.synchronize()


def _device_scores(lc, lu, L, cfg, omc, temperature, seed, step, row_offset, out):
    _lib.check(_lib.load().paella_test_tail_scores(_lib.ptr(lc), _lib.ptr(lu), lc.size(0), L, cfg, omc, temperature, seed, step, row_offset,
                                                   _lib.ptr(out), _stream()))
    torch.cuda.synchronize()


def _cfg_logits(rows, L, seed, rho=0.9, sigma=3.0):
    """Conditional / unconditional logits as correlated N(0, sigma^2) pairs (what classifier-free guidance mixes)."""
    g = torch.Generator().manual_seed(seed)
    lc = torch.randn(rows, L, generator=g) * sigma
    lu = rho * lc + (1 - rho * rho) ** 0.5 * sigma * torch.randn(rows, L, generator=g)
    return lc, lu


def _near_tie_eps(max_abs_score, logit_diff_over_t=0.0):
    """A token may differ from the model only where the model's top-1 / top-2 margin is below this: each of the two scores is
    off by <= DELTA (noise) + logit_diff_over_t (logits) + half an ulp (the score's own rounding)."""
    return 2.0 * (DELTA + logit_diff_over_t) + float(C.ulp32(np.array([max_abs_score]))[0])


def _compare_tokens(what, got_final, pre, final, margin, eps, mask=None, got_pre=None):
    """got_* device tokens, (pre, final, margin) the model's.  Pre-renoise tokens must equal the model's wherever its margin
    exceeds eps; renoised rows (mask) must equal the model's final tokens exactly; with got_pre given, the final tokens must be
    exactly the model's renoise of the DEVICE's pre-renoise tokens."""
    near = margin <= eps
    src = got_pre if got_pre is not None else got_final
    keep = np.ones_like(near) if (mask is None or got_pre is not None) else ~mask
    mism = (src != pre) & keep
    n_clear, n_near = int((mism & ~near).sum()), int((mism & near).sum())
    print("%s: %d rows, %d with model margin <= %.2e, %d of them differ; %d differ above it" % (what, margin.size, int(near.sum()), eps, n_near, n_clear))
    assert n_clear == 0, "%s: %d token(s) differ from the model where its decision margin exceeds %.2e (rows %s)" % (
        what, n_clear, eps, np.nonzero(mism & ~near)[0][:8].tolist())
    if got_pre is not None:
        want = np.where(mask, final, got_pre) if mask is not None else got_pre
        assert np.array_equal(got_final, want), "%s: renoised tokens differ from the model at %d rows" % (what, int((got_final != want).sum()))
    elif mask is not None:
        assert np.array_equal(got_final[mask], final[mask]), "%s: renoised rows differ from init_noise" % what
    return n_near


# ---------------------------------------------------------------------------------------------------------------- (a) start tokens
@pytest.mark.parametrize("L", [8192, 1000, 1])
def test_start_tokens_bit_exact(built_lib, L):
    """paella_start_tokens past the kernel's 4096-block grid (grid-stride loop), a seed with bit 63 set, device-resident seed and
    row-offset words, a seed word that wraps the seed past 2^64 and a row offset past 2^32."""
    n = 4096 * 256 + 4099
    out = torch.empty(n, dtype=torch.int64, device=DEV)
    for seed, seed_word, row_off, row_word in [(SEED_HI, None, 0, None),
                                               (SEED_HI, (1 << 64) - SEED_HI + 17, (1 << 32) + 5, None),
                                               (12345, 1 << 63, 7, (1 << 32) - 3)]:
        sw, rw = _word(seed_word), _word(row_word)
        _lib.check(built_lib.paella_start_tokens(seed, _lib.ptr(sw), row_off, _lib.ptr(rw), L, n, _lib.ptr(out), _stream()))
        torch.cuda.synchronize()
        want = C.start_tokens(seed, n, L, row_off, seed_word or 0, row_word or 0)
        got = out.cpu().numpy()
        assert np.array_equal(got, want), "start tokens L=%d seed=%#x: %d of %d differ" % (L, seed, int((got != want).sum()), n)
    if L > 1:
        assert np.unique(want).size == L or np.unique(want).size > 0.99 * L


def test_sampler_start_tokens_and_inpaint_random_x(built_lib):
    """sampling.start_tokens (shard rows) and inpaint(noise="philox")'s random_x -- the start tokens of the salted seed, here with a
    seed whose salted sum wraps past 2^64."""
    from paella_amd import editing
    B, H, W, L, total = 3, 16, 16, 8192, 7
    for seed in (SEED_HI, C.M64 - 11):
        got = sampling.start_tokens(L, (B, H, W), seed, DEV, shard=(2, total)).cpu().numpy().reshape(-1)
        assert np.array_equal(got, C.start_tokens(seed, B * H * W, L, row_offset=2 * H * W))
        rx = editing._philox_random_x(types.SimpleNamespace(num_labels=L), (B, H, W), seed, DEV, shard=(4, total)).cpu().numpy().reshape(-1)
        assert np.array_equal(rx, C.random_x_tokens(seed, B * H * W, L, row_offset=4 * H * W))
        assert not np.array_equal(rx, C.start_tokens(seed, B * H * W, L, row_offset=4 * H * W))


def test_add_noise_philox_branch(built_lib):
    """paella_add_noise with no mask, rand_u or random_x: mask u01_half_open(w0) <= t[b], random_x ((w1 << 32) | w2) mod L."""
    B, per, L = 3, 4096 * 100 + 17, 8192
    g = torch.Generator().manual_seed(5)
    x = torch.randint(0, L, (B, per), generator=g)
    t = torch.tensor([0.1, 0.5, 0.97], dtype=torch.float32)
    xd, td = x.to(DEV), t.to(DEV)
    xo, mo = torch.empty_like(xd), torch.empty_like(xd)
    _lib.check(built_lib.paella_add_noise(_lib.ptr(xd), _lib.ptr(td), None, None, None, SEED_HI, 11, L, B, per, _lib.ptr(xo), _lib.ptr(mo), _stream()))
    torch.cuda.synchronize()
    want_x, want_m = C.add_noise_philox(x.numpy(), t.numpy(), SEED_HI, 11, L)
    assert np.array_equal(mo.cpu().numpy(), want_m)
    assert np.array_equal(xo.cpu().numpy(), want_x)


# ---------------------------------------------------------------------------------------------------------------- (b) Gumbel transform
SEED_B = 0x9E3779B97F4A7C15  # with steps 0 and 1 over 8192 x 8192 labels it draws both end points of the 2^23-point u grid


def test_gumbel_transform_accuracy_against_fp64(built_lib):
    """All-zero logits at T = 1: every score is exactly -log_exp1(w).  2^27 draws (8192 rows x 8192 labels x 2 steps), both end points
    of the u grid among them, compared with fp64 log(-log u) against the stated bound (tests/counter_noise.py: GUMBEL_ULPS ulp of
    |log E| + GUMBEL_ABS)."""
    rows, L, chunk = 8192, 8192, 512
    zeros = torch.zeros(rows, L, device=DEV)
    scores = torch.empty_like(zeros)
    worst_err = worst_ratio = 0.0
    at_err = at_ratio = None
    near1_err = 0.0
    seen = [False, False]
    for step in (0, 1):
        _device_scores(zeros, None, L, 1.0, 0.0, 1.0, SEED_B, step, 0, scores)
        for a in range(0, rows, chunk):
            dev = -scores[a:a + chunk].cpu().numpy().astype(np.float64)
            w = C.categorical_words(SEED_B, chunk, L, step, row_offset=a)
            grid = w >> np.uint64(9)
            seen[0] |= bool((grid == 0).any())
            seen[1] |= bool((grid == (1 << 23) - 1).any())
            ref = C.log_exp1(w)
            err = np.abs(dev - ref)
            ratio = err / C.gumbel_bound(ref)
            i, j = np.unravel_index(np.argmax(err), err.shape), np.unravel_index(np.argmax(ratio), ratio.shape)
            if err[i] > worst_err:
                worst_err, at_err = float(err[i]), (float(C.u01_open(w[i])), float(ref[i]), float(dev[i]))
            if ratio[j] > worst_ratio:
                worst_ratio, at_ratio = float(ratio[j]), (float(C.u01_open(w[j])), float(ref[j]), float(dev[j]), float(err[j]))
            hi = grid >= (1 << 23) - (1 << 13)  # u > 1 - 2^-10: the largest Gumbel draws
            if hi.any():
                near1_err = max(near1_err, float(err[hi].max()))
    print("Gumbel transform, 2^27 draws: worst |err| %.3e at u = %.10f (log E %.7f, device %.7f); worst err / bound %.3f at u = %.10f "
          "(log E %.7f, device %.7f, err %.3e); worst |err| at u > 1 - 2^-10: %.3e; delta (bound at |log E| = 16.64) = %.3e"
          % ((worst_err,) + at_err + (worst_ratio,) + at_ratio + (near1_err, DELTA)))
    assert seen == [True, True], "the draws must include both end points of the u grid (u = 2^-24 and 1 - 2^-24)"
    assert worst_ratio <= 1.0, "log_exp1 is off by %.3g x its stated bound at u = %.10f" % (worst_ratio, at_ratio[0])


@pytest.mark.parametrize("mix", [(8.0, -7.0), (7.5, -6.5)], ids=["cfg8", "cfg7.5"])
@pytest.mark.parametrize("temperature", [1.0, 0.2, 0.05])
def test_gumbel_scores_with_guidance_against_fp64(built_lib, temperature, mix):
    """CFG 8 / -7 (and 7.5 / -6.5, whose products round) over correlated N(0, 3^2) logit pairs: device score - model score stays within
    the transform's bound plus half an ulp of the score -- the score is ONE rounding of mix * fp32(1/T) - log q, the mix two roundings."""
    cfg, omc = mix
    rows, L, chunk = 2048, 8192, 512
    lc, lu = _cfg_logits(rows, L, 11)
    lcd, lud = lc.to(DEV), lu.to(DEV)
    scores = torch.empty(rows, L, device=DEV)
    step, row_off = 5, 3 * (1 << 21) + 1   # (row + offset) * L/4 past 2^32
    _device_scores(lcd, lud, L, cfg, omc, temperature, SEED_HI, step, row_off, scores)
    worst = 0.0
    for a in range(0, rows, chunk):
        dev = scores[a:a + chunk].cpu().numpy().astype(np.float64)
        mixed = C.mix_logits(lc[a:a + chunk].numpy(), lu[a:a + chunk].numpy(), cfg, omc)
        w = C.categorical_words(SEED_HI, chunk, L, step, row_offset=row_off + a)
        lq = C.log_exp1(w)
        ref = C.scaled_logits(mixed, temperature) - lq
        ratio = np.abs(dev - ref) / (C.gumbel_bound(lq) + 0.5 * C.ulp32(dev))
        worst = max(worst, float(ratio.max()))
    print("scores with guidance %g / %g, T=%g: worst |device - model| / (bound + ulp/2) = %.3f" % (cfg, omc, temperature, worst))
    assert worst <= 1.0


# ---------------------------------------------------------------------------------------------------------------- (c) tail kernel
TAIL_CASES = [
    # L, rows, guidance, T, step, seed, seed word, row offset, row-offset word
    (8192, 512, True, 1.0, 0, SEED_HI, None, 0, None),
    (8192, 512, False, 0.7, 11, SEED_HI, (1 << 64) - 5, 3 * (1 << 21) + 9, None),       # seed word wraps; (row + off) * 2048 > 2^32
    (8192, 256, True, 0.3, 11, 77, 1 << 63, 5, (1 << 21) + 100),                         # the row-offset word carries past 2^32
    (4, 4096, True, 1.0, 11, SEED_HI, None, (1 << 32) + 3, None),
    (12, 2048, False, 0.5, 0, SEED_HI, 12345, 17, (1 << 30)),
    (1028, 1024, True, 0.8, 11, SEED_HI, None, (1 << 32) // 257 - 300, 3),
]


@pytest.mark.parametrize("case", TAIL_CASES, ids=lambda c: "L%d-%s-step%d" % (c[0], "cfg" if c[2] else "nocfg", c[4]))
def test_tail_kernel_against_model(built_lib, case):
    L, rows, guided, T, step, seed, seed_word, row_off, row_word = case
    lc, lu = _cfg_logits(rows, L, L + step)
    if not guided:
        lu = None
    cfg, omc = (8.0, -7.0) if guided else (1.0, 0.0)
    g = torch.Generator().manual_seed(3)
    init = torch.randint(0, L, (rows,), generator=g)
    lcd, lud, initd = lc.to(DEV), None if lu is None else lu.to(DEV), init.to(DEV)
    out = torch.empty(rows, dtype=torch.int64, device=DEV)
    pre_d = torch.empty_like(out)
    t_next = 0.45
    _tail_ex(lcd, lud, L, cfg, omc, T, 0, seed, step, out, pre_d, seed_word, row_off, row_word, initd, t_next)
    lun = None if lu is None else lu.numpy()
    pre, final, margin = C.sample_tail(lc.numpy(), T, seed, step, lu=lun, cfg=cfg, omc=omc, row_offset=row_off, seed_word=seed_word or 0,
                                       row_offset_word=row_word or 0, init_noise=init.numpy(), t_next=t_next)
    mask = C.renoise_mask(seed, rows, step, t_next, row_off, seed_word or 0, row_word or 0)
    assert 0.3 < mask.mean() < 0.6
    top = float(np.abs(C.scaled_logits(C.mix_logits(lc.numpy(), lun, cfg, omc), T)).max()) + 17.0
    _compare_tokens("tail L=%d step %d" % (L, step), out.cpu().numpy(), pre, final, margin, _near_tie_eps(top), mask, pre_d.cpu().numpy())
    # argmax mode: the first argmax of the fp32 mix, exactly
    _tail_ex(lcd, lud, L, cfg, omc, 1.0, 1, seed, step, out, None, seed_word, row_off, row_word)
    am = C.sample_tail(lc.numpy(), 1.0, seed, step, lu=lun, cfg=cfg, omc=omc, argmax=True)[0]
    assert np.array_equal(out.cpu().numpy(), am)


# ---------------------------------------------------------------------------------------------------------------- (d) fused head + tail
# UNET_TINY's body with an 8192-label head: 32 x 32 tokens -> 1024 x 8192 logits = 512 tiles of 128 x 128, enough for the fused tail
# to take the tile chosen by paella_test_gemm_tail_tile; c_out % 64 == 0 so the bf16 fast mode runs the head on bf16 operands.
HEAD_8K = dict(G.UNET_TINY, c_in=64, c_out=64, num_labels=8192)
FUSED_CASES = [
    # guidance, T, step, seed, seed word, row offset, row-offset word, renoise
    (True, 1.0, 0, SEED_HI, None, 0, None, False),
    (True, 0.3, 11, SEED_HI, (1 << 64) - 9, 3 * (1 << 21), None, True),
    (False, 0.8, 3, 4242, None, 5, (1 << 21) + 3, True),
]


def _fused_vs_model(m, cfg, B, grid, what):
    L = cfg["num_labels"]
    c, u = cond_for(cfg, B, 3, 0, 1), cond_for(cfg, B, 3, 0, 2)
    both = {k: (torch.cat([c[k], u[k]]) if c[k] is not None else None) for k in c}
    cache2, cache1 = m.prepare_cond(**to_dev(both, DEV)), m.prepare_cond(**to_dev(c, DEV))
    g = torch.Generator().manual_seed(9)
    x = torch.randint(0, L, (B, grid, grid), generator=g).to(DEV)
    r = torch.full((B,), 0.6, device=DEV)
    rows = B * grid * grid
    out = torch.empty(B, grid, grid, dtype=torch.int64, device=DEV)
    for guided, T, step, seed, seed_word, row_off, row_word, renoise in FUSED_CASES:
        cache, mix = (cache2, (8.0, -7.0)) if guided else (cache1, None)
        logits = m._forward_prepared_raw(x, r, cache, cfg_mix=mix).reshape(rows, L).cpu().numpy()
        init = torch.randint(0, L, (B, grid, grid), generator=g).to(DEV) if renoise else None
        t_next = 0.55 if renoise else 0.0
        m.forward_sample(x, r, cache, out, temperature=T, seed=seed, seed_dev=_word(seed_word), offset=step, row_offset=row_off,
                         row_offset_dev=_word(row_word), init_noise=init, t_next=t_next, cfg_mix=mix)
        torch.cuda.synchronize()
        pre, final, margin = C.sample_tail(logits, T, seed, step, row_offset=row_off, seed_word=seed_word or 0, row_offset_word=row_word or 0,
                                           init_noise=None if init is None else init.cpu().numpy(), t_next=t_next)
        mask = C.renoise_mask(seed, rows, step, t_next, row_off, seed_word or 0, row_word or 0) if renoise else None
        top = float(np.abs(C.scaled_logits(logits, T)).max()) + 17.0
        _compare_tokens("%s fused, %s T=%g step %d%s" % (what, "cfg" if guided else "no cfg", T, step, " + renoise" if renoise else ""),
                        out.cpu().numpy().reshape(-1), pre, final, margin, _near_tie_eps(top), mask)


@pytest.fixture(scope="module")
def head8k(built_lib):
    m = paella_amd.Paella(**HEAD_8K)
    weights_for(m, sum(HEAD_8K["blocks"]))
    return m.to(DEV)


def test_fused_tail_small_head_against_model(built_lib):
    """UNET_TINY (64 labels): the fused tail runs on tile 2."""
    cfg = G.UNET_TINY
    m = paella_amd.Paella(**cfg)
    weights_for(m, sum(cfg["blocks"]))
    _fused_vs_model(m.to(DEV), cfg, 2, 16, "UNET_TINY tile 2")


@pytest.mark.parametrize("tile", [9, 14, 18])
def test_fused_tail_large_head_against_model(built_lib, head8k, tile):
    default_tile = 18  # paella_amd/csrc/gemm.hip g_tail_tile
    built_lib.paella_test_gemm_tail_tile(tile)
    try:
        _fused_vs_model(head8k, HEAD_8K, 1, 32, "8192-label head, tile %d" % tile)
    finally:
        built_lib.paella_test_gemm_tail_tile(default_tile)


def test_fused_tail_bf16_head_against_model(built_lib, head8k):
    head8k.set_gemm_precision("bf16")
    try:
        _fused_vs_model(head8k, HEAD_8K, 1, 32, "8192-label head, bf16 fast mode")
    finally:
        head8k.set_gemm_precision("fp32")


# ---------------------------------------------------------------------------------------------------------------- (e) distribution
def _binned_chi2(counts, p, n, min_expected=50.0):
    """Labels sorted by probability, grouped into consecutive bins of expected count >= min_expected; returns (chi2, dof, p-value)."""
    from scipy.stats import chi2
    order = np.argsort(-p, kind="stable")
    obs, exp = [], []
    o = e = 0.0
    for i in order:
        o += counts[i]
        e += n * p[i]
        if e >= min_expected:
            obs.append(o)
            exp.append(e)
            o = e = 0.0
    if e > 0 or o > 0:
        obs[-1] += o
        exp[-1] += e
    obs, exp = np.array(obs), np.array(exp)
    stat = float(((obs - exp) ** 2 / exp).sum())
    dof = obs.size - 1
    return stat, dof, float(chi2.sf(stat, dof)) if dof > 0 else 1.0


@pytest.mark.parametrize("case", ["cfg-T1.0", "cfg-T0.2", "flat-heavy-tail"])
def test_categorical_distribution_at_8192_labels(built_lib, case):
    """4096 identical rows x 64 step offsets = 262144 draws from one categorical distribution over 8192 labels: chi-square against
    softmax(fp32(mix * fp32(1/T))) (bins of expected count >= 50), the summed frequency of the labels with p < 1e-4 (they win only
    through the largest Gumbel draws, u -> 1) within 5 binomial sigma, and per step the renoise fraction against t_next."""
    L, R, S = 8192, 4096, 64
    g = torch.Generator().manual_seed(21)
    if case.startswith("cfg"):
        T = 1.0 if case == "cfg-T1.0" else 0.2
        lc, lu = _cfg_logits(1, L, 21, rho=0.98)
        cfg, omc = 8.0, -7.0
        mix = C.mix_logits(lc.numpy(), lu.numpy(), cfg, omc)
    else:
        T = 1.0
        lc = torch.full((1, L), -6.0)
        lc[0, torch.randperm(L, generator=g)[:8]] = 0.0
        lu, cfg, omc = None, 1.0, 0.0
        mix = C.mix_logits(lc.numpy())
    a = C.scaled_logits(mix, T)[0]
    p = np.exp(a - a.max())
    p /= p.sum()
    lcd = lc.to(DEV).expand(R, L).contiguous()
    lud = None if lu is None else lu.to(DEV).expand(R, L).contiguous()
    sentinel = torch.full((R,), L, dtype=torch.int64, device=DEV)  # renoised rows carry a label outside the vocabulary
    out, pre = torch.empty(R, dtype=torch.int64, device=DEV), torch.empty(R, dtype=torch.int64, device=DEV)
    counts = torch.zeros(L, dtype=torch.int64, device=DEV)
    bad_steps = []
    for s in range(S):
        t_next = float(np.float32(1.0 - (s + 1) / (S + 1)))
        _tail_ex(lcd, lud, L, cfg, omc, T, 0, SEED_HI, s, out, pre, init=sentinel, t_next=t_next)
        counts += torch.bincount(pre, minlength=L)[:L]
        k = int((out == L).sum())
        assert int(((out != L) & (out != pre)).sum()) == 0
        sd = (R * t_next * (1 - t_next)) ** 0.5
        if abs(k - R * t_next) > 5 * sd + 1:
            bad_steps.append((s, k, R * t_next))
    counts = counts.cpu().numpy().astype(np.float64)
    n = R * S
    assert counts.sum() == n
    stat, dof, pval = _binned_chi2(counts, p, n)
    low = p < 1e-4
    P = float(p[low].sum())
    obs_low = float(counts[low].sum())
    sig = (n * P * (1 - P)) ** 0.5
    print("distribution %s: chi2 %.1f over %d dof, p = %.3g; labels with p < 1e-4: %d, expected %.1f draws, observed %d (%.2f sigma); "
          "renoise steps outside 5 sigma: %s" % (case, stat, dof, pval, int(low.sum()), n * P, obs_low, (obs_low - n * P) / max(sig, 1e-12), bad_steps))
    assert dof >= 1
    assert pval >= 1e-6, "%s: chi-square %.1f over %d dof (p = %.3g)" % (case, stat, dof, pval)
    assert abs(obs_low - n * P) <= 5 * sig + 1, "%s: labels with p < 1e-4 drawn %d times, expected %.1f" % (case, obs_low, n * P)
    assert not bad_steps, "renoise fraction outside 5 binomial sigma at (step, count, expected) %s" % bad_steps


# ---------------------------------------------------------------------------------------------------------------- (f) closed loop
@pytest.fixture(scope="module")
def tiny_sd(built_lib):
    m = paella_amd.Paella(**G.UNET_TINY)
    sd = weights_for(m, sum(G.UNET_TINY["blocks"]))
    return m.to(DEV), sd


def _record_sample(m, variant, cs, us, shape, seed, shard, kw):
    """Run sample() and record every step's (input tokens, output tokens) from the calls the loop makes."""
    rec = []
    if variant == "unfused":
        orig_fp, orig_tail = m.forward_prepared, sampling._tail

        def fp(x, *a, **k):
            rec.append([x.clone(), None])
            return orig_fp(x, *a, **k)

        def tail(*a, **k):
            orig_tail(*a, **k)
            rec[-1][1] = a[14].clone()
        m.forward_prepared, sampling._tail = fp, tail
        try:
            toks = paella_amd.sample(m, cs, shape, unconditional_inputs=us, device=DEV, noise="philox", seed=seed, shard=shard, fused_tail=False, **kw)
        finally:
            del m.forward_prepared
            sampling._tail = orig_tail
    else:
        orig = m.forward_sample

        def fs(x, r, cond, out, **k):
            xin = x.clone()
            res = orig(x, r, cond, out, **k)
            rec.append([xin, out.clone()])
            return res
        m.forward_sample = fs
        try:
            toks = paella_amd.sample(m, cs, shape, unconditional_inputs=us, device=DEV, noise="philox", seed=seed, shard=shard, **kw)
        finally:
            del m.forward_sample
    torch.cuda.synchronize()
    return toks, [(a.cpu(), b.cpu()) for a, b in rec]


@pytest.mark.parametrize("variant", ["fused", "shard", "unfused", "graph"])
def test_sample_closed_loop_against_oracle_and_model(tiny_sd, variant):
    """sample(noise="philox") on UNET_TINY, 4 steps, CFG 8, T (1.0, 0.3), renoise, a seed with its high 32 bits set: at every step the
    oracle's UNet on the DEVICE's input tokens, the model's draws (start tokens, step offset i, row offset lo*H*W, renoise) must give
    the device's output tokens, except where the model's margin is below eps = 2 (max|oracle - device mixed logit| / T + delta) + ulp."""
    m, sd = tiny_sd
    cfg = G.UNET_TINY
    L, total, H = cfg["num_labels"], 2, 16
    seed = 0xF00DFACE00C0FFEE
    steps, renoise_steps = 4, 3
    kw = dict(steps=steps, renoise_steps=renoise_steps, temperature=(1.0, 0.3), cfg=8.0)
    c_all, u_all = cond_for(cfg, total, 3, 1, 1), cond_for(cfg, total, 3, 1, 2)
    from paella_amd.dist import shard_inputs
    lo, B = (1, 1) if variant == "shard" else (0, total)
    shard = (lo, total) if variant == "shard" else None
    c, u = shard_inputs(c_all, lo, lo + B), shard_inputs(u_all, lo, lo + B)
    cs, us = to_dev(c, DEV), to_dev(u, DEV)
    shape = (B, H, H)
    if variant == "graph":
        eager, rec = _record_sample(m, "fused", cs, us, shape, seed, None, kw)
        gs = paella_amd.GraphSampler(m, cs, us, shape, device=DEV, **kw)
        toks = gs(seed=seed).clone()
        torch.cuda.synchronize()
        assert torch.equal(toks, eager), "graph replay differs from the eager call at %d positions" % int((toks != eager).sum())
    else:
        toks, rec = _record_sample(m, variant, cs, us, shape, seed, shard, kw)
    assert len(rec) == steps
    rows, row_off = B * H * H, lo * H * H
    start = C.start_tokens(seed, rows, L, row_offset=row_off)
    assert np.array_equal(rec[0][0].numpy().reshape(-1), start), "start tokens differ from the model"
    t_list = [float(v) for v in torch.linspace(1.0, 0.0, steps + 1)]
    temps = [float(v) for v in torch.linspace(1.0, 0.3, steps)]
    pair = (float(torch.tensor(8.0)), float(torch.tensor(1.0 - 8.0)))
    cache = m.prepare_cond(**to_dev({k: (torch.cat([c[k], u[k]]) if c[k] is not None else None) for k in c}, DEV))
    near_total = 0
    for i in range(steps):
        x_i, got = rec[i]
        if i:
            assert torch.equal(x_i, rec[i - 1][1]), "step %d did not start from step %d's tokens" % (i, i - 1)
        r = torch.ones(B) * t_list[i]
        with torch.no_grad():
            lc = O.unet_forward(sd, cfg, x_i, r, **c).permute(0, 2, 3, 1).reshape(rows, L).numpy()
            lu = O.unet_forward(sd, cfg, x_i, r, **u).permute(0, 2, 3, 1).reshape(rows, L).numpy()
        dev_logits = m._forward_prepared_raw(x_i.to(DEV), r.to(DEV), cache, cfg_mix=pair).reshape(rows, L).cpu().numpy()
        mix = C.mix_logits(lc, lu, *pair)
        diff = float(np.abs(dev_logits.astype(np.float64) - mix).max())
        renoise = i < renoise_steps
        t_next = t_list[i + 1] if renoise else 0.0
        pre, final, margin = C.sample_tail(lc, temps[i], seed, i, lu=lu, cfg=pair[0], omc=pair[1], row_offset=row_off,
                                           init_noise=start if renoise else None, t_next=t_next)
        mask = C.renoise_mask(seed, rows, i, t_next, row_off) if renoise else None
        inv_t = float(C.inv_temperature(temps[i]))
        top = float(np.abs(C.scaled_logits(mix, temps[i])).max()) + 17.0
        eps = _near_tie_eps(top, diff * inv_t)
        near_total += _compare_tokens("%s step %d (max |oracle - device logit| %.2e)" % (variant, i, diff), got.numpy().reshape(-1), pre, final,
                                      margin, eps, mask)
    assert torch.equal(toks.cpu(), rec[-1][1])
    print("%s: %d differing tokens at model near-ties over %d steps" % (variant, near_total, steps))
