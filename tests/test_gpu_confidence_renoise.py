"""GPU: confidence-ordered renoise and the per-token statistics -- the statistics form of the filtered tail against the fp64 model of tests/confidence_model.py
(bounds from tests/truncation_model.py's error model, every row), the renoise stage against the model's exact selection, then the samplers and the request stream."""
import functools

import numpy as np
import pytest
import torch

import paella_amd
from oracle import golden_configs as G
from paella_amd import _lib, sampling
from tests import confidence_model as CM
from tests import counter_noise as C
from tests import truncation_model as TM
from tests.helpers import cond_for, to_dev, weights_for

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -7
SEED_HI = 0xC3A5C85C97CB3127  # bit 63 set
p = _lib.ptr


def _stream():
    return _lib.stream_ptr(torch.device(DEV))


def _dev(a, dtype=None):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _f32(v):
    return torch.tensor(v, dtype=torch.float32, device=DEV)


def _seeds(v):
    return torch.tensor([sampling.seed_word(s) for s in v], dtype=torch.int64, device=DEV)


def _new(n, dtype=torch.int64, fill=SENTINEL):
    return torch.full((n,), fill, dtype=dtype, device=DEV)


# ---------------------------------------------------------------------------------------------------------------- 1. the statistics tail
FILTERS = {"off": (0, 1.0, 1.0, 1), "top_k": (7, 1.0, 1.0, 1), "typical": (0, 1.0, 0.2, 1)}
ROWS, B_REQ, HW_REQ = 32, 4, 8
REQ_TEMPS = [0.8, 1.0, 0.6, 1.3]
REQ_PAIRS = [(1.5, -0.5), (1.0, 0.0), (2.0, -1.0), (3.0, -2.0)]


@functools.lru_cache(maxsize=None)
def stats_inputs(L, with_u):
    lc, lu, cfg, omc, T = TM.candidate_logits(L, "top_k", with_u, n=ROWS)
    return lc, lu, cfg, omc, T


def _check_stats(z, top_k, tok, lp, ent, what):
    """every row: the kernel's logprob of the drawn token and its entropy within the model's bounds"""
    worst = [0.0, 0.0]
    for r in range(z.shape[0]):
        ref = CM.row_stats(z[r], top_k)
        assert ref["filtered"]
        t = int(tok[r])
        d_lp, d_h = abs(float(lp[r]) - ref["logprob"][t]), abs(float(ent[r]) - ref["entropy"])
        worst = [max(worst[0], d_lp / ref["eps_logp"][t]), max(worst[1], d_h / ref["eps_H"])]
        assert np.isfinite(ref["logprob"][t]), "%s row %d: the drawn label %d is outside A" % (what, r, t)
        assert d_lp <= ref["eps_logp"][t], "%s row %d: logprob %r vs %r, off by %.3g > %.3g" % (what, r, float(lp[r]), ref["logprob"][t], d_lp, ref["eps_logp"][t])
        assert d_h <= ref["eps_H"], "%s row %d: entropy %r vs %r, off by %.3g > %.3g" % (what, r, float(ent[r]), ref["entropy"], d_h, ref["eps_H"])
    print("%s: worst error / bound: logprob %.3f, entropy %.3f" % (what, worst[0], worst[1]))


@pytest.mark.parametrize("L", TM.GPU_SHAPES)
@pytest.mark.parametrize("with_u", (False, True), ids=("c", "cu"))
def test_stats_tail_scalar_form(built_lib, L, with_u):
    lib = built_lib
    lc, lu, cfg, omc, T = stats_inputs(L, with_u)
    nan_c = lc[:1].copy()
    nan_c[0, 5] = np.nan
    lc1, lu1 = np.concatenate([lc, nan_c]), (None if lu is None else np.concatenate([lu, lu[:1]]))
    n = ROWS + 1
    d_c, d_u = _dev(lc1), _dev(lu1)
    seed, step, row_off = SEED_HI, 5, 3
    z = TM.z_of(lc, lu, cfg, omc, T)
    plain = _new(n)
    _lib.check(lib.paella_sample_tail_ex(p(d_c), p(d_u), n, L, cfg, omc, T, 0, None, seed, None, step, row_off, None, None, None, 0.0, p(plain), None, _stream()))
    for name, f in FILTERS.items():
        want, tok, pre = _new(n), _new(n), _new(n)
        lp, ent = _new(n, torch.float32, 9.0), _new(n, torch.float32, 9.0)
        _lib.check(lib.paella_sample_tail_filter(p(d_c), p(d_u), n, L, cfg, omc, T, 0, seed, None, step, row_off, None, None, 0.0, None, None, *f, p(want), None, _stream()))
        _lib.check(lib.paella_sample_tail_stats(p(d_c), p(d_u), n, L, cfg, omc, T, 0, seed, None, step, row_off, None, None, 0.0, None, None, *f, p(tok), p(pre), p(lp), p(ent),
                                                _stream()))
        torch.cuda.synchronize()
        assert torch.equal(tok, want) and torch.equal(pre, want), "%s L=%d: the statistics changed a token" % (name, L)
        if name == "off":
            assert torch.equal(tok, plain), "filters off: not the plain tail's tokens"
        lp_h, ent_h = lp.cpu().numpy(), ent.cpu().numpy()
        _check_stats(z, f[0], tok.cpu().numpy()[:ROWS], lp_h[:ROWS], ent_h[:ROWS], "scalar %s L=%d" % (name, L))
        assert np.isneginf(lp_h[ROWS]) and np.isnan(ent_h[ROWS]) and int(tok[ROWS]) == int(plain[ROWS]), "a NaN row reports -inf / NaN and draws the plain tail's token"
        # either output alone: the same tokens, the same values
        only = _new(n, torch.float32, 9.0)
        tok2 = _new(n)
        _lib.check(lib.paella_sample_tail_stats(p(d_c), p(d_u), n, L, cfg, omc, T, 0, seed, None, step, row_off, None, None, 0.0, None, None, *f, p(tok2), None, None, p(only),
                                                _stream()))
        torch.cuda.synchronize()
        assert torch.equal(tok2, want) and np.array_equal(only.cpu().numpy(), ent_h, equal_nan=True)


@pytest.mark.parametrize("L", TM.GPU_SHAPES)
@pytest.mark.parametrize("with_u", (False, True), ids=("c", "cu"))
def test_stats_tail_request_form(built_lib, L, with_u):
    lib = built_lib
    lc, lu, _, _, _ = stats_inputs(L, with_u)
    rows = B_REQ * HW_REQ
    d_c, d_u = _dev(lc), _dev(lu)
    seeds, temps, pairs = _seeds([SEED_HI, 3, (1 << 64) - 2, 77]), _f32(REQ_TEMPS), (_f32(REQ_PAIRS) if with_u else None)
    step, never, init = _i32([3, 0, 7, 1]), _f32([-1.0] * B_REQ), torch.zeros(rows, dtype=torch.int64, device=DEV)
    z = np.concatenate([TM.z_of(lc[b * HW_REQ:(b + 1) * HW_REQ], None if lu is None else lu[b * HW_REQ:(b + 1) * HW_REQ], *(REQ_PAIRS[b] if with_u else (1.0, 0.0)), REQ_TEMPS[b])
                        for b in range(B_REQ)])
    for name, f in FILTERS.items():
        fk, fm = _i32([[f[0], f[3]]] * B_REQ), _f32([[f[1], f[2]]] * B_REQ)
        for active in ([1, 1, 1, 1], [1, 0, 1, 1]):
            act = _i32(active)
            want, tok = _new(rows), _new(rows)
            lp, ent = _new(rows, torch.float32, 9.0), _new(rows, torch.float32, 9.0)
            head = [p(d_c), p(d_u), rows, L, p(pairs), p(temps), p(seeds), HW_REQ, p(step), p(never), p(act), p(init), None, None, None]
            _lib.check(lib.paella_sample_tail_stream_filter(*head, p(fk), p(fm), p(want), None, _stream()))
            _lib.check(lib.paella_sample_tail_stream_stats(*head, p(fk), p(fm), p(tok), None, p(lp), p(ent), _stream()))
            torch.cuda.synchronize()
            assert torch.equal(tok, want), "%s L=%d: the statistics changed a token" % (name, L)
            on = np.repeat(np.array(active, bool), HW_REQ)
            lp_h, ent_h, tok_h = lp.cpu().numpy(), ent.cpu().numpy(), tok.cpu().numpy()
            assert (tok_h[~on] == SENTINEL).all() and (lp_h[~on] == 9.0).all() and (ent_h[~on] == 9.0).all(), "an inactive slot's rows were written"
            _check_stats(z[on], f[0], tok_h[on], lp_h[on], ent_h[on], "request %s L=%d" % (name, L))
            if name == "off":  # no filter tables at all: every request off; and the plain stream tail's tokens
                plain, tok3 = _new(rows), _new(rows)
                lp3 = _new(rows, torch.float32, 9.0)
                _lib.check(lib.paella_sample_tail_stream(*head[:12], p(plain), None, _stream()))
                _lib.check(lib.paella_sample_tail_stream_stats(*head, None, None, p(tok3), None, p(lp3), None, _stream()))
                torch.cuda.synchronize()
                assert torch.equal(tok, plain) and torch.equal(tok3, plain) and torch.equal(lp3, lp)


# ---------------------------------------------------------------------------------------------------------------- 2. the renoise stage
HWS = (1, 7, 256, 1000, 16384)
T_NEXT = (-1.0, 0.0, 0.25, 0.37, 1.0)
L_TOK = 8192


def hand_logprob(n, seed):
    """fp32 [n]: a few distinct values repeated many times (ties), with -inf, a NaN and both zeros among them"""
    rng = np.random.default_rng([41, n, seed])
    vals = np.float32([-0.0, 0.0, -0.25, -0.25, -1.5, -3.0, -7.75, -np.inf, -1e-30, -12.0])
    lp = vals[rng.integers(0, vals.size, n)]
    if n > 2:
        lp[rng.integers(0, n)] = np.nan
        lp[rng.integers(0, n)] = -np.inf
        lp[rng.integers(0, n)] = -0.0
    return lp


def stage_inputs(B, HW, seed=0):
    rng = np.random.default_rng([43, B, HW, seed])
    rows = B * HW
    return (np.concatenate([hand_logprob(HW, seed + b) for b in range(B)]), rng.integers(0, L_TOK, rows), rng.integers(0, L_TOK, rows), rng.integers(0, L_TOK, rows),
            rng.integers(0, 2, rows))


def _expect(scores, drawn, init, free, known, t_next, HW):
    """the stage's output for policy-1 samples from the scores it ranked: per sample, init where selected, known where pinned, else the draw"""
    out = drawn.copy()
    for b in range(scores.size // HW):
        sl = slice(b * HW, (b + 1) * HW)
        sel = CM.select(scores[sl], free[sl], t_next[b])
        assert sel.sum() == CM.renoise_count(t_next[b], int(free[sl].sum())) and not (sel & ~free[sl]).any()
        out[sl] = np.where(free[sl], np.where(sel, init[sl], drawn[sl]), known[sl])
    return out


@pytest.mark.parametrize("HW", HWS)
def test_renoise_stage_scalar_form(built_lib, HW):
    lib, B = built_lib, 3
    rows = B * HW
    lp, drawn, init, known, keep = stage_inputs(B, HW)
    d_lp, d_drawn, d_init, d_known, d_keep = _dev(lp), _dev(drawn), _dev(init), _dev(known), _dev(keep)
    seed, step = SEED_HI, 2
    all_free = np.ones(rows, bool)
    for t in T_NEXT:
        # g = 0: the output equals the model's selection on the inputs; with the pin the count is over the free positions and the known tokens are in place
        for pin in (False, True):
            out = _new(rows)
            _lib.check(lib.paella_renoise_select(p(d_drawn), p(d_lp), p(d_init), rows, HW, seed, None, step, 0, None, t, 1, 0.0, p(d_keep) if pin else None,
                                                 p(d_known) if pin else None, p(out), _stream()))
            torch.cuda.synchronize()
            free = keep != 0 if pin else all_free
            want = _expect(lp, drawn, init, free, known, [t] * B, HW)
            assert np.array_equal(out.cpu().numpy(), want), "HW=%d t_next=%r pin=%r: %d tokens differ from the model" % (HW, t, pin, int((out.cpu().numpy() != want).sum()))
        # g = 4.5: the hook's scores within the stated bound of the fp64 model, the output the model's selection on those scores
        out, scores = _new(rows), _new(rows, torch.float32, 9.0)
        _lib.check(lib.paella_test_renoise_scores(p(d_drawn), p(d_lp), p(d_init), rows, HW, seed, step, 0, t, 1, 4.5, None, None, None, None, None, None, None, None, None,
                                                  p(out), p(scores), _stream()))
        torch.cuda.synchronize()
        sc = scores.cpu().numpy()
        ref, bound = CM.score64(lp, 4.5, t, CM.renoise_words(seed, np.arange(rows), step)[1])
        fin = np.isfinite(ref)
        assert np.array_equal(np.isnan(sc), np.isnan(ref)) and np.array_equal(sc[~fin & ~np.isnan(ref)], ref[~fin & ~np.isnan(ref)])
        assert (np.abs(sc[fin] - ref[fin]) <= bound[fin]).all(), "HW=%d t_next=%r: a score is off by %.3g (bound %.3g)" % (
            HW, t, np.abs(sc[fin] - ref[fin]).max(), bound[fin][np.abs(sc[fin] - ref[fin]).argmax()])
        want = _expect(sc, drawn, init, all_free, known, [t] * B, HW)
        assert np.array_equal(out.cpu().numpy(), want), "HW=%d t_next=%r g=4.5: tokens differ from the model's selection on the kernel's scores" % (HW, t)
        plain = _new(rows)
        _lib.check(lib.paella_renoise_select(p(d_drawn), p(d_lp), p(d_init), rows, HW, seed, None, step, 0, None, t, 1, 4.5, None, None, p(plain), _stream()))
        # in place, and one sample at a time with its global row offset (a batch shard)
        alias = d_drawn.clone()
        _lib.check(lib.paella_renoise_select(p(alias), p(d_lp), p(d_init), rows, HW, seed, None, step, 0, None, t, 1, 4.5, None, None, p(alias), _stream()))
        k = B - 1
        sl = slice(k * HW, (k + 1) * HW)
        part, part0, d_dk, d_lk, d_ik = _new(HW), _new(HW), d_drawn[sl].clone(), d_lp[sl].clone(), d_init[sl].clone()
        roff = torch.tensor([HW], dtype=torch.int64, device=DEV)
        _lib.check(lib.paella_renoise_select(p(d_dk), p(d_lk), p(d_ik), HW, HW, seed, None, step, (k - 1) * HW, p(roff), t, 1, 4.5, None, None, p(part), _stream()))
        _lib.check(lib.paella_renoise_select(p(d_dk), None, p(d_ik), HW, HW, seed, None, step, k * HW, None, t, 0, 0.0, None, None, p(part0), _stream()))
        torch.cuda.synchronize()
        assert torch.equal(plain, out) and torch.equal(alias, out), "HW=%d t_next=%r: the hook, the entry point and the in-place call disagree" % (HW, t)
        assert torch.equal(part, out[sl]), "HW=%d t_next=%r: a shard with row_offset = k * HW differs from its rows of the unsharded call" % (HW, t)
        coin = C.renoise_mask(seed, rows, step, t)[sl]
        assert np.array_equal(part0.cpu().numpy(), np.where(coin, init[sl], drawn[sl])), "HW=%d t_next=%r: policy 0 differs from the model of the random mask" % (HW, t)


@pytest.mark.parametrize("HW", HWS)
def test_renoise_stage_stream_form(built_lib, HW):
    lib, B, L = built_lib, 4, 64
    rows = B * HW
    lp, _, init, known, keep = stage_inputs(B, HW, seed=1)
    seed_v = [SEED_HI, 3, (1 << 64) - 2, 77]
    seeds, step_v = _seeds(seed_v), [3, 0, 7, 1]
    step, temps = _i32(step_v), _f32([0.8, 1.0, 0.6, 1.3])
    d_lp, d_init, d_known, d_keep = _dev(lp), _dev(init), _dev(known), _dev(keep)
    logits = torch.randn(rows, L, generator=torch.Generator().manual_seed(HW)).to(DEV)
    for rot in range(2):
        t_v = [T_NEXT[(b + 2 * rot + (HW % 3)) % 5] for b in range(B)]
        if rot == 1:
            t_v[0] = 0.37  # (the policy-0 slot renoises something)
        t_next = _f32(t_v)
        for active in ([1, 1, 1, 1], [1, 1, 0, 1]):
            act, policy, noise = _i32(active), _i32([0, 1, 1, 1]), _f32([4.5, 0.0, 0.0, 0.0])
            on = np.repeat(np.array(active, bool), HW)
            # the plain stream tail with init_noise: its raw draw feeds the stage, its tokens are what a policy-0 slot must reproduce
            tail_tok, drawn_t = _new(rows), _new(rows)
            _lib.check(lib.paella_sample_tail_stream(p(logits), None, rows, L, None, p(temps), p(seeds), HW, p(step), p(t_next), p(act), p(d_init), p(tail_tok), p(drawn_t),
                                                     _stream()))
            torch.cuda.synchronize()
            drawn = drawn_t.cpu().numpy()
            out = _new(rows)
            _lib.check(lib.paella_renoise_select_stream(p(drawn_t), p(d_lp), p(d_init), rows, HW, p(seeds), p(step), p(t_next), p(act), p(policy), p(noise), None, None, None,
                                                        p(out), _stream()))
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert (got[~on] == SENTINEL).all(), "an inactive slot's rows were written"
            assert torch.equal(out[:HW], tail_tok[:HW]), "HW=%d: the policy-0 slot differs from paella_sample_tail_stream with init_noise" % HW
            want = _expect(lp, drawn, init, np.ones(rows, bool), known, t_v, HW)
            sl = on.copy()
            sl[:HW] = False
            assert np.array_equal(got[sl], want[sl]), "HW=%d t_next=%r: policy-1 slots differ from the model at %d tokens" % (HW, t_v, int((got[sl] != want[sl]).sum()))
            # the pin: slot 1 is not pinned (pin_on = 0), the others are; the count is over the free positions; g = 4.5 on slot 3 through the hook's scores
            pin_on, noise2 = _i32([1, 0, 1, 1]), _f32([0.0, 0.0, 0.0, 4.5])
            out2, scores = drawn_t.clone(), _new(rows, torch.float32, 9.0)
            _lib.check(lib.paella_test_renoise_scores(p(out2), p(d_lp), p(d_init), rows, HW, 0, 0, 0, 0.0, 0, 0.0, p(seeds), p(step), p(t_next), p(act), p(policy), p(noise2),
                                                      p(d_keep), p(d_known), p(pin_on), p(out2), p(scores), _stream()))
            torch.cuda.synchronize()
            got2, sc = out2.cpu().numpy(), scores.cpu().numpy()
            free = keep != 0
            free[HW:2 * HW] = True
            assert np.array_equal(got2[on & ~free], known[on & ~free]), "known positions do not hold the known tokens"
            ref, bound = CM.score64(lp[3 * HW:], 4.5, t_v[3], CM.renoise_words(seed_v[3], np.arange(HW), step_v[3])[1])
            fin = np.isfinite(ref) & free[3 * HW:]
            assert (np.abs(sc[3 * HW:][fin] - ref[fin]) <= bound[fin]).all(), "slot 3: a perturbed score is outside its bound"
            assert np.array_equal(sc[HW:3 * HW][on[HW:3 * HW]], lp[HW:3 * HW][on[HW:3 * HW]], equal_nan=True), "g = 0: the score is the logprob"
            want2 = _expect(np.where(on, sc, lp), drawn, init, free, known, t_v, HW)
            assert np.array_equal(got2[sl], want2[sl]), "HW=%d t_next=%r: pinned policy-1 slots differ from the model at %d tokens" % (HW, t_v, int((got2[sl] != want2[sl]).sum()))
            coin = C.renoise_mask(seed_v[0], HW, step_v[0], t_v[0])
            assert np.array_equal(got2[:HW], np.where(free[:HW], np.where(coin, init[:HW], drawn[:HW]), known[:HW])), "the pinned policy-0 slot differs from the model"
            assert (got2[~on] == drawn[~on]).all(), "an inactive slot's rows were written (in place)"


# ---------------------------------------------------------------------------------------------------------------- models
@pytest.fixture(scope="module")
def tiny(built_lib):
    m = paella_amd.Paella(**G.UNET_TINY)
    weights_for(m, sum(G.UNET_TINY["blocks"]))
    return m.to(DEV)


def _conds(B, seed=1):
    return to_dev(cond_for(G.UNET_TINY, B, 3, 0, seed), DEV), to_dev(cond_for(G.UNET_TINY, B, 3, 0, seed + 1), DEV)


KW = dict(steps=4, renoise_steps=3)
H = 8


def _compose(tiny, cs, us, B, s, cfg, policy, g, check_counts=True):
    """step by step on the host: forward_prepared (guidance folded through the head), the statistics entry point, paella_renoise_select"""
    L, rows, hw = G.UNET_TINY["num_labels"], B * H * H, H * H
    steps, renoise_steps = KW["steps"], KW["renoise_steps"]
    t_list = sampling.linspace_schedule(1.0, 0.0, steps + 1)
    temps = sampling.linspace_schedule(1.0, 0.2, steps)
    if cfg:
        pair = (float(torch.tensor(cfg, dtype=torch.float32)), float(torch.tensor(1.0 - cfg, dtype=torch.float32)))
        cache = tiny.prepare_cond(**{k: (torch.cat([cs[k], us[k]]) if cs[k] is not None else None) for k in cs})
    else:
        pair, cache = None, tiny.prepare_cond(**cs)
    init = sampling.start_tokens(L, (B, H, H), s, DEV)
    x = init.clone()
    lib = _lib.load()
    lp, ent = (torch.empty(B, H, H, dtype=torch.float32, device=DEV) for _ in range(2))
    for i in range(steps):
        logits = tiny._forward_prepared_raw(x, torch.full((B,), t_list[i], device=DEV), cache, **({} if pair is None else {"cfg_mix": pair})).reshape(rows, L).contiguous()
        drawn = torch.empty(B, H, H, dtype=torch.int64, device=DEV)
        _lib.check(lib.paella_sample_tail_stats(p(logits), None, rows, L, 1.0, 0.0, temps[i], 0, s, None, i, 0, None, None, 0.0, None, None, 0, 1.0, 1.0, 1, p(drawn), None,
                                                p(lp), p(ent), _stream()))
        x = drawn
        if i < renoise_steps:
            x = torch.empty_like(drawn)
            _lib.check(lib.paella_renoise_select(p(drawn), p(lp), p(init), rows, hw, s, None, i, 0, None, t_list[i + 1], policy, g, None, None, p(x), _stream()))
            torch.cuda.synchronize()
            if check_counts and policy == 1:
                d, o, n0 = drawn.cpu().numpy().reshape(B, hw), x.cpu().numpy().reshape(B, hw), init.cpu().numpy().reshape(B, hw)
                n = CM.renoise_count(t_list[i + 1], hw)
                for b in range(B):
                    changed = o[b] != d[b]
                    assert (o[b][changed] == n0[b][changed]).all() and changed.sum() <= n
                    if g == 0:
                        sel = CM.select(lp.cpu().numpy().reshape(B, hw)[b], np.ones(hw, bool), t_list[i + 1])
                        assert sel.sum() == n and np.array_equal(o[b], np.where(sel, n0[b], d[b])), "step %d sample %d: not exactly the %d least confident positions" % (i, b, n)
                        assert changed.sum() == (sel & (n0[b] != d[b])).sum()
    torch.cuda.synchronize()
    return x, lp.clone(), ent.clone()


@pytest.mark.parametrize("cfg", (4.0, None), ids=("guided", "unguided"))
def test_sample_equals_the_host_composition_the_graph_and_the_shards(tiny, cfg):
    from paella_amd.dist import shard_inputs
    B, s = 2, SEED_HI
    cs, us = _conds(B)
    un = dict(unconditional_inputs=us) if cfg else {}
    kw = dict(cfg=cfg, device=DEV, noise="philox", seed=s, **KW)
    for g in (0.0, 4.5):
        want, lp, ent = _compose(tiny, cs, us, B, s, cfg, 1, g)
        got, st = paella_amd.sample(tiny, cs, (B, H, H), renoise="confidence", confidence_noise=g, return_stats=True, **un, **kw)
        assert torch.equal(got, want), "g=%r: sample(renoise='confidence') differs from the host composition at %d tokens" % (g, int((got != want).sum()))
        assert torch.equal(st["logprob"], lp) and torch.equal(st["entropy"], ent) and st["logprob"].shape == (B, H, H) and st["entropy"].dtype == torch.float32
        assert torch.equal(paella_amd.sample(tiny, cs, (B, H, H), renoise="confidence", confidence_noise=g, fused_tail=False, **un, **kw), want)
        gs = paella_amd.GraphSampler(tiny, cs, us if cfg else None, (B, H, H), cfg=cfg, device=DEV, renoise="confidence", confidence_noise=g, return_stats=True, **KW)
        g_tok, g_st = gs(seed=s)
        assert torch.equal(g_tok, want) and torch.equal(g_st["logprob"], lp) and torch.equal(g_st["entropy"], ent), "GraphSampler differs from the eager call"
        parts = [paella_amd.sample(tiny, shard_inputs(cs, lo, lo + 1), (1, H, H), renoise="confidence", confidence_noise=g, shard=(lo, B),
                                   **(dict(unconditional_inputs=shard_inputs(us, lo, lo + 1)) if cfg else {}), **kw) for lo in range(B)]
        assert torch.equal(torch.cat(parts), want), "g=%r: the two shards differ from the unsharded call" % g
    plain = paella_amd.sample(tiny, cs, (B, H, H), **un, **kw)
    assert not torch.equal(plain, want), "renoise='confidence' changed no token"
    tok, st = paella_amd.sample(tiny, cs, (B, H, H), return_stats=True, **un, **kw)
    assert torch.equal(tok, plain), "return_stats alone changed %d tokens" % int((tok != plain).sum())
    rnd, lp0, ent0 = _compose(tiny, cs, us, B, s, cfg, 0, 0.0)
    assert torch.equal(rnd, plain) and torch.equal(st["logprob"], lp0) and torch.equal(st["entropy"], ent0), "policy 0 through the stage is not the plain call"
    assert bool((st["logprob"] <= 0).all()) and bool((st["entropy"] >= -1e-6).all())
    # with a filter: the statistics tail is the filtered tail
    f_tok, _ = paella_amd.sample(tiny, cs, (B, H, H), return_stats=True, top_k=5, **un, **kw)
    assert torch.equal(f_tok, paella_amd.sample(tiny, cs, (B, H, H), top_k=5, **un, **kw))


def test_sample_requests_with_per_request_policies(tiny):
    B, seeds = 3, [SEED_HI, 5, 77]
    cs, us = _conds(B, 3)
    kw = dict(cfg=[4.0, 2.0, (5.0, 3.0)], temperature=[(1.0, 0.2), (0.9, 0.5), (1.0, 0.3)], device=DEV, **KW)
    pol, gs_ = ["confidence", "random", "confidence"], [0.0, 2.0, 4.5]
    mixed = paella_amd.sample_requests(tiny, cs, us, (B, H, H), seeds, renoise=pol, confidence_noise=gs_, **kw)
    for b in range(B):
        same = paella_amd.sample_requests(tiny, cs, us, (B, H, H), seeds, renoise=pol[b], confidence_noise=gs_[b], **kw)
        assert torch.equal(mixed[b], same[b]), "request %d depends on its batch-mates' policies (%d tokens differ)" % (b, int((mixed[b] != same[b]).sum()))
    plain = paella_amd.sample_requests(tiny, cs, us, (B, H, H), seeds, **kw)
    assert torch.equal(mixed[1], plain[1]) and not torch.equal(mixed[0], plain[0]) and not torch.equal(mixed[2], plain[2])
    # a request of the batch is the batch-of-one sample() with its values
    from paella_amd.dist import shard_inputs
    one = paella_amd.sample(tiny, shard_inputs(cs, 0, 1), (1, H, H), unconditional_inputs=shard_inputs(us, 0, 1), cfg=4.0, device=DEV, noise="philox", seed=seeds[0],
                            renoise="confidence", **KW)
    alone = paella_amd.sample_requests(tiny, shard_inputs(cs, 0, 1), shard_inputs(us, 0, 1), (1, H, H), seeds[:1], cfg=4.0, device=DEV, renoise="confidence", **KW)
    assert torch.equal(alone, one)


# ---------------------------------------------------------------------------------------------------------------- 4. request stream
def _one(seed):
    return to_dev(cond_for(G.UNET_TINY, 1, 3, 0, seed), DEV), to_dev(cond_for(G.UNET_TINY, 1, 3, 0, seed + 100), DEV)


def _request(cseed, **kw):
    c, u = _one(cseed)
    return dict(model_inputs=c, unconditional_inputs=u, **kw)


def _hold_one(st):
    """slot 0 taken by a finished, uncollected one-step request: the next request lands in slot 1"""
    st.admit(**_request(60, seed=0, steps=1))
    assert st.tick() == [0] and st.free_slots[0] == 1


def _until(st, slot, **kw):
    for _ in range(16):
        for b in st.tick():
            res = st.result(b, **(kw if b == slot else {}))
            if b == slot:
                return res
    raise AssertionError("the request of slot %d did not finish" % slot)


def test_request_stream_with_confidence(tiny):
    """32x32 tokens (no 16-row block straddles two samples: the condition of the stream's bit-for-bit contract)"""
    HS, B = 32, 3
    ex_c, ex_u = _one(1)
    new = lambda **kw: paella_amd.RequestStream(tiny, ex_c, ex_u, (B, HS, HS), max_steps=6, device=DEV, **kw)
    X = _request(50, seed=SEED_HI, cfg=(9.0, 5.0), steps=4, temperature=(0.9, 0.3), renoise="confidence", confidence_noise=4.5)
    Y = _request(51, seed=77, cfg=3.0, steps=3)                                     # random
    alone = new(confidence=True)
    _hold_one(alone)
    assert alone.admit(**X) == 1
    tok_alone, maps_alone = _until(alone, 1, stats=True)
    assert maps_alone["logprob"].shape == (HS, HS) and bool((maps_alone["logprob"] <= 0).all()) and bool((maps_alone["entropy"] >= -1e-6).all())
    # run A: admitted at tick 0 next to a random and a g = 0 confidence request
    a = new(confidence=True)
    a.admit(**_request(2, seed=1, steps=3))
    assert a.admit(**X) == 1
    a.admit(**_request(4, seed=3, steps=6, temperature=(0.7, 0.7), renoise="confidence"))
    tok_a, maps_a = _until(a, 1, stats=True)
    # run B: admitted at tick 2 into a stream with other requests mid-flight; slot 1 held a confidence request before
    b = new(confidence=True)
    b.admit(**_request(7, seed=11, steps=6, cfg=(2.0, 6.0), renoise="confidence", confidence_noise=1.0))
    assert b.admit(**_request(9, seed=13, steps=2, renoise="confidence")) == 1
    b.admit(**_request(8, seed=12, steps=5, temperature=(1.2, 0.4)))
    for _ in range(2):
        for s_ in b.tick():
            b.result(s_)
    assert b.free_slots == [1] and b.admit(**X) == 1
    tok_b, maps_b = _until(b, 1, stats=True)
    for tok, maps, what in ((tok_a, maps_a, "batch-mates"), (tok_b, maps_b, "admission tick")):
        assert torch.equal(tok, tok_alone), "a confidence request depends on its %s (%d tokens differ)" % (what, int((tok != tok_alone).sum()))
        assert torch.equal(maps["logprob"], maps_alone["logprob"]) and torch.equal(maps["entropy"], maps_alone["entropy"]), "its maps depend on its %s" % what
    # a random request equals the confidence=False stream's; slot 1 is reused after the confidence request X and must not inherit its policy
    plain = new()
    _hold_one(plain)
    assert plain.admit(**Y) == 1
    tok_plain = _until(plain, 1)
    for _ in range(8):
        for s_ in b.tick():
            b.result(s_)
    assert not b.active and b.free_slots == [0, 1, 2]
    _hold_one(b)
    assert b.admit(**Y) == 1 and b.policy.cpu().tolist()[1] == 0 and b.confidence_noise.cpu().tolist()[1] == 0.0
    assert torch.equal(_until(b, 1), tok_plain), "a random request in a slot a confidence request left differs from the confidence=False stream"
    plain.reset()
    _hold_one(plain)
    assert plain.admit(**dict(X, renoise="random")) == 1
    assert not torch.equal(_until(plain, 1), tok_alone), "renoise='confidence' changed no token of the request"
    a.admit(**X)
    a.reset()
    assert a.policy.cpu().tolist() == [0] * B and a.confidence_noise.cpu().tolist() == [0.0] * B
    torch.cuda.synchronize()
    assert a.captures == 1 and b.captures == 1 and alone.captures == 1 and plain.captures == 1
    with pytest.raises(ValueError, match="renoise"):
        plain.admit(**X)


def test_request_stream_confidence_composes_with_editing_and_filtering(tiny):
    HS, L = 16, G.UNET_TINY["num_labels"]
    c, u = _one(5)
    g = torch.Generator().manual_seed(8)
    known = torch.randint(0, L, (HS, HS), generator=g).to(DEV)
    mask = torch.randint(0, 2, (HS, HS), generator=g).to(DEV)
    # editing, pin="step", on a one-slot stream: the tokens of sample_distributed(pin=, renoise="confidence") started from the same tokens
    st = paella_amd.RequestStream(tiny, c, u, (1, HS, HS), max_steps=4, device=DEV, confidence=True, editing=True)
    seed, kw = 10, dict(steps=4, temperature=(1.0, 0.2), cfg=(4.0, 4.0))
    assert st.admit(c, u, seed=seed, known=known, mask=mask, pin="step", renoise="confidence", confidence_noise=2.0, **kw) == 0
    start = st.tokens.clone()
    seen = []
    for _ in range(4):
        done = st.tick()
        seen.append(st.tokens[0].clone())
    assert done == [0]
    tok = st.result(0)
    assert all(torch.equal(t[mask == 0], known[mask == 0]) for t in seen), "the known tokens did not survive every tick"
    ref = paella_amd.sample_distributed(tiny, c, u, (1, HS, HS), init_x=start, noise="philox", seed=seed, pin=(mask[None].contiguous(), known[None].contiguous()),
                                        renoise="confidence", confidence_noise=2.0, **kw)
    assert torch.equal(tok, ref[0]), "the editing request differs from sample_distributed(pin=, renoise='confidence') at %d tokens" % int((tok != ref[0]).sum())
    assert 0 < int((mask == 0).sum()) < HS * HS and st.captures == 1
    # filtering: a top-k request with confidence renoise next to a plain one; the filter and the policy both act
    ex_c, ex_u = _one(1)
    new = lambda **k: paella_amd.RequestStream(tiny, ex_c, ex_u, (2, HS, HS), max_steps=4, device=DEV, **k)
    both, conf_only, filt_only = new(confidence=True, filtering=True), new(confidence=True), new(filtering=True)
    R = _request(6, seed=9, steps=3)
    toks = []
    for s_, extra in ((both, dict(top_k=16, renoise="confidence")), (conf_only, dict(renoise="confidence")), (filt_only, dict(top_k=16)), (both, dict())):
        s_.admit(**_request(7, seed=4, steps=2))
        assert s_.admit(**R, **extra) == 1
        toks.append(_until(s_, 1))
        for _ in range(4):
            for d in s_.tick():
                s_.result(d)
    assert not torch.equal(toks[0], toks[1]) and not torch.equal(toks[0], toks[2]), "top_k=16 or the confidence policy changed no token"
    plain = new()
    plain.admit(**_request(7, seed=4, steps=2))
    assert plain.admit(**R) == 1
    assert torch.equal(toks[3], _until(plain, 1)), "a request with neither on differs from the plain stream"
    assert both.captures == 1
