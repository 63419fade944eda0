"""GPU: truncated sampling (top-k, nucleus, typical filtering): `sample_tail_filter_kernel` against the fp64 model of tests/truncation_model.py, then the samplers.
Inputs are chosen, never outputs: a row is used only when the model reports an empty band (no label whose membership the kernel's fp32 error could change), so
every comparison in this file is exact -- kept sets, tokens, and "filter off == the plain tail" bit for bit."""
import functools

import numpy as np
import pytest
import torch

import paella_amd
from oracle import golden_configs as G
from paella_amd import _lib, sampling
from tests import counter_noise as C
from tests import truncation_model as TM
from tests.helpers import cond_for, to_dev, weights_for

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -7
SEED_HI = 0xC3A5C85C97CB3127  # bit 63 set
ROWS, B_REQ, HW_REQ = 37, 3, 16
OFF = dict(top_k=0, top_p=1.0, typical_mass=1.0, min_tokens=1)


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


def _full(f):
    return dict(OFF, **f)


def _pick(lc, lu, cfg, omc, T, filt, n):
    """the first n rows with an empty band -> (row indices, kept [n, L])"""
    kept, band = TM.truncate_rows(TM.z_of(lc, lu, cfg, omc, T), **filt)
    idx = np.nonzero(~band.any(axis=1))[0][:n]
    assert idx.size == n, "only %d of %d candidate rows have an empty band" % (idx.size, lc.shape[0])
    return idx, kept[idx]


@functools.lru_cache(maxsize=None)
def scalar_case(L, name, with_u):
    """37 rows: 33 random ones with an empty band plus an all-equal row, a one-hot-dominated row, a row with -inf labels and a NaN row"""
    filt = TM.GPU_FILTERS[name]
    lc, lu, cfg, omc, T, _, _ = TM.select_rows(L, name, with_u, ROWS - 4)
    rng = np.random.default_rng([7, L, int(with_u)])
    sp_c = np.zeros((4, L), np.float32)
    sp_c[1, 5] = 40.0                                                   # one label carries all the mass
    sp_c[2] = lc[0]
    sp_c[2, rng.choice(L, L // 4, replace=False)] = -np.inf             # -inf labels: probability 0
    sp_c[3] = lc[1]
    sp_c[3, 3] = np.nan                                                 # a NaN: the row is not filtered
    sp_u = None
    if with_u:
        sp_u = np.zeros((4, L), np.float32)
        sp_u[2], sp_u[3] = lu[0], lu[1]
    lc = np.concatenate([lc, sp_c])
    lu = None if lu is None else np.concatenate([lu, sp_u])
    kept, band = TM.truncate_rows(TM.z_of(lc, lu, cfg, omc, T), **filt)
    assert not band.any(), "a special row of %s at L=%d has a non-empty band" % (name, L)
    assert kept[ROWS - 4].all() and kept[ROWS - 1].all(), "all-equal and NaN rows keep every label"
    if "top_p" in filt or "typical_mass" in filt:  # the dominated row keeps its one label -- or, when min_tokens reaches into the tie of all the others, everything
        assert kept[ROWS - 3].sum() == (L if filt.get("min_tokens", 1) > 1 else 1)
    return lc, lu, cfg, omc, T, kept


REQ_FILTERS = ("top_p", "typical", "top_k+typical", "min_tokens")
REQ_PAIRS = [(1.5, -0.5), (1.0, 0.0), (2.0, -1.0)]
REQ_TEMPS = [0.8, 1.0, 0.6]


@functools.lru_cache(maxsize=None)
def request_case(L, name, with_u):
    """B = 3 requests of 16 rows: request 0 carries the case's filter, request 1 none, request 2 typical_mass + min_tokens; own guidance pair and temperature each"""
    filters = [TM.GPU_FILTERS[name], {}, TM.GPU_FILTERS["typical+min_tokens"]]
    rng = np.random.default_rng([11, L, sorted(TM.GPU_FILTERS).index(name), int(with_u)])
    lcs, lus, kepts = [], [], []
    for b in range(B_REQ):
        lc = (rng.standard_normal((64, L)) * TM.GPU_SCALE).astype(np.float32)
        lu = (rng.standard_normal((64, L)) * TM.GPU_SCALE).astype(np.float32) if with_u else None
        cfg, omc = REQ_PAIRS[b] if with_u else (1.0, 0.0)
        idx, kept = _pick(lc, lu, cfg, omc, REQ_TEMPS[b], filters[b], HW_REQ)
        lcs.append(lc[idx]), lus.append(None if lu is None else lu[idx]), kepts.append(kept)
    fk = np.int32([[_full(f)["top_k"], _full(f)["min_tokens"]] for f in filters])
    fm = np.float32([[_full(f)["top_p"], _full(f)["typical_mass"]] for f in filters])
    return np.concatenate(lcs), (np.concatenate(lus) if with_u else None), np.concatenate(kepts), fk, fm


def _keep_scalar(lib, lc, lu, L, cfg, omc, T, f):
    rows = lc.size(0)
    keep = torch.full((rows, L), 9, dtype=torch.uint8, device=DEV)
    rec = torch.zeros(rows, 4, device=DEV)
    _lib.check(lib.paella_test_tail_filter_keep(_lib.ptr(lc), _lib.ptr(lu), rows, L, cfg, omc, T, f["top_k"], f["top_p"], f["typical_mass"], f["min_tokens"], None, None,
                                                None, 0, None, None, _lib.ptr(keep), _lib.ptr(rec), _stream()))
    torch.cuda.synchronize()
    return keep.cpu().numpy().astype(bool), rec.cpu().numpy()


def _first_argmax(scores, kept):
    s = np.where(np.isnan(scores), -np.inf, scores)
    return np.where(kept, s, -np.inf).argmax(axis=1)


SHAPES = [(L, u) for L in TM.GPU_SHAPES for u in (False, True)]


# ---------------------------------------------------------------------------------------------------------------- 1. + 2. kept set and token, scalar form
@pytest.mark.parametrize("L,with_u", SHAPES, ids=lambda v: str(v))
def test_kept_set_and_token_scalar_form(built_lib, L, with_u):
    seed, step, row_off = SEED_HI, 5, 3
    for name in sorted(TM.GPU_FILTERS):
        lc, lu, cfg, omc, T, kept = scalar_case(L, name, with_u)
        f = _full(TM.GPU_FILTERS[name])
        d_c, d_u = _dev(lc), _dev(lu)
        got, rec = _keep_scalar(built_lib, d_c, d_u, L, cfg, omc, T, f)
        bad = np.nonzero((got != kept).any(axis=1))[0]
        assert bad.size == 0, "%s L=%d: kept set differs from the model on rows %s (row %d: kernel keeps %d, model %d)" % (
            name, L, bad.tolist(), bad[0], got[bad[0]].sum(), kept[bad[0]].sum())
        z = TM.z_of(lc, lu, cfg, omc, T)
        ref = TM.truncate_row(z[0], **TM.GPU_FILTERS[name])
        assert rec[0, 0] == ref["m"] and abs(rec[0, 1] - ref["logsum"]) < 1e-4 and abs(rec[0, 2] - ref["H"]) < 1e-4 and abs(rec[0, 3] - ref["threshold"]) < 1e-4, (rec[0], ref)
        assert np.isnan(rec[ROWS - 1]).all(), "a NaN row has no record"
        # the token: the first arg-max of the unfiltered scores over the model's kept set
        tok = torch.full((ROWS,), SENTINEL, dtype=torch.int64, device=DEV)
        pre = tok.clone()
        _lib.check(built_lib.paella_sample_tail_filter(_lib.ptr(d_c), _lib.ptr(d_u), ROWS, L, cfg, omc, T, 0, seed, None, step, row_off, None, None, 0.0, None, None,
                                                       f["top_k"], f["top_p"], f["typical_mass"], f["min_tokens"], _lib.ptr(tok), _lib.ptr(pre), _stream()))
        scores = torch.empty(ROWS, L, device=DEV)
        _lib.check(built_lib.paella_test_tail_scores(_lib.ptr(d_c), _lib.ptr(d_u), ROWS, L, cfg, omc, T, seed, step, row_off, _lib.ptr(scores), _stream()))
        torch.cuda.synchronize()
        want = _first_argmax(scores.cpu().numpy(), kept)
        assert np.array_equal(tok.cpu().numpy(), want) and torch.equal(tok, pre), "%s L=%d: tokens differ from the arg-max over the kept set at rows %s" % (
            name, L, np.nonzero(tok.cpu().numpy() != want)[0].tolist())
        if name == "top_k=1":
            top2 = np.sort(np.where(np.isnan(z), -np.inf, z), axis=1)[:, -2:]
            uniq = (top2[:, 1] > top2[:, 0]) & ~np.isnan(z).any(axis=1)
            assert uniq.sum() >= ROWS - 4 and np.array_equal(tok.cpu().numpy()[uniq], z.argmax(axis=1)[uniq]), "top_k = 1 is not the arg-max of z"


# ---------------------------------------------------------------------------------------------------------------- 1. + 2. request form
@pytest.mark.parametrize("L,with_u", SHAPES, ids=lambda v: str(v))
def test_kept_set_and_token_request_form(built_lib, L, with_u):
    rows, step = B_REQ * HW_REQ, 2
    seeds = _seeds([SEED_HI, 3, (1 << 64) - 2])
    temps, pairs = _f32(REQ_TEMPS), (_f32(REQ_PAIRS) if with_u else None)
    steps, never, active = _i32([step] * B_REQ), _f32([-1.0] * B_REQ), _i32([1] * B_REQ)  # (named: a pointer does not keep its tensor alive)
    for name in REQ_FILTERS:
        lc, lu, kept, fk, fm = request_case(L, name, with_u)
        d_c, d_u, d_fk, d_fm = _dev(lc), _dev(lu), _dev(fk), _dev(fm)
        keep = torch.full((rows, L), 9, dtype=torch.uint8, device=DEV)
        _lib.check(built_lib.paella_test_tail_filter_keep(_lib.ptr(d_c), _lib.ptr(d_u), rows, L, 1.0, 0.0, 1.0, 0, 1.0, 1.0, 1, _lib.ptr(pairs), _lib.ptr(temps),
                                                          _lib.ptr(seeds), HW_REQ, _lib.ptr(d_fk), _lib.ptr(d_fm), _lib.ptr(keep), None, _stream()))
        torch.cuda.synchronize()
        got = keep.cpu().numpy().astype(bool)
        bad = np.nonzero((got != kept).any(axis=1))[0]
        assert bad.size == 0, "%s L=%d: request-form kept set differs from the model on rows %s" % (name, L, bad.tolist())
        assert kept[HW_REQ:2 * HW_REQ].all()
        tok = torch.full((rows,), SENTINEL, dtype=torch.int64, device=DEV)
        pre = tok.clone()
        init = torch.zeros(rows, dtype=torch.int64, device=DEV)
        _lib.check(built_lib.paella_sample_tail_stream_filter(_lib.ptr(d_c), _lib.ptr(d_u), rows, L, _lib.ptr(pairs), _lib.ptr(temps), _lib.ptr(seeds), HW_REQ,
                                                              _lib.ptr(steps), _lib.ptr(never), _lib.ptr(active), _lib.ptr(init),
                                                              None, None, None, _lib.ptr(d_fk), _lib.ptr(d_fm), _lib.ptr(tok), _lib.ptr(pre), _stream()))
        scores = torch.empty(rows, L, device=DEV)
        _lib.check(built_lib.paella_test_tail_scores_req(_lib.ptr(d_c), _lib.ptr(d_u), rows, L, _lib.ptr(pairs), _lib.ptr(temps), _lib.ptr(seeds), HW_REQ, step,
                                                         _lib.ptr(scores), _stream()))
        torch.cuda.synchronize()
        want = _first_argmax(scores.cpu().numpy(), kept)
        assert np.array_equal(tok.cpu().numpy(), want) and torch.equal(tok, pre), "%s L=%d: request-form tokens differ at rows %s" % (
            name, L, np.nonzero(tok.cpu().numpy() != want)[0].tolist())


# ---------------------------------------------------------------------------------------------------------------- 3. off == plain
@pytest.mark.parametrize("L,with_u", SHAPES, ids=lambda v: str(v))
def test_filter_off_is_the_plain_tail_bit_for_bit(built_lib, L, with_u):
    lib, p = built_lib, _lib.ptr
    g = torch.Generator().manual_seed(L)
    new = lambda n: torch.full((n,), SENTINEL, dtype=torch.int64, device=DEV)
    # scalar form: renoise, pin, sampled_out, a device seed word and a row offset
    lc, lu, cfg, omc, T, _ = scalar_case(L, "typical", with_u)
    d_c, d_u = _dev(lc), _dev(lu)
    init, known, keep = (torch.randint(0, n, (ROWS,), generator=g).to(DEV) for n in (L, L, 2))
    sw = torch.tensor([12345], dtype=torch.int64, device=DEV)
    base, base_pre = new(ROWS), new(ROWS)
    _lib.check(lib.paella_sample_tail_pin(p(d_c), p(d_u), ROWS, L, cfg, omc, T, 0, SEED_HI, p(sw), 4, 7, None, p(init), 0.4, p(keep), p(known), p(base), p(base_pre), _stream()))
    for off in (OFF, dict(top_k=L, top_p=1.0, typical_mass=1.0, min_tokens=5), dict(top_k=L + 9, top_p=1.0, typical_mass=1.0, min_tokens=1)):
        got, got_pre = new(ROWS), new(ROWS)
        _lib.check(lib.paella_sample_tail_filter(p(d_c), p(d_u), ROWS, L, cfg, omc, T, 0, SEED_HI, p(sw), 4, 7, None, p(init), 0.4, p(keep), p(known), off["top_k"], off["top_p"],
                                                 off["typical_mass"], off["min_tokens"], p(got), p(got_pre), _stream()))
        torch.cuda.synchronize()
        assert torch.equal(got, base) and torch.equal(got_pre, base_pre), "scalar form, filter off %r: tokens differ from paella_sample_tail_pin" % (off,)
    assert bool((base != base_pre).any()), "the case renoises / pins nothing"
    # stream form: every request off, slot 1 inactive; then null tables; then request 1 filtering between two plain ones
    lc, lu, kept, fk, fm = request_case(L, "typical", with_u)
    rows = B_REQ * HW_REQ
    d_c, d_u = _dev(lc), _dev(lu)
    seeds, temps, pairs = _seeds([SEED_HI, 3, (1 << 64) - 2]), _f32(REQ_TEMPS), (_f32(REQ_PAIRS) if with_u else None)
    step, t_next, pin_on = _i32([3, 0, 7]), _f32([0.45, 0.9, -1.0]), _i32([1, 1, 0])
    init, known, keep = (torch.randint(0, n, (rows,), generator=g).to(DEV) for n in (L, L, 2))

    def tail(fn, active, tables, out, pre):
        act = _i32(active)
        args = [p(d_c), p(d_u), rows, L, p(pairs), p(temps), p(seeds), HW_REQ, p(step), p(t_next), p(act), p(init), p(keep), p(known), p(pin_on)]
        _lib.check(fn(*args, *(p(t) for t in tables), p(out), p(pre), _stream()))
        torch.cuda.synchronize()

    all_off = (_dev(np.int32([[0, 1]] * B_REQ)), _dev(np.float32([[1.0, 1.0]] * B_REQ)))
    for active in ([1, 0, 1], [1, 1, 1]):
        base, base_pre, got, got_pre, null, null_pre = (new(rows) for _ in range(6))
        tail(lib.paella_sample_tail_stream_pin, active, (), base, base_pre)
        tail(lib.paella_sample_tail_stream_filter, active, all_off, got, got_pre)
        tail(lib.paella_sample_tail_stream_filter, active, (None, None), null, null_pre)
        assert torch.equal(got, base) and torch.equal(got_pre, base_pre), "stream form, every request off: tokens differ from paella_sample_tail_stream_pin"
        assert torch.equal(null, base) and torch.equal(null_pre, base_pre), "stream form, null tables: not paella_sample_tail_stream_pin"
        if not active[1]:
            assert bool((got[HW_REQ:2 * HW_REQ] == SENTINEL).all()) and bool((got_pre[HW_REQ:2 * HW_REQ] == SENTINEL).all()), "an inactive slot's rows were written"
    # request 1 filters between two requests that do not
    mixed = (_dev(np.int32([[0, 1], [3, 1], [0, 1]])), _dev(np.float32([[1.0, 1.0], [1.0, 0.3], [1.0, 1.0]])))
    got, got_pre = new(rows), new(rows)
    tail(lib.paella_sample_tail_stream_filter, [1, 1, 1], mixed, got, got_pre)
    for b in (0, 2):
        sl = slice(b * HW_REQ, (b + 1) * HW_REQ)
        assert torch.equal(got[sl], base[sl]) and torch.equal(got_pre[sl], base_pre[sl]), "request %d does not filter, yet its tokens changed next to one that does" % b
    assert bool((got_pre[HW_REQ:2 * HW_REQ] != base_pre[HW_REQ:2 * HW_REQ]).any()), "request 1 (top_k = 3) drew the unfiltered tokens on all of its rows"


# ---------------------------------------------------------------------------------------------------------------- 4. distribution
def test_distribution_under_typical_filtering(built_lib):
    L, n, T = 64, 65536, 1.0
    rng = np.random.default_rng(2024)
    cand = rng.standard_normal((32, L)).astype(np.float32)
    idx, kept = _pick(cand, None, 1.0, 0.0, T, dict(typical_mass=0.5), 1)
    row, kept = cand[idx[0]], kept[0]
    dof = int(kept.sum()) - 1
    assert dof >= 4, "the fixed row keeps only %d labels" % (dof + 1)
    lc = torch.from_numpy(row).to(DEV)[None].expand(n, L).contiguous()
    tok = torch.empty(n, dtype=torch.int64, device=DEV)
    _lib.check(built_lib.paella_sample_tail_filter(_lib.ptr(lc), None, n, L, 1.0, 0.0, T, 0, 99, None, 0, 0, None, None, 0.0, None, None, 0, 1.0, 0.5, 1, _lib.ptr(tok), None,
                                                   _stream()))
    torch.cuda.synchronize()
    counts = np.bincount(tok.cpu().numpy(), minlength=L)
    assert counts[~kept].sum() == 0, "%d tokens fall outside the kept set" % counts[~kept].sum()
    p = np.exp(row.astype(np.float64) - row.max()) * kept
    p /= p.sum()
    chi2 = (((counts - n * p) ** 2)[kept] / (n * p[kept])).sum()
    from scipy.stats import chi2 as chi2_dist
    crit = float(chi2_dist.isf(1e-6, dof))
    print("typical_mass = 0.5 at L = 64: %d labels kept, chi-square %.2f over %d draws (critical value %.2f at 1e-6, %d degrees of freedom)" % (dof + 1, chi2, n, crit, dof))
    assert chi2 < crit


# ---------------------------------------------------------------------------------------------------------------- models
@pytest.fixture(scope="module")
def tiny(built_lib):
    m = paella_amd.Paella(**G.UNET_TINY)
    weights_for(m, sum(G.UNET_TINY["blocks"]))
    return m.to(DEV)


def _conds(B, seed=1):
    return to_dev(cond_for(G.UNET_TINY, B, 3, 0, seed), DEV), to_dev(cond_for(G.UNET_TINY, B, 3, 0, seed + 1), DEV)


KW = dict(steps=3, renoise_steps=2)


# ---------------------------------------------------------------------------------------------------------------- 5. four paths, one result
def test_sample_with_a_filter_through_four_paths(tiny):
    from paella_amd.dist import shard_inputs
    B, H, s = 2, 16, SEED_HI
    cs, us = _conds(B)
    kw = dict(cfg=4.0, device=DEV, noise="philox", seed=s, **KW)
    ref = paella_amd.sample(tiny, cs, (B, H, H), unconditional_inputs=us, typical_mass=0.2, **kw)
    plain = paella_amd.sample(tiny, cs, (B, H, H), unconditional_inputs=us, **kw)
    assert not torch.equal(ref, plain), "typical_mass = 0.2 changed no token"
    assert torch.equal(paella_amd.sample(tiny, cs, (B, H, H), unconditional_inputs=us, typical_mass=0.2, fused_tail=False, **kw), ref)
    assert torch.equal(paella_amd.sample(tiny, cs, (B, H, H), unconditional_inputs=us, top_k=0, top_p=1.0, typical_mass=1.0, min_tokens=3, **kw), plain), "off values changed tokens"
    gs = paella_amd.GraphSampler(tiny, cs, us, (B, H, H), cfg=4.0, device=DEV, typical_mass=0.2, **KW)
    assert torch.equal(gs(seed=s), ref), "GraphSampler differs from the eager call"
    # two shards against the unsharded call
    parts = [paella_amd.sample(tiny, shard_inputs(cs, lo, lo + 1), (1, H, H), unconditional_inputs=shard_inputs(us, lo, lo + 1), typical_mass=0.2, shard=(lo, B), **kw)
             for lo in range(B)]
    assert torch.equal(torch.cat(parts), ref), "the two shards differ from the unsharded call"
    # a request batch with that one setting against a batch-of-one sample
    c1, u1 = shard_inputs(cs, 0, 1), shard_inputs(us, 0, 1)
    one = paella_amd.sample(tiny, c1, (1, H, H), unconditional_inputs=u1, typical_mass=0.2, **kw)
    assert torch.equal(paella_amd.sample_requests(tiny, c1, u1, (1, H, H), [s], cfg=4.0, device=DEV, typical_mass=0.2, **KW), one)
    gr = paella_amd.GraphRequestSampler(tiny, c1, u1, (1, H, H), cfg=4.0, device=DEV, filtering=True, **KW)
    assert torch.equal(gr([s], typical_mass=0.2), one), "GraphRequestSampler(filtering=True) differs from the batch-of-one sample"
    assert torch.equal(gr([s]), paella_amd.sample(tiny, c1, (1, H, H), unconditional_inputs=u1, **kw)), "a replay with every filter off is not the plain call"
    assert torch.equal(gr([s], top_k=[5], top_p=0.7, min_tokens=2), paella_amd.sample(tiny, c1, (1, H, H), unconditional_inputs=u1, top_k=5, top_p=0.7, min_tokens=2, **kw))
    assert gr.captures == 1
    with pytest.raises(ValueError, match="filtering=True"):
        paella_amd.GraphRequestSampler(tiny, c1, u1, (1, H, H), cfg=4.0, device=DEV, **KW)([s], top_k=3)


# ---------------------------------------------------------------------------------------------------------------- 6. closed loop against a host composition
def test_closed_loop_against_the_model_and_the_score_hook(tiny):
    """every step: the logits of forward_prepared (guidance folded through the head), the model's kept set of every row -- whose bands are asserted empty -- and
    the first arg-max of the hook's scores over it, renoised with the model of the counter-based mask, give the tokens of the step; the last step's are sample()'s"""
    B, H, s, cfg = 2, 8, 4242, 4.0
    L, rows = G.UNET_TINY["num_labels"], B * H * H
    cs, us = _conds(B, 5)
    filt = dict(typical_mass=0.2)
    steps, renoise_steps = KW["steps"], KW["renoise_steps"]
    t_list = sampling.linspace_schedule(1.0, 0.0, steps + 1)
    temps = sampling.linspace_schedule(1.0, 0.2, steps)
    pair = (float(torch.tensor(cfg, dtype=torch.float32)), float(torch.tensor(1.0 - cfg, dtype=torch.float32)))
    cache = tiny.prepare_cond(**{k: (torch.cat([cs[k], us[k]]) if cs[k] is not None else None) for k in cs})
    init = sampling.start_tokens(L, (B, H, H), s, DEV)
    x = init.clone()
    lib = _lib.load()
    for i in range(steps):
        renoise = i < renoise_steps
        logits = tiny._forward_prepared_raw(x, torch.full((B,), t_list[i], device=DEV), cache, cfg_mix=pair).reshape(rows, L).contiguous()
        kept, band = TM.truncate_rows(TM.z_of(logits.cpu().numpy(), None, 1.0, 0.0, temps[i]), **filt)
        assert not band.any(), "step %d: %d rows have a non-empty band (choose another seed)" % (i, int(band.any(axis=1).sum()))
        scores = torch.empty(rows, L, device=DEV)
        _lib.check(lib.paella_test_tail_scores(_lib.ptr(logits), None, rows, L, 1.0, 0.0, temps[i], s, i, 0, _lib.ptr(scores), _stream()))
        dev_tok = torch.empty(B, H, H, dtype=torch.int64, device=DEV)
        sampling._tail(logits, None, rows, L, 1.0, 0.0, temps[i], 0, None, s, i, init if renoise else None, None, t_list[i + 1] if renoise else 0.0, dev_tok,
                       filt=sampling.check_filter(**filt))
        torch.cuda.synchronize()
        want = _first_argmax(scores.cpu().numpy(), kept)
        if renoise:
            want = np.where(C.renoise_mask(s, rows, i, t_list[i + 1]), init.cpu().numpy().reshape(-1), want)
        assert np.array_equal(dev_tok.cpu().numpy().reshape(-1), want), "step %d: %d tokens differ from the host composition" % (i, int((dev_tok.cpu().numpy().reshape(-1) != want).sum()))
        assert kept.sum(axis=1).min() >= 1 and kept.sum(axis=1).mean() < L / 2
        x = dev_tok
    got = paella_amd.sample(tiny, cs, (B, H, H), unconditional_inputs=us, cfg=cfg, device=DEV, noise="philox", seed=s, **filt, **KW)
    assert torch.equal(got, x), "sample() differs from the step-by-step composition"


# ---------------------------------------------------------------------------------------------------------------- 7. request stream
def _one(seed):
    return to_dev(cond_for(G.UNET_TINY, 1, 3, 0, seed), DEV), to_dev(cond_for(G.UNET_TINY, 1, 3, 0, seed + 100), DEV)


def _request(cseed, **kw):
    c, u = _one(cseed)
    return dict(model_inputs=c, unconditional_inputs=u, **kw)


def _hold_two(st):
    """slots 0 and 1 taken by finished, uncollected one-step requests: the next request lands in slot 2 and runs with no running batch-mate"""
    for k in range(2):
        st.admit(**_request(60 + k, seed=k, steps=1))
    assert st.tick() == [0, 1] and st.free_slots == [2, 3]


def _until(st, slot):
    for _ in range(16):
        for b in st.tick():
            res = st.result(b)
            if b == slot:
                return res
    raise AssertionError("the request of slot %d did not finish" % slot)


def test_request_stream_with_filters(tiny):
    """32x32 tokens (no 16-row block straddles two samples: the condition of the stream's bit-for-bit contract).  "The one-slot stream" is the stream of
    the same shape serving the request alone in the same slot: the logits of another batch size differ in their last bits, as for every request of a stream."""
    H, B = 32, 4
    ex_c, ex_u = _one(1)
    new = lambda **kw: paella_amd.RequestStream(tiny, ex_c, ex_u, (B, H, H), max_steps=6, device=DEV, **kw)
    X = _request(50, seed=SEED_HI, cfg=(9.0, 5.0), steps=4, temperature=(0.9, 0.3), typical_mass=0.2)
    Y = _request(51, seed=77, cfg=3.0, steps=3)                                    # no filter
    # alone in slot 2
    alone = new(filtering=True)
    _hold_two(alone)
    assert alone.admit(**X) == 2
    tok_alone = _until(alone, 2)
    # run A: admitted at tick 0 next to an unfiltered, a top-k and a typical request
    a = new(filtering=True)
    a.admit(**_request(2, seed=1, steps=3))
    a.admit(**_request(3, seed=2, steps=4, cfg=3.0, top_k=5))
    assert a.admit(**X) == 2
    a.admit(**_request(4, seed=3, steps=6, temperature=(0.7, 0.7), typical_mass=0.6, min_tokens=2))
    tok_a = _until(a, 2)
    # run B: admitted at tick 3 into a stream with other requests mid-flight; slot 2 held a top-p request before (its row must not be inherited)
    b = new(filtering=True)
    b.admit(**_request(7, seed=11, steps=6, cfg=(2.0, 6.0), top_p=0.5))
    b.admit(**_request(8, seed=12, steps=5, temperature=(1.2, 0.4)))
    assert b.admit(**_request(9, seed=13, steps=2, top_k=1)) == 2
    for tick in range(3):
        for s_ in b.tick():
            b.result(s_)
    assert 2 in b.free_slots
    assert b.admit(**X) == 2
    tok_b = _until(b, 2)
    assert torch.equal(tok_a, tok_alone) and torch.equal(tok_b, tok_alone), "a filtered request depends on its batch-mates or its admission tick (%d / %d tokens differ)" % (
        int((tok_a != tok_alone).sum()), int((tok_b != tok_alone).sum()))
    # the filter does something, and a request with filters off is the request of a filtering=False stream; slot 2 is reused after the filtered X
    plain = new()
    _hold_two(plain)
    assert plain.admit(**Y) == 2
    tok_plain = _until(plain, 2)
    for _ in range(8):
        for s_ in b.tick():
            b.result(s_)
    assert not b.active and b.free_slots == [0, 1, 2, 3]
    _hold_two(b)
    assert b.admit(**Y) == 2
    tok_reused = _until(b, 2)
    assert torch.equal(tok_reused, tok_plain), "an unfiltered request in a slot a filtered one left differs from the filtering=False stream at %d tokens" % int((tok_reused != tok_plain).sum())
    Xoff = dict(X, typical_mass=None)
    plain.reset()
    _hold_two(plain)
    assert plain.admit(**Xoff) == 2
    assert not torch.equal(_until(plain, 2), tok_alone), "typical_mass = 0.2 changed no token of the request"
    # reset writes "off" everywhere
    b.reset()
    assert b.filter_k.cpu().tolist() == [[0, 1]] * B and bool((b.filter_mass == 1.0).all())
    torch.cuda.synchronize()
    assert a.captures == 1 and b.captures == 1 and alone.captures == 1 and plain.captures == 1
    with pytest.raises(ValueError, match="filtering=True"):
        plain.admit(**X)


def test_request_stream_filter_composes_with_editing(tiny):
    H, B, L = 16, 2, G.UNET_TINY["num_labels"]
    ex_c, ex_u = _one(1)
    st = paella_amd.RequestStream(tiny, ex_c, ex_u, (B, H, H), max_steps=4, device=DEV, filtering=True, editing=True)
    g = torch.Generator().manual_seed(8)
    known = torch.randint(0, L, (H, H), generator=g).to(DEV)
    mask = torch.randint(0, 2, (H, H), generator=g).to(DEV)
    st.admit(**_request(5, seed=9, steps=3, typical_mass=0.3))
    assert st.admit(**_request(6, seed=10, steps=4, known=known, mask=mask, pin="step", top_k=4, top_p=0.8)) == 1
    tok = _until(st, 1)
    assert torch.equal(tok[mask == 0], known[mask == 0]), "the known tokens of a filtered editing request did not stay pinned"
    assert 0 < int((mask == 0).sum()) < H * H and st.captures == 1
    # the same editing request through an unfiltered editing stream draws other tokens somewhere in the regenerated region
    ref = paella_amd.RequestStream(tiny, ex_c, ex_u, (B, H, H), max_steps=4, device=DEV, editing=True)
    ref.admit(**_request(5, seed=9, steps=3))
    ref.admit(**_request(6, seed=10, steps=4, known=known, mask=mask, pin="step"))
    assert not torch.equal(_until(ref, 1), tok)
