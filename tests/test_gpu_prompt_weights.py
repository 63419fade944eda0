"""GPU: per-request prompt weights -- the per-sample key-weight table of the attention kernels (kw_table / kw_len / kw_pitch next to the shared key_weights
vector), the three _kw forward entry points, `KeyWeights`, and `attn_weights` per request in `sample_requests`, `GraphRequestSampler` and `RequestStream`.

The kernel contract (include/paella_hip.h, "Per-request prompt weights"): (1) sample b of a table launch equals, bit for bit, the same kernel launched for that
sample alone with the shared vector = row b (NULL when its count is 0); (2) entries beyond a row's count are never read (they hold NaN here); (3) without the
count table every launch is the launch it was."""
import numpy as np
import pytest
import torch

import paella_amd
from oracle import golden_configs as G
from oracle import paella_oracle as O
from paella_amd import KeyWeights, _lib, sampling
from paella_amd.modules import CondCache
from tests.helpers import cond_for, to_dev, weights_for

pytestmark = pytest.mark.gpu
DEV = "cuda"

NHEAD, S_SLOT = 4, 40
COND_LEN = [40, 4, 16, 17, 32, 33]
WANT = [0, 4, 1, 17, 33, 10 ** 6]      # none, a few, one, a straddled 16-key tile, a straddled 32-key stage, every key
PITCH = 320                             # >= 256 self keys + 40 conditioning keys


def _stream():
    return _lib.stream_ptr(torch.device(DEV))


def _variants(Lq):
    """the dispatch variants paella_test_attention_variant can force at this query count (attention.hip: launch_attention)"""
    if Lq < 64:
        return [0]
    if Lq < 256:
        return [0, 20, 21, 22]
    return [0, 10, 11, 22]


def _attn_inputs(D, Lq, Lself, seed):
    B, ld = len(COND_LEN), NHEAD * D
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B * Lq, ld, generator=g).to(DEV)
    ks = torch.randn(B * max(Lself, 1), ld, generator=g).to(DEV)
    vs = torch.randn(B * max(Lself, 1), ld, generator=g).to(DEV)
    kc = torch.randn(B, S_SLOT, ld, generator=g)
    vc = torch.randn(B, S_SLOT, ld, generator=g)
    counts = [min(w, Lself + n) for w, n in zip(WANT, COND_LEN)]
    table = torch.rand(B, PITCH, generator=g) + 0.5
    table[3, 2], table[4, 20] = 0.0, 1.0          # one exact 0 and one exact 1 among the weights that are used
    for b, n in enumerate(COND_LEN):              # never read: the padding rows of every slot and the table entries beyond every count
        kc[b, n:] = float("nan")
        vc[b, n:] = float("nan")
        table[b, counts[b]:] = float("nan")
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    return q, ks, vs, kc.to(DEV), vc.to(DEV), table.to(DEV), counts, i32(counts), i32(COND_LEN)


@pytest.mark.parametrize("Lq,Lself", [(16, 16), (64, 64), (64, 0), (256, 256)])
@pytest.mark.parametrize("D", [16, 64, 80])
def test_attention_kw_is_bit_identical_to_each_sample_alone(built_lib, D, Lq, Lself):
    lib = built_lib
    B, ld = len(COND_LEN), NHEAD * D
    q, ks, vs, kc, vc, table, counts, counts_d, lens_d = _attn_inputs(D, Lq, Lself, 100 * D + Lq + Lself)
    ksp, vsp = (_lib.ptr(ks), _lib.ptr(vs)) if Lself else (None, None)
    n_same = min(4, Lself + min(COND_LEN))
    same = table[1, :n_same].contiguous()
    same_table = torch.full((B, PITCH), float("nan"), device=DEV)
    same_table[:, :n_same] = same
    same_counts = torch.full((B,), n_same, dtype=torch.int32, device=DEV)
    try:
        for variant in _variants(Lq):
            lib.paella_test_attention_variant(variant)
            out = torch.full((B * Lq, ld), float("nan"), device=DEV)
            _lib.check(lib.paella_op_attention_kw(_lib.ptr(q), ksp, vsp, _lib.ptr(kc), _lib.ptr(vc), _lib.ptr(out), B, NHEAD, D, Lq, Lself, S_SLOT, _lib.ptr(lens_d),
                                                  _lib.ptr(table), _lib.ptr(counts_d), PITCH, _stream()))
            torch.cuda.synchronize()
            assert torch.isfinite(out).all(), "variant %d: a NaN (padding row, or a table entry beyond its count) was read" % variant
            for b, n in enumerate(COND_LEN):
                qb = q[b * Lq:(b + 1) * Lq].contiguous()
                ksb, vsb = ks[b * Lself:(b + 1) * Lself].contiguous(), vs[b * Lself:(b + 1) * Lself].contiguous()
                kcb, vcb = kc[b, :n].contiguous(), vc[b, :n].contiguous()
                wb = table[b, :counts[b]].contiguous() if counts[b] else None
                ref = torch.empty(Lq, ld, device=DEV)
                _lib.check(lib.paella_op_attention(_lib.ptr(qb), _lib.ptr(ksb) if Lself else None, _lib.ptr(vsb) if Lself else None, _lib.ptr(kcb), _lib.ptr(vcb),
                                                   _lib.ptr(ref), 1, NHEAD, D, Lq, Lself, n, _lib.ptr(wb), counts[b], _stream()))
                torch.cuda.synchronize()
                got = out[b * Lq:(b + 1) * Lq]
                assert torch.equal(got, ref), "variant %d, sample %d (%d conditioning keys, %d weights): %d values differ" % (variant, b, n, counts[b], int((got != ref).sum()))
            # every row the same vector == the shared vector of the ragged entry point
            a, r = torch.empty(B * Lq, ld, device=DEV), torch.empty(B * Lq, ld, device=DEV)
            _lib.check(lib.paella_op_attention_kw(_lib.ptr(q), ksp, vsp, _lib.ptr(kc), _lib.ptr(vc), _lib.ptr(a), B, NHEAD, D, Lq, Lself, S_SLOT, _lib.ptr(lens_d),
                                                  _lib.ptr(same_table), _lib.ptr(same_counts), PITCH, _stream()))
            _lib.check(lib.paella_op_attention_ragged(_lib.ptr(q), ksp, vsp, _lib.ptr(kc), _lib.ptr(vc), _lib.ptr(r), B, NHEAD, D, Lq, Lself, S_SLOT, _lib.ptr(lens_d),
                                                      _lib.ptr(same), n_same, _stream()))
            torch.cuda.synchronize()
            assert torch.equal(a, r), "variant %d: a table of equal rows differs from the shared vector at %d values" % (variant, int((a != r).sum()))
    finally:
        lib.paella_test_attention_variant(0)


@pytest.mark.parametrize("D", [64, 80])
def test_attention_bf16_kw_is_bit_identical_to_each_sample_alone(built_lib, D):
    lib, Lq, Lself = built_lib, 256, 256
    B, ld = len(COND_LEN), NHEAD * D
    bits = lambda t: t.to(torch.bfloat16).contiguous().view(torch.int16)
    q, ks, vs, kc, vc, table, counts, counts_d, lens_d = _attn_inputs(D, Lq, Lself, 7 * D)
    q16, ks16, vs16 = bits(q), bits(ks), bits(vs)
    out = torch.full((B * Lq, ld), -1, dtype=torch.int16, device=DEV)
    _lib.check(lib.paella_test_attention_bf16_kw(_lib.ptr(q16), _lib.ptr(ks16), _lib.ptr(vs16), _lib.ptr(kc), _lib.ptr(vc), _lib.ptr(out), B, NHEAD, D, Lq, Lself, S_SLOT,
                                                 _lib.ptr(lens_d), _lib.ptr(table), _lib.ptr(counts_d), PITCH, _stream()))
    torch.cuda.synchronize()
    assert torch.isfinite(out.view(torch.bfloat16).float()).all(), "a NaN (padding row, or a table entry beyond its count) was read"
    for b, n in enumerate(COND_LEN):
        sl = slice(b * Lq, (b + 1) * Lq)
        kcb, vcb = kc[b, :n].contiguous(), vc[b, :n].contiguous()
        wb = table[b, :counts[b]].contiguous() if counts[b] else None
        ref = torch.empty(Lq, ld, dtype=torch.int16, device=DEV)
        _lib.check(lib.paella_test_attention_bf16(_lib.ptr(q16[sl].contiguous()), _lib.ptr(ks16[sl].contiguous()), _lib.ptr(vs16[sl].contiguous()), _lib.ptr(kcb),
                                                  _lib.ptr(vcb), _lib.ptr(ref), 1, NHEAD, D, Lq, Lself, n, _lib.ptr(wb), counts[b], _stream()))
        torch.cuda.synchronize()
        assert torch.equal(out[sl], ref), "bf16 sample %d (%d conditioning keys, %d weights): %d values differ" % (b, n, counts[b], int((out[sl] != ref).sum()))
    # every row the same vector == the shared vector of the ragged hook
    same = table[1, :4].contiguous()
    same_table = torch.full((B, PITCH), float("nan"), device=DEV)
    same_table[:, :4] = same
    same_counts = torch.full((B,), 4, dtype=torch.int32, device=DEV)
    a, r = (torch.full((B * Lq, ld), -1, dtype=torch.int16, device=DEV) for _ in range(2))
    _lib.check(lib.paella_test_attention_bf16_kw(_lib.ptr(q16), _lib.ptr(ks16), _lib.ptr(vs16), _lib.ptr(kc), _lib.ptr(vc), _lib.ptr(a), B, NHEAD, D, Lq, Lself, S_SLOT,
                                                 _lib.ptr(lens_d), _lib.ptr(same_table), _lib.ptr(same_counts), PITCH, _stream()))
    _lib.check(lib.paella_test_attention_bf16_ragged(_lib.ptr(q16), _lib.ptr(ks16), _lib.ptr(vs16), _lib.ptr(kc), _lib.ptr(vc), _lib.ptr(r), B, NHEAD, D, Lq, Lself,
                                                     S_SLOT, _lib.ptr(lens_d), _lib.ptr(same), 4, _stream()))
    torch.cuda.synchronize()
    assert torch.equal(a, r), "bf16: a table of equal rows differs from the shared vector at %d values" % int((a != r).sum())


def test_attention_kw_argument_errors(built_lib):
    lib = built_lib
    q, o = torch.zeros(16, 64, device=DEV), torch.empty(16, 64, device=DEV)
    t, n = torch.ones(1, 4, device=DEV), torch.ones(1, dtype=torch.int32, device=DEV)
    args = lambda tab, cnt, pitch: (_lib.ptr(q), _lib.ptr(q), _lib.ptr(q), _lib.ptr(q), _lib.ptr(q), _lib.ptr(o), 1, 4, 16, 16, 16, 16, None, tab, cnt, pitch, _stream())
    assert lib.paella_op_attention_kw(*args(None, _lib.ptr(n), 4)) == -1 and b"kw_table" in lib.paella_last_error()
    assert lib.paella_op_attention_kw(*args(_lib.ptr(t), _lib.ptr(n), 0)) == -1
    assert lib.paella_op_attention_kw(*args(_lib.ptr(t), None, 4)) == 0          # no count table: the table is ignored
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- models
def _model(cfg):
    m = paella_amd.Paella(**cfg)
    sd = weights_for(m, sum(cfg["blocks"]))
    return m.to(DEV), sd


@pytest.fixture(scope="module")
def tiny(built_lib):
    return _model(G.UNET_TINY)


def _table(rows, pitch, nan=False):
    """a KeyWeights with these rows (None = count 0); nan: the entries no count covers hold NaN"""
    kw = KeyWeights(len(rows), pitch, DEV)
    if nan:
        kw.buf.fill_(float("nan"))
    for b, w in enumerate(rows):
        kw.set(b, w)
    return kw


def test_table_forward_against_the_reference_fixture(golden, tiny):
    """tests/golden/unet_tiny_attnw.npz: the reference's weighted and unweighted logits of one B = 2 batch -- a table that weighs one sample only must give that
    sample's weighted logits and the other's unweighted ones (the tolerance tests/test_gpu_unet.py applies to this fixture)"""
    m, _ = tiny
    g = golden("unet_tiny_attnw")
    x, r = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["r"]).to(DEV)
    cache = m.prepare_cond(**to_dev(cond_for(G.UNET_TINY, 2, 5, 2, G.COND_SEED), DEV))
    w = torch.from_numpy(g["attn_weights"]).to(DEV)
    for rows, want in (([w, None], (g["logits"][0], g["logits_noaw"][1])), ([None, w], (g["logits_noaw"][0], g["logits"][1]))):
        got = m.forward_prepared(x, r, cache, attn_weights=_table(rows, 8, nan=True)).cpu().numpy()
        for b in range(2):
            d = float(np.abs(got[b] - want[b]).max())
            print("attnw fixture, rows %s, sample %d: max |diff| %.3e" % (["w" if v is not None else "-" for v in rows], b, d))
            np.testing.assert_allclose(got[b], want[b], atol=2e-5, rtol=0)
    assert float(np.abs(g["logits"] - g["logits_noaw"]).max()) > 1e-3     # the two references really differ


def _unequal(cfg, B=2):
    """13 conditioning rows (5 ByT5 + clip + one clip_image) against 6 (2 ByT5 + clip)"""
    return cond_for(cfg, B, 5, 1, G.COND_SEED), cond_for(cfg, B, 2, 0, G.COND_SEED + 5)


def _one_sample(inputs, b):
    return {k: (None if v is None else [t[b:b + 1] for t in v] if isinstance(v, (list, tuple)) else v[b:b + 1]) for k, v in inputs.items()}


# the convex mix of tests/test_gpu_ragged_conditioning.py: the per-forward tolerance holds for the mixed logits with no new number; and post-softmax multipliers
# in [0.25, 1] only shrink every attention output together with its error, so the tolerances of the unweighted test carry over
MIX = (0.625, 0.375)


@pytest.mark.parametrize("cfg_name,grid,atol", [("UNET_TINY", 32, 2e-5), ("UNET_MID", 16, 3e-4)])
def test_guided_ragged_forward_one_vector_per_slot_against_oracle(built_lib, cfg_name, grid, atol):
    cfg = getattr(G, cfg_name)
    m, sd = _model(cfg)
    B, L = 2, cfg["num_labels"]
    c, u = _unequal(cfg, B)
    cd, ud = to_dev(c, DEV), to_dev(u, DEV)
    g = torch.Generator().manual_seed(3)
    x = torch.randint(0, L, (B, grid, grid), generator=g)
    r = torch.tensor([0.7, 0.3])
    wt = lambda n: torch.rand(n, generator=g) * 0.75 + 0.25
    rows = [wt(4), None, wt(6), wt(3)]             # slots: conditional 0, 1, unconditional 0, 1; wt(6) is as long as the unconditional side's 6 rows
    with torch.no_grad():
        ref = torch.cat([O.unet_forward(sd, cfg, x[b:b + 1], r[b:b + 1], **_one_sample(c, b), attn_weights=rows[b]).float() * MIX[0] +
                         O.unet_forward(sd, cfg, x[b:b + 1], r[b:b + 1], **_one_sample(u, b), attn_weights=rows[B + b]).float() * MIX[1] for b in range(B)])
    cache = sampling._prepare_ragged_pair(m, cd, ud, B, None)
    assert cache.lens.tolist() == [13, 13, 6, 6]
    dev_rows = [None if w is None else w.to(DEV) for w in rows]
    got = m.forward_prepared(x.to(DEV), r.to(DEV), cache, attn_weights=_table(dev_rows, 8), cfg_mix=MIX)
    diff = float((got.cpu() - ref).abs().max())
    print("%s guided ragged forward, one weight vector per slot, mixed logits vs oracle: max |diff| %.3e (bound %.0e)" % (cfg_name, diff, atol))
    assert diff <= atol
    got_nan = m.forward_prepared(x.to(DEV), r.to(DEV), cache, attn_weights=_table(dev_rows, 8, nan=True), cfg_mix=MIX)
    assert torch.equal(got, got_nan), "NaN in the unused table entries changed %d logits" % int((got != got_nan).sum())
    unweighted = m.forward_prepared(x.to(DEV), r.to(DEV), cache, cfg_mix=MIX)
    assert float((got - unweighted).abs().max()) > atol, "the weights did not act"


def test_fused_table_step_equals_unfused(tiny):
    """forward_sample on forward_sample_req_kw == forward_shared_req_kw + paella_sample_tail_req on the same seeds"""
    m, _ = tiny
    cfg, B, H = G.UNET_TINY, 2, 16
    L, hw = cfg["num_labels"], H * H
    cs, us = to_dev(cond_for(cfg, B, 3, 0, 1), DEV), to_dev(cond_for(cfg, B, 3, 0, 2), DEV)
    cache = m.prepare_cond(**{k: (torch.cat([cs[k], us[k]]) if cs[k] is not None else None) for k in cs})
    req = sampling.RequestTables(sampling.request_tables(B, 3, [11, (1 << 64) - 2], [3.0, (9.0, 5.0)], [(1.0, 0.2), (0.7, 0.3)]), DEV)
    g = torch.Generator().manual_seed(9)
    x = torch.randint(0, L, (B, H, H), generator=g).to(DEV)
    init = torch.randint(0, L, (B, H, H), generator=g).to(DEV)
    r = torch.full((B,), 0.6, device=DEV)
    kw = _table([(torch.rand(5, generator=g) + 0.5).to(DEV), None, None, (torch.rand(2, generator=g) + 0.5).to(DEV)], 8, nan=True)
    fused, unfused, plain = (torch.empty(B, H, H, dtype=torch.int64, device=DEV) for _ in range(3))
    for step, renoise in [(0, False), (2, True)]:
        t_next = 0.55 if renoise else 0.0
        m.forward_sample(x, r, cache, fused, temperature=1.0, offset=step, init_noise=init if renoise else None, t_next=t_next, req=req.step(step), attn_weights=kw)
        lg = m._forward_prepared_raw(x, r, cache, req_mix=req.pairs[step], attn_weights=kw).reshape(B * hw, L)
        _lib.check(_lib.load().paella_sample_tail_req(_lib.ptr(lg), None, B * hw, L, None, _lib.ptr(req.temps[step]), _lib.ptr(req.seeds), hw, step,
                                                      _lib.ptr(init if renoise else None), t_next, _lib.ptr(unfused), None, _stream()))
        torch.cuda.synchronize()
        assert torch.equal(fused, unfused), "step %d: the fused table step differs from forward_shared_req_kw + request tail at %d positions" % (step, int((fused != unfused).sum()))
        m.forward_sample(x, r, cache, plain, temperature=1.0, offset=step, init_noise=init if renoise else None, t_next=t_next, req=req.step(step))
        assert not torch.equal(fused, plain), "the weights did not act"
    with pytest.raises(ValueError, match="attn_weights"):
        m.forward_sample(x, r, cache, fused, temperature=1.0, cfg_mix=(8.0, -7.0), attn_weights=kw)           # the scalar form takes one vector
    with pytest.raises(ValueError, match="attn_weights"):
        m.forward_prepared(x, r, cache, attn_weights=_table([None] * 3, 8))                                   # one row per conditioning slot


# ---------------------------------------------------------------------------------------------------------------- sample_requests / GraphRequestSampler
def test_sample_requests_weights_per_request(tiny):
    m, _ = tiny
    cfg, B, H = G.UNET_TINY, 3, 16
    cs, us = to_dev(cond_for(cfg, B, 3, 0, 1), DEV), to_dev(cond_for(cfg, B, 3, 0, 2), DEV)
    g = torch.Generator().manual_seed(4)
    wt = lambda n: (torch.rand(n, generator=g) * 1.5 + 0.25).to(DEV)
    w0, w2c, o1, o2 = wt(4), wt(7), wt(3), wt(5)
    kw = dict(seeds=[0xF00DFACE00C0FFEE, 5, 77], cfg=[3.0, 8.0, (9.0, 5.0)], temperature=[(1.0, 0.3), (0.8, 0.2), (0.6, 0.6)], steps=3, renoise_steps=2, device=DEV)
    run = lambda aw: paella_amd.sample_requests(m, cs, us, (B, H, H), attn_weights=aw, **kw)
    mixed = [w0, None, (w2c, None)]
    got = run(mixed)
    assert int(got.min()) >= 0 and int(got.max()) < cfg["num_labels"]
    everyone = [run(w0), run(None), run([(w2c, None)] * B)]          # every request with request b's weights: the shared vector where the form allows
    for b in range(B):
        assert torch.equal(got[b], everyone[b][b]), "request %d: %d tokens differ from the call in which everyone carries its weights" % (b, int((got[b] != everyone[b][b]).sum()))
    assert not torch.equal(everyone[0][0], everyone[1][0]), "the weights did not act"
    for b, mates in enumerate(([w0, (o1, o2), o2], [(None, o1), None, o2], [o1, (o2, o1), (w2c, None)])):
        other = run(mates)
        assert torch.equal(other[b], got[b]), "request %d: its tokens depend on its batch-mates' weights (%d positions)" % (b, int((other[b] != got[b]).sum()))
    # captured: the table is rewritten in place
    gr = paella_amd.GraphRequestSampler(m, cs, us, (B, H, H), steps=3, renoise_steps=2, device=DEV, max_attn_weights=8)
    call = {k: kw[k] for k in ("seeds", "cfg", "temperature")}
    for aw in (mixed, None, w0, [(None, o1), None, o2]):
        out = gr(attn_weights=aw, **call).clone()
        eager = run(aw)
        assert torch.equal(out, eager), "graph replay differs from the eager call at %d positions" % int((out != eager).sum())
    assert gr.captures == 1
    with pytest.raises(ValueError, match="attn_weights"):
        gr(attn_weights=[wt(9), None, None], **call)                  # longer than the table's rows
    with pytest.raises(ValueError, match="attn_weights"):
        run([wt(12), None, None])                                     # 4 self keys + 7 rows = 11 keys at the smallest attention level
    with pytest.raises(ValueError, match="max_attn_weights"):
        paella_amd.GraphRequestSampler(m, cs, us, (B, H, H), steps=3, renoise_steps=2, device=DEV).__call__(attn_weights=w0, **call)


# ---------------------------------------------------------------------------------------------------------------- request stream
STREAM_SHAPE, STEPS = (3, 32, 32), 3


def _request(cfg, n_byt5, n_img, seed, **over):
    """one request: n_byt5 ByT5 rows + clip (+ a CLIP image) against an unconditional side of 1 ByT5 row + clip"""
    return dict(dict(model_inputs=to_dev(cond_for(cfg, 1, n_byt5, n_img, seed), DEV), unconditional_inputs=to_dev(cond_for(cfg, 1, 1, 0, seed + 100), DEV),
                     seed=1000 + seed, steps=STEPS, cfg=6.0), **over)


def _serve(st, before, req, pre_ticks):
    """admit `before` (they take the first slots), tick pre_ticks times, then admit `req` (the next slot) and run it to the end: its slot and tokens"""
    st.reset()
    for q in before:
        st.admit(**q)
    for _ in range(pre_ticks):
        st.tick()
    slot = st.admit(**req)
    assert slot == len(before)
    for _ in range(STEPS + 1):
        if slot in st.tick():
            break
    return st.result(slot)


def test_request_stream_weights_per_request(tiny):
    m, _ = tiny
    cfg = G.UNET_TINY
    g = torch.Generator().manual_seed(8)
    wt = lambda n: (torch.rand(n, generator=g) * 1.5 + 0.25).to(DEV)
    w0, w1c, w1u = wt(4), wt(8), wt(2)
    reqs = [_request(cfg, 3, 0, 1, attn_weights=w0), _request(cfg, 7, 1, 2, attn_weights=(w1c, w1u)), _request(cfg, 1, 0, 3, attn_weights=None)]
    mk = lambda **k: paella_amd.RequestStream(m, reqs[0]["model_inputs"], reqs[0]["unconditional_inputs"], STREAM_SHAPE, max_steps=4, device=DEV, max_cond_rows=16, **k)
    st = mk(max_attn_weights=8)
    assert st.key_weights.buf.shape == (6, 8) and st.key_weights.lens.tolist() == [0] * 6
    idle = lambda i, **k: dict(_request(cfg, 2 + i, 0, 50 + i, **k), steps=1)       # finishes with the first tick and keeps its slot: an idle mate
    alone = []
    for i, q in enumerate(reqs):
        others = [reqs[j] for j in range(3) if j != i]
        a = _serve(st, [idle(0), idle(1, attn_weights=wt(5))], q, 1)                # (a) slot 2, nobody else running
        lens = st.key_weights.lens.tolist()
        assert (lens[2], lens[5]) == ((4, 4), (8, 2), (0, 0))[i] and lens[1] == lens[4] == 5
        b = _serve(st, others, q, 0)                                                # two running mates with other weights, joined together
        d = _serve(st, [dict(o, steps=4, attn_weights=(None, wt(3))) for o in others], q, 2)     # joins two ticks after its mates, whose weights changed
        assert torch.equal(a, b), "request %d: tokens depend on its batch-mates (%d positions)" % (i, int((a != b).sum()))
        assert torch.equal(a, d), "request %d: tokens depend on the tick it joined at or its mates' weights (%d positions)" % (i, int((a != d).sum()))
        alone.append(a)
    # (c) slot 2 reused, WITHOUT a reset, by an unweighted request right after a weighted one == a stream that never saw a weight
    a = _serve(st, [idle(0), idle(1)], reqs[1], 1)
    assert torch.equal(a, alone[1]) and st.key_weights.lens.tolist()[2] == 8
    plain_req = dict(reqs[1], attn_weights=None)
    assert st.admit(**plain_req) == 2 and st.key_weights.lens.tolist()[2::3] == [0, 0]
    for _ in range(STEPS):
        done = st.tick()
    assert done == [2]
    reused = st.result(2)
    fresh = _serve(mk(), [idle(0), idle(1)], {k: v for k, v in plain_req.items() if k != "attn_weights"}, 1)
    assert torch.equal(reused, fresh), "a reused slot inherits its predecessor's weights: %d positions differ from a fresh stream" % int((reused != fresh).sum())
    assert not torch.equal(reused, alone[1]), "the weights did not act"
    # (b) weights w at admission == a stream built with stream-wide attn_weights = w serving the same request
    wide = mk(attn_weights=w0)
    strip = lambda q: {k: v for k, v in q.items() if k != "attn_weights"}
    s = _serve(wide, [strip(idle(0)), strip(idle(1))], strip(reqs[0]), 1)
    assert torch.equal(s, alone[0]), "per-request weights differ from the stream-wide vector at %d positions" % int((s != alone[0]).sum())
    st.reset()
    assert st.key_weights.lens.tolist() == [0] * 6
    assert st.captures == 1 and wide.captures == 1                                   # (e)
    # (f) refusals
    with pytest.raises(ValueError, match="attn_weights"):
        st.admit(**dict(reqs[0], attn_weights=wt(9)))                               # longer than max_attn_weights
    with pytest.raises(ValueError, match="attn_weights"):
        wide.admit(**reqs[0])                                                       # a stream without the table
    with pytest.raises(ValueError, match="attn_weights"):
        mk(max_attn_weights=8, attn_weights=w0)                                     # mutually exclusive
    long = mk(max_attn_weights=64)
    with pytest.raises(ValueError, match="attn_weights"):
        long.admit(**dict(reqs[2], attn_weights=(None, wt(22))))                    # 16 self keys + 5 unconditional rows = 21 keys at the smallest attention level
    assert long.admit(**dict(reqs[2], attn_weights=(None, wt(21)))) == 0 and long.free_slots == [1, 2]


def test_request_stream_editing_with_weights(tiny):
    """(d) one editing request with pin="step" and weights == an editing stream with those weights stream-wide"""
    m, _ = tiny
    cfg, (B, H, W) = G.UNET_TINY, STREAM_SHAPE
    g = torch.Generator().manual_seed(12)
    w = (torch.rand(5, generator=g) * 1.5 + 0.25).to(DEV)
    known = torch.randint(0, cfg["num_labels"], (H, W), generator=g).to(DEV)
    mask = torch.zeros(H, W, dtype=torch.int64)
    mask[8:24, 4:20] = 1
    base = _request(cfg, 3, 0, 1)
    edit = dict(base, known=known, mask=mask.to(DEV), pin="step", t_start=0.7, temperature=(0.7, 0.3))
    mk = lambda **k: paella_amd.RequestStream(m, base["model_inputs"], base["unconditional_inputs"], STREAM_SHAPE, max_steps=4, device=DEV, editing=True, max_cond_rows=16, **k)
    mate = lambda i, **k: dict(_request(cfg, 3, 0, 50 + i, **k), steps=1)
    st, wide = mk(max_attn_weights=8), mk(attn_weights=w)
    a = _serve(st, [mate(0, attn_weights=(w[:2], None)), mate(1)], dict(edit, attn_weights=w), 1)
    s = _serve(wide, [mate(0), mate(1)], edit, 1)
    assert torch.equal(a, s), "editing request with weights differs from the stream-wide vector at %d positions" % int((a != s).sum())
    keep0 = mask.to(DEV) == 0
    assert torch.equal(a[keep0], known[keep0]) and st.captures == 1 and wide.captures == 1
    none = _serve(st, [mate(0), mate(1)], edit, 1)
    assert not torch.equal(none, a), "the weights did not act"


def test_fused_table_step_with_pin_tables(tiny):
    """paella_unet_forward_sample_req_kw with its pin tables: the tokens of forward_shared_req_kw + paella_sample_tail_req with the known tokens written, here in
    torch, wherever the pin applies to the slot (pin_on NULL: every slot) and keep == 0"""
    m, _ = tiny
    cfg, B, H = G.UNET_TINY, 2, 16
    L, hw = cfg["num_labels"], H * H
    cs, us = to_dev(cond_for(cfg, B, 3, 0, 1), DEV), to_dev(cond_for(cfg, B, 3, 0, 2), DEV)
    cache = m.prepare_cond(**{k: (torch.cat([cs[k], us[k]]) if cs[k] is not None else None) for k in cs})
    req = sampling.RequestTables(sampling.request_tables(B, 3, [11, (1 << 64) - 2], [3.0, (9.0, 5.0)], [(1.0, 0.2), (0.7, 0.3)]), DEV)
    g = torch.Generator().manual_seed(21)
    x = torch.randint(0, L, (B, H, H), generator=g).to(DEV)
    init = torch.randint(0, L, (B, H, H), generator=g).to(DEV)
    known = torch.randint(0, L, (B, H, H), generator=g).to(DEV)
    keep = (torch.rand(B, H, H, generator=g) < 0.5).to(torch.int64).to(DEV)
    r = torch.full((B,), 0.6, device=DEV)
    kw = _table([(torch.rand(5, generator=g) + 0.5).to(DEV), None, None, (torch.rand(2, generator=g) + 0.5).to(DEV)], 8, nan=True)
    h, lib = m._engine(), _lib.load()
    ws = m.new_workspace(2 * B, H, H, cache.S)
    step, t_next = 1, 0.55
    seeds, temps, pairs = req.step(step)
    lg = m._forward_prepared_raw(x, r, cache, req_mix=pairs, attn_weights=kw).reshape(B * hw, L)
    plain = torch.empty(B, H, H, dtype=torch.int64, device=DEV)
    _lib.check(lib.paella_sample_tail_req(_lib.ptr(lg), None, B * hw, L, None, _lib.ptr(temps), _lib.ptr(seeds), hw, step, _lib.ptr(init), t_next, _lib.ptr(plain), None,
                                          _stream()))
    torch.cuda.synchronize()
    for pin_on in (None, torch.tensor([0, 1], dtype=torch.int32, device=DEV)):
        on = torch.ones(B, dtype=torch.bool, device=DEV) if pin_on is None else pin_on.bool()
        want = torch.where(on[:, None, None] & (keep == 0), known, plain)
        got = torch.full((B, H, H), -1, dtype=torch.int64, device=DEV)
        _lib.check(lib.paella_unet_forward_sample_req_kw(h, _lib.ptr(x), _lib.ptr(r), _lib.ptr(cache.buf), 2 * B, B, _lib.ptr(pairs), H, H, cache.S, None, _lib.ptr(kw.buf),
                                                         _lib.ptr(kw.lens), kw.pitch, _lib.ptr(seeds), _lib.ptr(temps), hw, step, _lib.ptr(init), t_next, _lib.ptr(keep),
                                                         _lib.ptr(known), _lib.ptr(pin_on), _lib.ptr(got), _lib.ptr(ws), ws.numel(), _stream()))
        torch.cuda.synchronize()
        assert torch.equal(got, want), "pin_on %s: %d tokens differ" % (None if pin_on is None else pin_on.tolist(), int((got != want).sum()))
        assert not torch.equal(want, plain)
    # one pin table without the other is refused before anything is enqueued
    assert lib.paella_unet_forward_sample_req_kw(h, _lib.ptr(x), _lib.ptr(r), _lib.ptr(cache.buf), 2 * B, B, _lib.ptr(pairs), H, H, cache.S, None, _lib.ptr(kw.buf),
                                                 _lib.ptr(kw.lens), kw.pitch, _lib.ptr(seeds), _lib.ptr(temps), hw, step, _lib.ptr(init), t_next, _lib.ptr(keep), None, None,
                                                 _lib.ptr(got), _lib.ptr(ws), ws.numel(), _stream()) == -1


def test_sample_requests_weights_unguided_and_slot_placement(tiny):
    """the unguided list form (a table of B rows, no pair table) in the eager and the captured sampler; and where a guided list call puts every vector:
    request b's conditional vector in row b, its unconditional one in row B + b of the table every step's forward receives"""
    m, _ = tiny
    cfg, B, H = G.UNET_TINY, 3, 16
    cs, us = to_dev(cond_for(cfg, B, 3, 0, 1), DEV), to_dev(cond_for(cfg, B, 3, 0, 2), DEV)
    g = torch.Generator().manual_seed(14)
    wt = lambda n: (torch.rand(n, generator=g) * 1.5 + 0.25).to(DEV)
    w0, w2, o = wt(4), wt(7), wt(3)
    kw = dict(seeds=[9, 5, 77], cfg=None, temperature=[(1.0, 0.3), (0.8, 0.2), (0.6, 0.6)], steps=3, renoise_steps=2, device=DEV)
    run = lambda aw: paella_amd.sample_requests(m, cs, None, (B, H, H), attn_weights=aw, **kw)
    mixed = [w0, None, (w2, None)]
    got = run(mixed)
    everyone = [run(w0), run(None), run(w2)]
    for b in range(B):
        assert torch.equal(got[b], everyone[b][b]), "unguided request %d: %d tokens differ from the call in which everyone carries its weights" % (b, int((got[b] != everyone[b][b]).sum()))
    assert not torch.equal(everyone[0][0], everyone[1][0]), "the weights did not act"
    assert torch.equal(run([o, o, (w2, None)])[2], got[2])
    with pytest.raises(ValueError, match="unguided"):
        run([w0, None, (w2, o)])
    gr = paella_amd.GraphRequestSampler(m, cs, None, (B, H, H), steps=3, renoise_steps=2, cfg=None, device=DEV, max_attn_weights=8)
    assert gr.key_weights.buf.shape == (B, 8)
    for aw in (mixed, None, w2):
        out = gr([9, 5, 77], temperature=kw["temperature"], attn_weights=aw).clone()
        eager = run(aw)
        assert torch.equal(out, eager), "unguided graph replay differs from the eager call at %d positions" % int((out != eager).sum())
    assert gr.captures == 1
    # guided: the table every forward_sample call receives
    seen = []
    fs = m.forward_sample

    def spy(*a, **k):
        t = k["attn_weights"]
        seen.append((t.lens.tolist(), t.buf.clone()))
        return fs(*a, **k)
    m.forward_sample = spy
    try:
        paella_amd.sample_requests(m, cs, us, (B, H, H), seeds=[9, 5, 77], steps=3, renoise_steps=2, device=DEV, attn_weights=[(w0, o), None, (None, w2)])
    finally:
        del m.forward_sample
    assert len(seen) == 3
    for lens, buf in seen:
        assert lens == [4, 0, 0, 3, 0, 7]
        assert torch.equal(buf[0, :4], w0) and torch.equal(buf[3, :3], o) and torch.equal(buf[5, :7], w2)
