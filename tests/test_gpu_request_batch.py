"""GPU: the request batch (per-request seed, guidance and temperature inside one sampled batch; paella_amd.sample_requests, GraphRequestSampler and the
request forms of the tail kernels / the fused head).  The contract: request b draws what `sample(latent_shape=(1, H, W), noise="philox", seed=seeds[b])`
draws alone -- tests/counter_noise.py, called per request with seed=seeds[b], row_offset=0, is the independent model.  Token policy: exact where the
arithmetic is the same, otherwise every mismatch must sit at a model near-tie, counted and printed."""
import numpy as np
import pytest
import torch

import paella_amd
from oracle import golden_configs as G
from oracle import paella_oracle as O
from paella_amd import _lib, sampling
from tests import counter_noise as C
from tests.helpers import cond_for, to_dev, weights_for
from tests.test_gpu_counter_noise import HEAD_8K, SEED_HI, _cfg_logits, _compare_tokens, _near_tie_eps, _stream, _tail_ex

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _tables(B, steps, seeds, cfg, temperature):
    return sampling.RequestTables(sampling.request_tables(B, steps, seeds, cfg, temperature), torch.device(DEV))


def _tail_req(lc, lu, L, hw, req, step, out, sampled=None, init=None, t_next=0.0):
    _lib.check(_lib.load().paella_sample_tail_req(_lib.ptr(lc), _lib.ptr(lu), lc.size(0), L, _lib.ptr(None if lu is None else req.pairs[step]),
                                                  _lib.ptr(req.temps[step]), _lib.ptr(req.seeds), hw, step, _lib.ptr(init), t_next, _lib.ptr(out),
                                                  _lib.ptr(sampled), _stream()))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- 1. same logits -> same tokens
SEEDS5 = [SEED_HI, 3, (1 << 64) - 2, 77, SEED_HI ^ 0x5BD1E9955BD1E995]
TAIL_CASES = [(8192, 16, True), (8192, 256, False), (1028, 1024, True), (1028, 16, False), (12, 256, True), (12, 1024, False), (8192, 1024, True)]


@pytest.mark.parametrize("L,hw,guided", TAIL_CASES, ids=lambda v: str(v))
def test_request_tail_equals_the_scalar_tail_per_sample(built_lib, L, hw, guided):
    B = 3 if hw == 1024 else 5
    steps, step = 4, 2
    seeds = SEEDS5[:B]
    req = _tables(B, steps, seeds, [3.0, 8.0, (9.0, 5.0), 1.0, 7.5][:B] if guided else None, [(1.0, 0.2), (0.7, 0.3), (0.9, 0.9), (0.05, 0.4), (1.3, 1.0)][:B])
    rows = B * hw
    lc, lu = _cfg_logits(rows, L, L + hw)
    g = torch.Generator().manual_seed(5)
    init = torch.randint(0, L, (rows,), generator=g).to(DEV)
    lcd, lud = lc.to(DEV), (lu.to(DEV) if guided else None)
    out, pre = torch.empty(rows, dtype=torch.int64, device=DEV), torch.empty(rows, dtype=torch.int64, device=DEV)
    t_next = 0.45
    _tail_req(lcd, lud, L, hw, req, step, out, pre, init, t_next)
    temps, pairs = req.temps.cpu(), (req.pairs.cpu() if guided else None)
    o1, p1 = torch.empty(hw, dtype=torch.int64, device=DEV), torch.empty(hw, dtype=torch.int64, device=DEV)
    for b in range(B):
        sl = slice(b * hw, (b + 1) * hw)
        cfg, omc = (float(pairs[step, b, 0]), float(pairs[step, b, 1])) if guided else (1.0, 0.0)
        T = float(temps[step, b])
        _tail_ex(lcd[sl].contiguous(), None if lud is None else lud[sl].contiguous(), L, cfg, omc, T, 0, seeds[b], step, o1, p1, init=init[sl].contiguous(), t_next=t_next)
        assert torch.equal(pre[sl], p1), "request %d: pre-renoise tokens differ from the scalar tail at %d rows" % (b, int((pre[sl] != p1).sum()))
        assert torch.equal(out[sl], o1), "request %d: final tokens differ from the scalar tail" % b
        # and the numpy model, called per request with its own seed and row offset 0
        mp, mf, margin = C.sample_tail(lc[sl].numpy(), T, seeds[b], step, lu=lu[sl].numpy() if guided else None, cfg=cfg, omc=omc, init_noise=init[sl].cpu().numpy(), t_next=t_next)
        mask = C.renoise_mask(seeds[b], hw, step, t_next)
        top = float(np.abs(C.scaled_logits(C.mix_logits(lc[sl].numpy(), lu[sl].numpy() if guided else None, cfg, omc), T)).max()) + 17.0
        _compare_tokens("request tail L=%d hw=%d request %d" % (L, hw, b), out[sl].cpu().numpy(), mp, mf, margin, _near_tie_eps(top), mask, pre[sl].cpu().numpy())


def test_request_start_tokens(built_lib):
    for L, hw in [(8192, 1024), (1000, 16), (64, 192)]:
        B = len(SEEDS5)
        seeds_dev = torch.tensor([sampling.seed_word(s) for s in SEEDS5], dtype=torch.int64, device=DEV)
        got = sampling.start_tokens_requests(L, (B, hw, 1), seeds_dev).cpu().numpy().reshape(B, hw)
        one = torch.empty(hw, dtype=torch.int64, device=DEV)
        for b, s in enumerate(SEEDS5):
            _lib.check(built_lib.paella_start_tokens(s, None, 0, None, L, hw, _lib.ptr(one), _stream()))
            torch.cuda.synchronize()
            assert np.array_equal(got[b], one.cpu().numpy()) and np.array_equal(got[b], C.start_tokens(s, hw, L))


def test_argument_errors_of_the_c_abi(built_lib):
    x = torch.zeros(64, 12, device=DEV)
    out = torch.zeros(64, dtype=torch.int64, device=DEV)
    req = _tables(2, 1, [1, 2], None, (1.0, 1.0))
    lib = built_lib
    assert lib.paella_sample_tail_req(_lib.ptr(x), None, 64, 12, None, _lib.ptr(req.temps[0]), None, 32, 0, None, 0.0, _lib.ptr(out), None, _stream()) == -1
    assert lib.paella_sample_tail_req(_lib.ptr(x), None, 64, 12, None, _lib.ptr(req.temps[0]), _lib.ptr(req.seeds), 48, 0, None, 0.0, _lib.ptr(out), None, _stream()) == -1
    assert b"rows_per_sample" in lib.paella_last_error()
    assert lib.paella_start_tokens_req(None, 2, 32, 12, _lib.ptr(out), _stream()) == -1


# ---------------------------------------------------------------------------------------------------------------- models
@pytest.fixture(scope="module")
def tiny_sd(built_lib):
    m = paella_amd.Paella(**G.UNET_TINY)
    sd = weights_for(m, sum(G.UNET_TINY["blocks"]))
    return m.to(DEV), sd


@pytest.fixture(scope="module")
def head8k(built_lib):
    m = paella_amd.Paella(**HEAD_8K)
    weights_for(m, sum(HEAD_8K["blocks"]))
    return m.to(DEV)


def _conds(cfg, B, seed=1):
    return to_dev(cond_for(cfg, B, 3, 0, seed), DEV), to_dev(cond_for(cfg, B, 3, 0, seed + 1), DEV)


KW = dict(steps=4, renoise_steps=3)
REQ3 = dict(seeds=[0xF00DFACE00C0FFEE, 5, SEED_HI], cfg=[3.0, 8.0, (9.0, 5.0)], temperature=[(1.0, 0.3), (0.8, 0.2), (0.6, 0.6)])


# ---------------------------------------------------------------------------------------------------------------- 2. one request == today's call
@pytest.mark.parametrize("shape", [(1, 16, 16), (1, 24, 8)])
def test_one_request_equals_sample(tiny_sd, shape):
    m, _ = tiny_sd
    cs, us = _conds(G.UNET_TINY, 1)
    for s, cfg, temp in [(SEED_HI, 8.0, (1.0, 0.2)), (11, 3.5, (0.7, 0.3))]:
        ref = paella_amd.sample(m, cs, shape, unconditional_inputs=us, cfg=cfg, temperature=temp, device=DEV, noise="philox", seed=s, **KW)
        assert torch.equal(paella_amd.sample_requests(m, cs, us, shape, [s], cfg=cfg, temperature=temp, device=DEV, **KW), ref)
        assert torch.equal(paella_amd.sample_requests(m, cs, us, shape, [s], cfg=cfg, temperature=temp, device=DEV, fused_tail=False, **KW), ref)
    ref = paella_amd.sample(m, cs, shape, cfg=None, device=DEV, noise="philox", seed=9, **KW)
    assert torch.equal(paella_amd.sample_requests(m, cs, None, shape, [9], cfg=None, device=DEV, **KW), ref)
    gs = paella_amd.GraphSampler(m, cs, us, shape, device=DEV, **KW)
    gr = paella_amd.GraphRequestSampler(m, cs, us, shape, device=DEV, **KW)
    assert torch.equal(gr([SEED_HI]), gs(seed=SEED_HI))


# ---------------------------------------------------------------------------------------------------------------- 3. fused == unfused, 4. against the model
def _fused_vs_unfused_and_model(m, cfg, B, H, W, what, guided=True):
    L, hw = cfg["num_labels"], H * W
    rows = B * hw
    seeds = (SEEDS5 * 2)[:B]
    req = _tables(B, 3, seeds, ([3.0, 8.0, (9.0, 5.0), 1.0] * 2)[:B] if guided else None, ([(1.0, 0.2), (0.7, 0.3), (0.4, 0.9), (1.2, 1.0)] * 2)[:B])
    cs, us = _conds(cfg, B)
    both = {k: (torch.cat([cs[k], us[k]]) if cs[k] is not None else None) for k in cs}
    cache = m.prepare_cond(**(both if guided else cs))
    g = torch.Generator().manual_seed(9)
    x = torch.randint(0, L, (B, H, W), generator=g).to(DEV)
    init = torch.randint(0, L, (B, H, W), generator=g).to(DEV)
    r = torch.full((B,), 0.6, device=DEV)
    fused, unfused, pre = (torch.empty(B, H, W, dtype=torch.int64, device=DEV) for _ in range(3))
    for step, renoise in [(0, False), (2, True)]:
        t_next = 0.55 if renoise else 0.0
        m.forward_sample(x, r, cache, fused, temperature=1.0, offset=step, init_noise=init if renoise else None, t_next=t_next, req=req.step(step))
        logits = m._forward_prepared_raw(x, r, cache, req_mix=req.pairs[step]) if guided else m._forward_prepared_raw(x, r, cache)
        lg = logits.reshape(rows, L)
        only_temps = sampling.RequestTables((req.seeds, req.temps, None), DEV)
        _tail_req(lg, None, L, hw, only_temps, step, unfused.view(-1), pre.view(-1), init.view(-1) if renoise else None, t_next)
        assert torch.equal(fused, unfused), "%s step %d: fused request step differs from forward_shared + request tail at %d positions" % (what, step, int((fused != unfused).sum()))
        lgn, temps = lg.cpu().numpy(), req.temps.cpu()
        for b in range(B):
            sl = slice(b * hw, (b + 1) * hw)
            T = float(temps[step, b])
            mp, mf, margin = C.sample_tail(lgn[sl], T, seeds[b], step, init_noise=init.view(-1)[sl].cpu().numpy() if renoise else None, t_next=t_next)
            mask = C.renoise_mask(seeds[b], hw, step, t_next) if renoise else None
            top = float(np.abs(C.scaled_logits(lgn[sl], T)).max()) + 17.0
            _compare_tokens("%s step %d request %d" % (what, step, b), fused.view(-1)[sl].cpu().numpy(), mp, mf, margin, _near_tie_eps(top), mask)


@pytest.mark.parametrize("grid", [(4, 8, 8), (3, 24, 8), (2, 16, 16)], ids=lambda g: "%dx%dx%d" % g)
def test_fused_request_step_tiny(tiny_sd, grid):
    """UNET_TINY (tile 2, 64 rows): 8x8 = 64 positions fill a tile exactly, 24x8 = 192 make tiles span samples at B = 3"""
    _fused_vs_unfused_and_model(tiny_sd[0], G.UNET_TINY, grid[0], grid[1], grid[2], "UNET_TINY %s" % (grid,))
    _fused_vs_unfused_and_model(tiny_sd[0], G.UNET_TINY, grid[0], grid[1], grid[2], "UNET_TINY %s unguided" % (grid,), guided=False)


@pytest.mark.parametrize("tile", [9, 14, 18])
def test_fused_request_step_large_head(built_lib, head8k, tile):
    built_lib.paella_test_gemm_tail_tile(tile)
    try:
        _fused_vs_unfused_and_model(head8k, HEAD_8K, 2, 32, 32, "8192-label head, tile %d" % tile)
        _fused_vs_unfused_and_model(head8k, HEAD_8K, 6, 24, 8, "8192-label head, tile %d, 24x8" % tile)  # 192-position samples under 128- / 64-row tiles
    finally:
        built_lib.paella_test_gemm_tail_tile(18)


def test_fused_request_step_bf16(built_lib, head8k):
    head8k.set_gemm_precision("bf16")
    try:
        _fused_vs_unfused_and_model(head8k, HEAD_8K, 2, 32, 32, "8192-label head, bf16")
        _fused_vs_unfused_and_model(head8k, HEAD_8K, 6, 24, 8, "8192-label head, bf16, 24x8")
    finally:
        head8k.set_gemm_precision("fp32")


# ---------------------------------------------------------------------------------------------------------------- 5. closed loop
def _record(m, fused, run):
    rec = []
    if fused:
        orig = m.forward_sample

        def fs(x, r, cond, out, **k):
            xin = x.clone()
            res = orig(x, r, cond, out, **k)
            rec.append([xin, out.clone()])
            return res
        m.forward_sample = fs
        try:
            toks = run()
        finally:
            del m.forward_sample
    else:
        orig_fp, orig_tail = m.forward_prepared, sampling._tail_req

        def fp(x, *a, **k):
            rec.append([x.clone(), None])
            return orig_fp(x, *a, **k)

        def tail(*a, **k):
            orig_tail(*a, **k)
            rec[-1][1] = a[9].clone()
        m.forward_prepared, sampling._tail_req = fp, tail
        try:
            toks = run()
        finally:
            del m.forward_prepared
            sampling._tail_req = orig_tail
    torch.cuda.synchronize()
    return toks, [(a.cpu(), b.cpu()) for a, b in rec]


@pytest.mark.parametrize("variant", ["fused", "unfused", "graph"])
def test_request_batch_closed_loop_against_oracle_and_model(tiny_sd, variant):
    """B = 3 requests (guidance 3, 8 and the schedule (9, 5); three temperature ranges; a seed with its high bits set) on UNET_TINY, 4 steps, 3 renoised: at
    every step the oracle's UNet on the DEVICE's input tokens plus the model's per-request draws give the device's tokens, except where the model's margin is
    below eps = 2 (max|oracle - device mixed logit| / T + delta) + ulp (as test_sample_closed_loop_against_oracle_and_model); start tokens and renoised rows exact."""
    m, sd = tiny_sd
    cfg = G.UNET_TINY
    L, B, H = cfg["num_labels"], 3, 16
    hw = H * H
    steps, renoise_steps = KW["steps"], KW["renoise_steps"]
    c, u = cond_for(cfg, B, 3, 1, 1), cond_for(cfg, B, 3, 1, 2)
    cs, us = to_dev(c, DEV), to_dev(u, DEV)
    run = lambda fused=True: paella_amd.sample_requests(m, cs, us, (B, H, H), device=DEV, fused_tail=fused, **REQ3, **KW)
    toks, rec = _record(m, variant != "unfused", (lambda: run(False)) if variant == "unfused" else run)
    if variant == "graph":
        gr = paella_amd.GraphRequestSampler(m, cs, us, (B, H, H), device=DEV, **KW)
        got = gr(**REQ3).clone()
        torch.cuda.synchronize()
        assert torch.equal(got, toks), "graph replay differs from the eager call at %d positions" % int((got != toks).sum())
        toks = got
    assert len(rec) == steps
    seeds = REQ3["seeds"]
    _, temp_t, pair_t = sampling.request_tables(B, steps, **REQ3)
    start = np.concatenate([C.start_tokens(s, hw, L) for s in seeds])
    assert np.array_equal(rec[0][0].numpy().reshape(-1), start), "start tokens differ from the model"
    t_list = [float(v) for v in torch.linspace(1.0, 0.0, steps + 1)]
    cache = m.prepare_cond(**to_dev({k: (torch.cat([c[k], u[k]]) if c[k] is not None else None) for k in c}, DEV))
    near_total = 0
    for i in range(steps):
        x_i, got = rec[i]
        if i:
            assert torch.equal(x_i, rec[i - 1][1])
        r = torch.ones(B) * t_list[i]
        with torch.no_grad():
            lc = O.unet_forward(sd, cfg, x_i, r, **c).permute(0, 2, 3, 1).reshape(B * hw, L).numpy()
            lu = O.unet_forward(sd, cfg, x_i, r, **u).permute(0, 2, 3, 1).reshape(B * hw, L).numpy()
        dev_logits = m._forward_prepared_raw(x_i.to(DEV), r.to(DEV), cache, req_mix=pair_t[i].to(DEV)).reshape(B * hw, L).cpu().numpy()
        renoise = i < renoise_steps
        t_next = t_list[i + 1] if renoise else 0.0
        for b in range(B):
            sl = slice(b * hw, (b + 1) * hw)
            pair, T = (float(pair_t[i, b, 0]), float(pair_t[i, b, 1])), float(temp_t[i, b])
            mix = C.mix_logits(lc[sl], lu[sl], *pair)
            diff = float(np.abs(dev_logits[sl].astype(np.float64) - mix).max())
            pre, final, margin = C.sample_tail(lc[sl], T, seeds[b], i, lu=lu[sl], cfg=pair[0], omc=pair[1], init_noise=start[sl] if renoise else None, t_next=t_next)
            mask = C.renoise_mask(seeds[b], hw, i, t_next) if renoise else None
            eps = _near_tie_eps(float(np.abs(C.scaled_logits(mix, T)).max()) + 17.0, diff * float(C.inv_temperature(T)))
            near_total += _compare_tokens("%s step %d request %d (max |oracle - device logit| %.2e)" % (variant, i, b, diff), got.numpy().reshape(-1)[sl], pre, final, margin, eps, mask)
    assert torch.equal(toks.cpu(), rec[-1][1])
    print("%s: %d differing tokens at model near-ties over %d steps" % (variant, near_total, steps))


# ---------------------------------------------------------------------------------------------------------------- 6. slot / batch-mate independence
def test_request_does_not_depend_on_slot_or_batch_mates(tiny_sd):
    """The same request in slot 0 of one batch and in slot B-1 of another with different neighbours, teacher-forced per step on the same input tokens: its
    tokens may differ only where the request-form score hook puts the top-1 / top-2 margin below twice the MEASURED logit difference between the placements."""
    m, _ = tiny_sd
    cfg = G.UNET_TINY
    L, B, H = cfg["num_labels"], 4, 16
    hw = H * H
    steps = 3
    mine = dict(seed=SEED_HI, cfg=(9.0, 5.0), temperature=(0.9, 0.3))
    ca, ua = cond_for(cfg, B, 3, 0, 1), cond_for(cfg, B, 3, 0, 2)
    cb, ub = cond_for(cfg, B, 3, 0, 5), cond_for(cfg, B, 3, 0, 6)
    for k in ca:  # request `mine` carries its own conditioning: slot 0 of batch A, slot B-1 of batch B
        if ca[k] is not None:
            cb[k][B - 1], ub[k][B - 1] = ca[k][0], ua[k][0]
    place = [(0, ca, ua, _tables(B, steps, [mine["seed"], 1, 2, 3], [mine["cfg"], 3.0, 8.0, 1.0], [mine["temperature"], (1.0, 0.2), (0.5, 0.5), (0.7, 0.1)])),
             (B - 1, cb, ub, _tables(B, steps, [9, 8, 7, mine["seed"]], [2.0, (4.0, 6.0), 7.0, mine["cfg"]], [(0.3, 0.3), (1.1, 0.9), (0.6, 0.2), mine["temperature"]]))]
    g = torch.Generator().manual_seed(3)
    diff_total = 0
    for step in range(steps):
        x1 = torch.randint(0, L, (1, H, H), generator=g)
        init1 = torch.randint(0, L, (1, H, H), generator=g)
        res = []
        for slot, c, u, req in place:
            x = torch.randint(0, L, (B, H, H), generator=g)
            init = torch.randint(0, L, (B, H, H), generator=g)
            x[slot], init[slot] = x1[0], init1[0]
            x, init = x.to(DEV), init.to(DEV)
            cache = m.prepare_cond(**to_dev({k: (torch.cat([c[k], u[k]]) if c[k] is not None else None) for k in c}, DEV))
            r = torch.full((B,), 0.7, device=DEV)
            out = torch.empty(B, H, H, dtype=torch.int64, device=DEV)
            m.forward_sample(x, r, cache, out, temperature=1.0, offset=step, init_noise=init, t_next=0.4, req=req.step(step))
            logits = m._forward_prepared_raw(x, r, cache, req_mix=req.pairs[step]).reshape(B * hw, L)
            scores = torch.empty_like(logits)
            _lib.check(_lib.load().paella_test_tail_scores_req(_lib.ptr(logits), None, B * hw, L, None, _lib.ptr(req.temps[step]), _lib.ptr(req.seeds), hw, step,
                                                               _lib.ptr(scores), _stream()))
            torch.cuda.synchronize()
            sl = slice(slot * hw, (slot + 1) * hw)
            res.append((out.view(-1)[sl].cpu(), logits[sl].cpu().double(), scores[sl].cpu().double(), float(req.temps[step, slot])))
        (ta, la, sa, T), (tb, lb, sb, _) = res
        ldiff = float((la - lb).abs().max())
        sdiff = float((sa - sb).abs().max())  # the same noise on both sides: the logit difference as the scores see it (times 1 / T), in the margin's units
        top = sa.topk(2, dim=1).values
        margin = top[:, 0] - top[:, 1]
        bound = 2.0 * sdiff
        mism = ta != tb
        n_clear = int((mism & (margin > bound)).sum())
        print("step %d: max |logit difference| between the two placements %.3e (T %.3f), %d of %d tokens differ, %d of them above the margin bound %.3e"
              % (step, ldiff, T, int(mism.sum()), hw, n_clear, bound))
        assert n_clear == 0
        diff_total += int(mism.sum())
    print("slot independence: %d differing tokens over %d steps, all at near-ties" % (diff_total, steps))


# ---------------------------------------------------------------------------------------------------------------- 7. graph
def test_graph_request_sampler_replays_without_recapture(tiny_sd):
    m, sd = tiny_sd
    cfg = G.UNET_TINY
    shape = (3, 24, 8)
    cs, us = _conds(cfg, 3)
    gr = paella_amd.GraphRequestSampler(m, cs, us, shape, device=DEV, **KW)
    sets = [REQ3, dict(seeds=[1, 2, 3], cfg=8.0, temperature=(1.0, 0.2)), dict(seeds=[SEED_HI, SEED_HI, 4], cfg=[(2.0, 6.0), 1.0, 4.5], temperature=[(0.5, 0.5), (1.0, 0.1), (0.9, 0.8)])]
    for s in sets:
        eager = paella_amd.sample_requests(m, cs, us, shape, device=DEV, **s, **KW)
        got = gr(**s)
        assert torch.equal(got, eager), "replay differs from the eager call at %d positions" % int((got != eager).sum())
        assert gr.captures == 1
    m.load_state_dict({k: v * 1.05 for k, v in sd.items()})
    try:
        eager = paella_amd.sample_requests(m, cs, us, shape, device=DEV, **REQ3, **KW)
        assert torch.equal(gr(**REQ3), eager) and gr.captures == 2
    finally:
        m.load_state_dict(sd)
    with pytest.raises(ValueError):
        gr([1, 2, 3], temperature=(1.0, 0.0))
    with pytest.raises(ValueError):
        gr([1, 2])
