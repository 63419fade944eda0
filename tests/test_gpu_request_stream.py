"""GPU: continuous request batching (paella_amd.RequestStream; the stream forms of the tail kernels and of the fused head; request_step_kernel).
The contract: a request admitted to a stream draws at its step j what `sample_distributed(latent_shape=(1, H, W), noise="philox", seed=seed)` draws at step j
-- tests/counter_noise.py per request at the request's OWN step index is the independent model -- and at a given slot and B its tokens do not depend on the
batch-mates or on the tick it was admitted at, bit for bit.  Token policy as tests/test_gpu_request_batch.py: exact where the arithmetic is the same."""
import re

import numpy as np
import pytest
import torch

import paella_amd
from oracle import golden_configs as G
from oracle import paella_oracle as O
from paella_amd import _lib, sampling
from tests import counter_noise as C
from tests import test_gpu_request_batch as RB
from tests.helpers import cond_for, to_dev, weights_for
from tests.test_gpu_counter_noise import HEAD_8K, SEED_HI, _cfg_logits, _compare_tokens, _near_tie_eps, _stream, _tail_ex
from tests.test_gpu_request_batch import KW, REQ3, SEEDS5, TAIL_CASES, _conds, _tables, _tail_req, head8k, tiny_sd  # noqa: F401  (fixtures)
from tests.test_request_stream import request_step_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -7


def _i32(v):
    return torch.tensor(v, dtype=torch.int32, device=DEV)


def _f32(v):
    return torch.tensor(v, dtype=torch.float32, device=DEV)


def _tail_stream(lc, lu, L, hw, pairs, temps, seeds, step, t_next, active, init, out, sampled=None):
    _lib.check(_lib.load().paella_sample_tail_stream(_lib.ptr(lc), _lib.ptr(lu), lc.size(0), L, _lib.ptr(pairs), _lib.ptr(temps), _lib.ptr(seeds), hw, _lib.ptr(step),
                                                     _lib.ptr(t_next), _lib.ptr(active), _lib.ptr(init), _lib.ptr(out), _lib.ptr(sampled), _stream()))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- 1. the stream tail
@pytest.mark.parametrize("L,hw,guided", TAIL_CASES, ids=lambda v: str(v))
def test_stream_tail_equals_the_request_tail_and_the_scalar_tail(built_lib, L, hw, guided):
    B = 3 if hw == 1024 else 5
    steps, i, t = 4, 2, 0.45
    seeds = SEEDS5[:B]
    req = _tables(B, steps, seeds, [3.0, 8.0, (9.0, 5.0), 1.0, 7.5][:B] if guided else None, [(1.0, 0.2), (0.7, 0.3), (0.9, 0.9), (0.05, 0.4), (1.3, 1.0)][:B])
    rows = B * hw
    lc, lu = _cfg_logits(rows, L, L + hw)
    g = torch.Generator().manual_seed(5)
    init = torch.randint(0, L, (rows,), generator=g).to(DEV)
    lcd, lud = lc.to(DEV), (lu.to(DEV) if guided else None)
    pairs = req.pairs[i] if guided else None
    new = lambda: torch.full((rows,), SENTINEL, dtype=torch.int64, device=DEV)
    # (a) all slots at step i with threshold t == the request tail with offset = i, t_next = t
    want, want_pre, got, got_pre = new(), new(), new(), new()
    _tail_req(lcd, lud, L, hw, req, i, want, want_pre, init, t)
    _tail_stream(lcd, lud, L, hw, pairs, req.temps[i], req.seeds, _i32([i] * B), _f32([t] * B), _i32([1] * B), init, got, got_pre)
    assert torch.equal(got, want) and torch.equal(got_pre, want_pre)
    # (b) every request at its own step and threshold, one without renoise, one slot inactive == the scalar tail called for that request alone
    step_b = [3, 0, 7, 1, 2][:B]
    t_b = [0.45, -1.0, 0.9, 0.05, 0.3][:B]
    act_b = [1, 1, 0, 1, 1][:B]
    got, got_pre = new(), new()
    _tail_stream(lcd, lud, L, hw, pairs, req.temps[i], req.seeds, _i32(step_b), _f32(t_b), _i32(act_b), init, got, got_pre)
    temps, pairs_h = req.temps.cpu(), (req.pairs.cpu() if guided else None)
    o1, p1 = torch.empty(hw, dtype=torch.int64, device=DEV), torch.empty(hw, dtype=torch.int64, device=DEV)
    for b in range(B):
        sl = slice(b * hw, (b + 1) * hw)
        if not act_b[b]:
            assert bool((got[sl] == SENTINEL).all()) and bool((got_pre[sl] == SENTINEL).all()), "an inactive slot's rows were written"
            continue
        cfg, omc = (float(pairs_h[i, b, 0]), float(pairs_h[i, b, 1])) if guided else (1.0, 0.0)
        renoise = t_b[b] >= 0
        _tail_ex(lcd[sl].contiguous(), None if lud is None else lud[sl].contiguous(), L, cfg, omc, float(temps[i, b]), 0, seeds[b], step_b[b], o1, p1,
                 init=init[sl].contiguous() if renoise else None, t_next=t_b[b] if renoise else 0.0)
        assert torch.equal(got_pre[sl], p1), "request %d: pre-renoise tokens differ from the scalar tail at its own step" % b
        assert torch.equal(got[sl], o1), "request %d: final tokens differ from the scalar tail" % b
        if not renoise:
            assert torch.equal(got[sl], got_pre[sl]), "a negative threshold renoised"


def test_stream_argument_errors_of_the_c_abi(built_lib):
    x = torch.zeros(64, 12, device=DEV)
    out = torch.zeros(64, dtype=torch.int64, device=DEV)
    req = _tables(2, 1, [1, 2], None, (1.0, 1.0))
    st, tn, ac = _i32([0, 0]), _f32([0.5, 0.5]), _i32([1, 1])
    lib, p = built_lib, _lib.ptr
    call = lambda step, t_next, active, init: lib.paella_sample_tail_stream(p(x), None, 64, 12, None, p(req.temps[0]), p(req.seeds), 32, p(step), p(t_next), p(active),
                                                                            p(init), p(out), None, _stream())
    assert call(st, tn, ac, out) == 0
    for bad in [(None, tn, ac, out), (st, None, ac, out), (st, tn, None, out), (st, tn, ac, None)]:
        assert call(*bad) == -1
    assert b"required" in lib.paella_last_error()
    assert lib.paella_request_step(None, 4, p(st), p(st), 2, p(tn), p(tn), None, p(tn), p(st), p(ac), _stream()) == -1
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- 2. fused == unfused, stream form
def _fused_vs_unfused_stream(m, cfg, B, H, W, what, guided=True):
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
    r = _f32([0.6, 0.3, 0.9, 0.1, 0.5, 0.7][:B])
    step = _i32([5, 0, 2, 9, 1, 3][:B])          # step words differ per request
    t_next = _f32([0.55, -1.0, 0.2, 0.8, -1.0, 0.4][:B])
    active = _i32([1, 0, 1, 1, 1, 1][:B])        # slot 1 is inactive
    fused = torch.full((B, H, W), SENTINEL, dtype=torch.int64, device=DEV)
    unfused = fused.clone()
    row = 1  # a step of the tables; the temperatures and pairs of that row are this tick's
    m.forward_sample(x, r, cache, fused, temperature=1.0, init_noise=init, req=req.step(row), stream=(step, t_next, active))
    logits = m._forward_prepared_raw(x, r, cache, req_mix=req.pairs[row]) if guided else m._forward_prepared_raw(x, r, cache)
    _tail_stream(logits.reshape(rows, L), None, L, hw, None, req.temps[row], req.seeds, step, t_next, active, init.view(-1), unfused.view(-1))
    assert torch.equal(fused, unfused), "%s: fused stream step differs from forward_shared_req + stream tail at %d positions" % (what, int((fused != unfused).sum()))
    assert bool((fused[1] == SENTINEL).all()) and not bool((fused[0] == SENTINEL).all())
    # in place: the same tick with out == x
    xin = x.clone()
    m.forward_sample(xin, r, cache, xin, temperature=1.0, init_noise=init, req=req.step(row), stream=(step, t_next, active))
    want = fused.clone()
    want[1] = x[1]
    assert torch.equal(xin, want), "%s: the in-place tick differs" % what


@pytest.mark.parametrize("grid", [(4, 8, 8), (3, 24, 8), (2, 16, 16)], ids=lambda g: "%dx%dx%d" % g)
def test_fused_stream_step_tiny(tiny_sd, grid):
    _fused_vs_unfused_stream(tiny_sd[0], G.UNET_TINY, grid[0], grid[1], grid[2], "UNET_TINY %s" % (grid,))
    _fused_vs_unfused_stream(tiny_sd[0], G.UNET_TINY, grid[0], grid[1], grid[2], "UNET_TINY %s unguided" % (grid,), guided=False)


@pytest.mark.parametrize("tile", [9, 14, 18])
def test_fused_stream_step_large_head(built_lib, head8k, tile):
    built_lib.paella_test_gemm_tail_tile(tile)
    try:
        _fused_vs_unfused_stream(head8k, HEAD_8K, 2, 32, 32, "8192-label head, tile %d" % tile)
        _fused_vs_unfused_stream(head8k, HEAD_8K, 6, 24, 8, "8192-label head, tile %d, 24x8" % tile)
    finally:
        built_lib.paella_test_gemm_tail_tile(18)


def test_fused_stream_step_bf16(built_lib, head8k):
    head8k.set_gemm_precision("bf16")
    try:
        _fused_vs_unfused_stream(head8k, HEAD_8K, 2, 32, 32, "8192-label head, bf16")
        _fused_vs_unfused_stream(head8k, HEAD_8K, 6, 24, 8, "8192-label head, bf16, 24x8")
    finally:
        head8k.set_gemm_precision("fp32")


# ---------------------------------------------------------------------------------------------------------------- 3. lock-step tie to the request batch
def test_lock_step_stream_tick_equals_the_request_step(tiny_sd):
    """one shared CondCache; a stream tick whose tables say "all slots at step i" == forward_sample(req=..., offset=i, t_next=...) for every i of a 4-step run"""
    m, _ = tiny_sd
    cfg = G.UNET_TINY
    B, H, steps, renoise_steps = 3, 16, KW["steps"], KW["renoise_steps"]
    cs, us = _conds(cfg, B)
    cache = m.prepare_cond(**{k: (torch.cat([cs[k], us[k]]) if cs[k] is not None else None) for k in cs})
    req = _tables(B, steps, **REQ3)
    init = sampling.start_tokens_requests(cfg["num_labels"], (B, H, H), req.seeds)
    t_list = sampling.linspace_schedule(1.0, 0.0, steps + 1)
    x = init.clone()
    for i in range(steps):
        renoise = i < renoise_steps
        r = _f32([t_list[i]] * B)
        want, got = torch.empty_like(x), x.clone()
        m.forward_sample(x, r, cache, want, temperature=1.0, offset=i, init_noise=init if renoise else None, t_next=t_list[i + 1] if renoise else 0.0, req=req.step(i))
        m.forward_sample(got, r, cache, got, temperature=1.0, init_noise=init, req=req.step(i),
                         stream=(_i32([i] * B), _f32([t_list[i + 1] if renoise else -1.0] * B), _i32([1] * B)))
        assert torch.equal(got, want), "step %d: the lock-step stream tick differs from the request step at %d positions" % (i, int((got != want).sum()))
        x = want


# ---------------------------------------------------------------------------------------------------------------- 4. request_step_kernel
@pytest.mark.parametrize("guided", [True, False])
def test_request_step_kernel_against_its_model(built_lib, guided):
    B, max_steps = 300, 6  # more than one 256-thread workgroup
    rng = np.random.default_rng(1)
    program = np.tile(np.float32([0.0, 1.0, 1.0, 0.0, -1.0]), (B, max_steps, 1))
    pos, length = np.zeros(B, np.int32), np.zeros(B, np.int32)
    d_prog, d_pos, d_len = torch.from_numpy(program).to(DEV), torch.from_numpy(pos).to(DEV), torch.from_numpy(length).to(DEV)
    d_r, d_t, d_tn = (torch.full((B,), 99.0, device=DEV) for _ in range(3))
    d_pairs = torch.full((B, 2), 99.0, device=DEV) if guided else None
    d_step, d_act = _i32([-1] * B), _i32([-1] * B)
    for tick in range(12):
        for b in rng.choice(B, 40, replace=False):  # staggered admissions into slots that are idle
            if pos[b] >= length[b]:
                n = int(rng.integers(1, max_steps + 1))
                program[b, :n] = rng.standard_normal((n, 5)).astype(np.float32)
                length[b], pos[b] = n, 0
        d_prog.copy_(torch.from_numpy(program))
        d_len.copy_(torch.from_numpy(length))
        d_pos.copy_(torch.from_numpy(pos))
        want = request_step_model(program, pos, length)
        _lib.check(built_lib.paella_request_step(_lib.ptr(d_prog), max_steps, _lib.ptr(d_pos), _lib.ptr(d_len), B, _lib.ptr(d_r), _lib.ptr(d_t), _lib.ptr(d_pairs),
                                                 _lib.ptr(d_tn), _lib.ptr(d_step), _lib.ptr(d_act), _stream()))
        torch.cuda.synchronize()
        got = (d_r, d_t, d_pairs, d_tn, d_step, d_act)
        for name, g_, w_ in zip(("r", "temperature", "pairs", "t_next", "step", "active"), got, want):
            if g_ is not None:
                assert np.array_equal(g_.cpu().numpy(), w_), "tick %d: %s differs from the model" % (tick, name)
        assert np.array_equal(d_pos.cpu().numpy(), pos), "tick %d: cursors differ" % tick
        assert 0 < int(want[5].sum()) < B


# ---------------------------------------------------------------------------------------------------------------- 5. admission-time independence
def _one(cfg, seed):
    return to_dev(cond_for(cfg, 1, 3, 0, seed), DEV), to_dev(cond_for(cfg, 1, 3, 0, seed + 100), DEV)


def _request(model_cfg, cseed, **kw):
    c, u = _one(model_cfg, cseed)
    return dict(model_inputs=c, unconditional_inputs=u, **kw)


def _admission_independence(m, cfg, H, graph=True):
    """request X (a high-bit seed, the guidance schedule (9, 5), 5 steps) always in slot 2 of B = 4.  Run A: admitted at tick 0 together with three others of 3, 4
    and 6 steps.  Run B: admitted at tick 3 into a stream whose slots 0 and 1 hold different requests mid-flight; slot 3 is idle.  Returns both token grids."""
    ex_c, ex_u = _one(cfg, 1)
    X = _request(cfg, 50, seed=SEED_HI, cfg=(9.0, 5.0), steps=5, temperature=(0.9, 0.3))
    new = lambda: paella_amd.RequestStream(m, ex_c, ex_u, (4, H, H), max_steps=6, device=DEV)

    def run_until_x(st, slot_x):
        for _ in range(16):
            done = st.tick(graph=graph)
            for b in done:
                if b == slot_x:
                    return st.result(b)
                st.result(b)
        raise AssertionError("X did not finish")

    a = new()
    a.admit(**_request(cfg, 2, seed=1, steps=3))
    a.admit(**_request(cfg, 3, seed=2, steps=4, cfg=3.0))
    assert a.admit(**X) == 2
    a.admit(**_request(cfg, 4, seed=3, steps=6, temperature=(0.7, 0.7)))
    tok_a = run_until_x(a, 2)
    b = new()
    b.admit(**_request(cfg, 7, seed=11, steps=6, cfg=(2.0, 6.0)))
    b.admit(**_request(cfg, 8, seed=12, steps=4, temperature=(1.2, 0.4)))
    assert b.admit(**_request(cfg, 9, seed=13, steps=2)) == 2
    for tick in range(3):
        for s in b.tick(graph=graph):
            assert s == 2 and tick == 1
            b.result(s)
    assert b.free_slots == [2, 3] and b.active == [0, 1]
    assert b.admit(**X) == 2
    tok_b = run_until_x(b, 2)
    torch.cuda.synchronize()
    assert a.captures == 1 and b.captures == 1
    return tok_a, tok_b


def test_admission_time_independence_bit_for_bit(tiny_sd):
    """32x32 tokens: 256 / 64 / 16 rows per sample at UNET_TINY's three levels, so no 16-row block straddles two samples -- the condition of the bit-for-bit
    contract ("Request stream": the folded LayerNorm's guard decides per 16-row block; at 16x16 tokens the deepest level has 4 rows per sample)"""
    tok_a, tok_b = _admission_independence(tiny_sd[0], G.UNET_TINY, 32)
    assert torch.equal(tok_a, tok_b), "request X differs with its admission tick / batch-mates at %d of %d positions" % (int((tok_a != tok_b).sum()), tok_a.numel())


# ---------------------------------------------------------------------------------------------------------------- 6. closed loop
def _lock_step_near_ties(tiny_sd, capsys):
    """the differing tokens the existing lock-step closed-loop test accepts at model near-ties on REQ3 (its own printed summary), and the tokens it compares"""
    RB.test_request_batch_closed_loop_against_oracle_and_model(tiny_sd, "fused")
    out = capsys.readouterr().out
    n = re.search(r"fused: (\d+) differing tokens at model near-ties over (\d+) steps", out)
    assert n, "the lock-step closed-loop test printed no summary"
    return int(n.group(1)), int(n.group(2)) * 3 * 16 * 16


def test_request_stream_closed_loop_against_oracle_and_model(tiny_sd, capsys):
    """B = 3 on UNET_TINY, 16x16: requests of 3, 4 and 6 steps admitted at ticks 0, 0 and 2, the second one with init_x and t_start = 0.6.  At every tick, for
    every running slot: the oracle's UNet on the DEVICE's input tokens plus the model's draw for that request at its OWN step index give the device's tokens,
    except at model near-ties (eps as test_request_batch_closed_loop_against_oracle_and_model); start tokens and renoised rows exact; idle and finished slots
    unchanged across the tick.  The share of differing tokens accepted at near-ties must not exceed twice the share the lock-step closed-loop test accepts on
    REQ3 in this session (same kernels, same model; the factor two covers the other request mix)."""
    m, sd = tiny_sd
    cfg = G.UNET_TINY
    L, B, H = cfg["num_labels"], 3, 16
    hw = H * H
    lock_near, lock_total = _lock_step_near_ties(tiny_sd, capsys)
    g = torch.Generator().manual_seed(21)
    init_x = torch.randint(0, L, (H, H), generator=g)
    conds = [(cond_for(cfg, 1, 3, 1, 30 + b), cond_for(cfg, 1, 3, 1, 40 + b)) for b in range(B)]
    reqs = [dict(seed=REQ3["seeds"][0], steps=3, cfg=3.0, temperature=(1.0, 0.3)),
            dict(seed=REQ3["seeds"][1], steps=4, cfg=8.0, temperature=(0.8, 0.2), init_x=init_x, t_start=0.6, renoise_steps=4),
            dict(seed=REQ3["seeds"][2], steps=6, cfg=(9.0, 5.0), temperature=(0.6, 0.6))]
    admit_at = [0, 0, 2]
    progs = [paella_amd.request_program(**{k: v for k, v in q.items() if k not in ("seed", "init_x")})[0].numpy() for q in reqs]
    st = paella_amd.RequestStream(m, to_dev(conds[0][0], DEV), to_dev(conds[0][1], DEV), (B, H, H), max_steps=6, device=DEV)
    starts, near_total, compared, near_rows = {}, 0, 0, 0
    for tick in range(8):
        for b in range(B):
            if admit_at[b] == tick:
                q = dict(reqs[b])
                if "init_x" in q:
                    q["init_x"] = q["init_x"].to(DEV)
                assert st.admit(to_dev(conds[b][0], DEV), to_dev(conds[b][1], DEV), **q) == b
                starts[b] = C.start_tokens(reqs[b]["seed"], hw, L)
                assert np.array_equal(st.random_x[b].cpu().numpy().reshape(-1), starts[b]), "request %d: start tokens differ from the model" % b
                want0 = reqs[b]["init_x"].numpy().reshape(-1) if "init_x" in reqs[b] else starts[b]
                assert np.array_equal(st.tokens[b].cpu().numpy().reshape(-1), want0), "request %d: the slot does not start from its tokens" % b
        running = {b: st._pos[b] for b in st.active}
        if not running:
            break
        x = st.tokens.clone()
        st.tick()
        torch.cuda.synchronize()
        got = st.tokens.cpu().numpy().reshape(B, hw)
        xc = x.cpu()
        rows = [progs[b][running[b]] if b in running else np.float32([0, 1, 1, 0, -1]) for b in range(B)]
        dev_logits = m._forward_prepared_raw(x, _f32([float(r_[0]) for r_ in rows]), st.cache, req_mix=_f32([[float(r_[2]), float(r_[3])] for r_ in rows]))
        dev_logits = dev_logits.reshape(B, hw, L).cpu().numpy()
        for b in range(B):
            if b not in running:
                assert np.array_equal(got[b], xc[b].numpy().reshape(-1)), "tick %d: idle / finished slot %d changed" % (tick, b)
                continue
            j = running[b]
            r_j, T, cfg_j, omc_j, t_next = (float(v) for v in progs[b][j])
            with torch.no_grad():
                lc = O.unet_forward(sd, cfg, xc[b:b + 1], torch.tensor([r_j]), **conds[b][0]).permute(0, 2, 3, 1).reshape(hw, L).numpy()
                lu = O.unet_forward(sd, cfg, xc[b:b + 1], torch.tensor([r_j]), **conds[b][1]).permute(0, 2, 3, 1).reshape(hw, L).numpy()
            mix = C.mix_logits(lc, lu, cfg_j, omc_j)
            diff = float(np.abs(dev_logits[b].astype(np.float64) - mix).max())
            renoise = t_next >= 0
            pre, final, margin = C.sample_tail(lc, T, reqs[b]["seed"], j, lu=lu, cfg=cfg_j, omc=omc_j, init_noise=starts[b] if renoise else None, t_next=t_next if renoise else 0.0)
            mask = C.renoise_mask(reqs[b]["seed"], hw, j, t_next) if renoise else None
            eps = _near_tie_eps(float(np.abs(C.scaled_logits(mix, T)).max()) + 17.0, diff * float(C.inv_temperature(T)))
            near_total += _compare_tokens("tick %d slot %d step %d (max |oracle - device logit| %.2e)" % (tick, b, j, diff), got[b], pre, final, margin, eps, mask)
            near_rows += int((margin <= eps).sum())
            compared += hw
    assert compared == (3 + 4 + 6) * hw and not st.active
    for b in range(B):
        assert torch.equal(st.result(b).cpu().reshape(-1), torch.from_numpy(got[b]))
    share, lock_share = near_total / compared, lock_near / lock_total
    with capsys.disabled():
        print("\nrequest stream closed loop: %d of %d tokens differ at model near-ties (share %.3e; %d rows sat at a near-tie); lock-step REQ3 in this session: %d of %d "
              "(share %.3e); bound 2 x lock-step = %.3e" % (near_total, compared, share, near_rows, lock_near, lock_total, lock_share, 2 * lock_share))
    # NOTE: the bound is the issue's (twice the lock-step share of the same session).  Both shares measure 0 (profiles/request_stream_parity.txt), so as it stands
    # the assertion is `share <= 0`: one legitimate flip at a model near-tie in the stream run fails it while the lock-step run stays at 0.  The lock-step figure is
    # read from the printed summary of the existing test (it returns nothing); a change of that line's wording fails the regex above, loudly.
    assert share <= 2 * lock_share, "the stream accepts a larger near-tie share (%.3e) than twice the lock-step test's (%.3e)" % (share, lock_share)


# ---------------------------------------------------------------------------------------------------------------- 7. graph and life cycle
MIX10 = [dict(seed=100 + i, steps=s, cfg=c, temperature=t)
         for i, (s, c, t) in enumerate([(3, 8.0, (1.0, 0.2)), (6, 3.0, (0.7, 0.3)), (1, (9.0, 5.0), (0.9, 0.9)), (4, 1.0, (1.0, 0.5)), (2, 7.5, (1.3, 1.0)),
                                        (5, (2.0, 6.0), (0.6, 0.2)), (6, 8.0, (1.0, 0.2)), (3, 4.5, (0.5, 0.5)), (4, 8.0, (0.8, 0.4)), (2, 2.0, (1.0, 0.1))])]


def _drain(st, cfg, graph, H):
    g = torch.Generator().manual_seed(4)
    reqs = []
    for i, q in enumerate(MIX10):
        q = dict(_request(cfg, 60 + i, **q))
        if i == 5:
            q.update(init_x=torch.randint(0, cfg["num_labels"], (H, H), generator=g).to(DEV), t_start=0.5)
        reqs.append(q)
    out = {i: t.clone() for i, t in st.drain(reqs, graph=graph)}
    torch.cuda.synchronize()
    return out


def test_stream_drains_ten_requests_through_three_slots_with_one_capture(tiny_sd):
    m, _ = tiny_sd
    cfg, H = G.UNET_TINY, 32  # (whole 16-row blocks per sample at every level: the second drain below meets other leftovers in the idle slots)
    ex_c, ex_u = _one(cfg, 1)
    new = lambda **k: paella_amd.RequestStream(m, ex_c, ex_u, (3, H, H), max_steps=6, device=DEV, **k)
    st = new()
    got = _drain(st, cfg, True, H)
    assert sorted(got) == list(range(10)) and st.captures == 1 and st.free_slots == [0, 1, 2] and st.active == []
    eager = _drain(new(), cfg, False, H)
    for i in range(10):
        assert torch.equal(got[i], eager[i]), "request %d: the graph ticks differ from the eager tick loop at %d positions" % (i, int((got[i] != eager[i]).sum()))
        assert int(got[i].min()) >= 0 and int(got[i].max()) < cfg["num_labels"]
    assert st.tick() == [] and st.captures == 1
    # a second drain through the same stream: same requests, same slots and ticks -> same tokens, still one capture
    again = _drain(st, cfg, True, H)
    assert all(torch.equal(again[i], got[i]) for i in range(10)) and st.captures == 1


def test_stream_life_cycle_errors_and_staleness(tiny_sd):
    m, sd = tiny_sd
    cfg, H = G.UNET_TINY, 32  # (whole 16-row blocks per sample: a reset stream keeps other leftovers in its idle slot than a fresh one)
    ex_c, ex_u = _one(cfg, 1)
    st = paella_amd.RequestStream(m, ex_c, ex_u, (2, H, H), max_steps=4, device=DEV)
    q = _request(cfg, 5, seed=7, steps=3)
    assert st.admit(**q) == 0 and st.admit(**_request(cfg, 6, seed=8, steps=2)) == 1
    with pytest.raises(RuntimeError, match="no free slot"):
        st.admit(**q)
    with pytest.raises(RuntimeError, match="to run"):
        st.result(0)
    wrong_s = _request(cfg, 5, seed=7, steps=3)
    wrong_s["model_inputs"] = to_dev(cond_for(cfg, 1, 5, 0, 5), DEV)  # 5 ByT5 rows instead of 3
    two = dict(q, model_inputs=to_dev(cond_for(cfg, 2, 3, 0, 5), DEV))   # two requests at once
    img = dict(q, model_inputs=to_dev(cond_for(cfg, 1, 3, 1, 5), DEV))   # a CLIP image the stream's layout has not
    st.tick(), st.tick()
    assert st.active == [0] and st.free_slots == []
    st.result(1)
    for bad in (wrong_s, two, img, dict(q, steps=5), dict(q, cfg=None), dict(q, temperature=(1.0, 0.0)), dict(q, init_x=torch.zeros(H, H + 1, dtype=torch.int64, device=DEV))):
        with pytest.raises(ValueError):
            st.admit(**bad)
    assert st.free_slots == [1]
    # a weight change with a request in flight raises -- its conditioning was prepared with the old weights
    m.load_state_dict({k: v * 1.05 for k, v in sd.items()})
    try:
        with pytest.raises(RuntimeError, match="in flight"):
            st.tick()
        with pytest.raises(RuntimeError, match="in flight"):
            st.admit(**q)
    finally:
        m.load_state_dict(sd)
    # loading the same values back is again a change of the tensors' versions: still in flight, still refused; reset() abandons the request and is the way out
    with pytest.raises(RuntimeError, match="in flight"):
        st.tick()
    with pytest.raises(RuntimeError, match="empty stream"):
        list(st.drain([q]))
    st.reset()
    assert st.free_slots == [0, 1] and st.active == [] and st.tick() == []
    got = dict(st.drain([q]))
    assert st.captures == 2
    fresh = dict(paella_amd.RequestStream(m, ex_c, ex_u, (2, H, H), max_steps=4, device=DEV).drain([q]))
    assert torch.equal(got[0], fresh[0]), "a reset stream differs from a fresh one"
    # idle stream + changed weights: recapture, results equal a fresh stream's
    idle = paella_amd.RequestStream(m, ex_c, ex_u, (2, H, H), max_steps=4, device=DEV)
    strict = paella_amd.RequestStream(m, ex_c, ex_u, (2, H, H), max_steps=4, device=DEV, on_stale="raise")
    m.load_state_dict({k: v * 1.05 for k, v in sd.items()})
    try:
        with pytest.raises(RuntimeError, match="stale"):
            strict.admit(**q)
        got = dict(idle.drain([q]))
        assert idle.captures == 2
        fresh = dict(paella_amd.RequestStream(m, ex_c, ex_u, (2, H, H), max_steps=4, device=DEV).drain([q]))
        assert torch.equal(got[0], fresh[0])
    finally:
        m.load_state_dict(sd)
    with pytest.raises(ValueError):
        paella_amd.RequestStream(m, ex_c, ex_u, (2, H, H), max_steps=4, device=DEV, on_stale="ignore")
    with pytest.raises(TypeError):
        paella_amd.RequestStream(m, ex_c, None, (2, H, H), max_steps=4, device=DEV)


def test_unguided_stream_equals_sample_distributed_words(tiny_sd):
    """an unguided stream of one slot: the whole request equals sample_distributed(cfg=None, latent_shape=(1, H, W), noise="philox") bit for bit (same batch size,
    same kernels up to the tail form), with and without init_x / t_start"""
    m, _ = tiny_sd
    cfg, H = G.UNET_TINY, 16
    c, _u = _one(cfg, 3)
    st = paella_amd.RequestStream(m, c, None, (1, H, H), max_steps=5, guided=False, device=DEV)
    g = torch.Generator().manual_seed(8)
    init_x = torch.randint(0, cfg["num_labels"], (1, H, H), generator=g).to(DEV)
    for kw in (dict(steps=5, temperature=(1.0, 0.2)), dict(steps=3, renoise_steps=3, temperature=(0.7, 0.3), t_start=0.6, t_end=0.1, init_x=init_x)):
        want = paella_amd.sample_distributed(m, c, c, (1, H, H), cfg=None, noise="philox", seed=SEED_HI, **kw)
        q = dict(kw)
        if "init_x" in q:
            q["init_x"] = q["init_x"][0]
        got = dict(st.drain([dict(model_inputs=c, seed=SEED_HI, cfg=None, **q)]))[0]
        assert torch.equal(got, want[0]), "the stream's request differs from sample_distributed at %d positions" % int((got != want[0]).sum())
    assert st.captures == 1


def test_vqgan_stream_image_equals_decode_indices(tiny_sd):
    m, _ = tiny_sd
    cfg, H = G.UNET_TINY, 16
    vc = dict(G.VQ_TINY_F8, codebook_size=cfg["num_labels"])
    vq = paella_amd.VQModel(**vc)
    weights_for(vq, vc["bottleneck_blocks"])
    vq = vq.to(DEV)
    ex_c, ex_u = _one(cfg, 1)
    st = paella_amd.RequestStream(m, ex_c, ex_u, (2, H, H), max_steps=3, device=DEV, vqgan=vq)
    res = list(st.drain([_request(cfg, 5, seed=7, steps=3), _request(cfg, 6, seed=8, steps=2), _request(cfg, 7, seed=9, steps=1)]))
    assert sorted(r[0] for r in res) == [0, 1, 2] and st.captures == 1
    for _, toks, img in res:
        assert torch.equal(img, vq.decode_indices(toks[None])[0])


# ---------------------------------------------------------------------------------------------------------------- 8. one 570M-class check
def test_request_stream_570m(built_lib):
    """configs[1]'s model on its 32x32 grid, B = 4: tokens in range, replay determinism (the same run twice through fresh streams) and admission-time
    independence as test_admission_time_independence_bit_for_bit -- size-independent checks, no oracle"""
    cfg = G.UNET_570M
    m = paella_amd.Paella(**cfg)
    weights_for(m, sum(cfg["blocks"]))
    m = m.to(DEV)
    tok_a, tok_b = _admission_independence(m, cfg, 32)
    assert int(tok_a.min()) >= 0 and int(tok_a.max()) < cfg["num_labels"] and tuple(tok_a.shape) == (32, 32)
    assert torch.equal(tok_a, tok_b), "request X differs with its admission tick / batch-mates at %d of %d positions" % (int((tok_a != tok_b).sum()), tok_a.numel())
    again_a, _ = _admission_independence(m, cfg, 32)
    assert torch.equal(again_a, tok_a), "a second run through fresh streams gives other tokens"
