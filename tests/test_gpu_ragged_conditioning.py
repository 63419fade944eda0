"""GPU: ragged conditioning (ABI 8) -- per-sample conditioning-key counts in the attention kernels, conditioning prepared into slots, and classifier-free
guidance on unequal layouts as ONE 2B-slot forward (sample, graph, shard, request stream).

The two kernel properties (include/paella_hip.h): sample b of a ragged launch equals, bit for bit, the same kernel launched for it alone with Lcond = cond_len[b]
and packed K / V; and rows >= cond_len[b] of a slot are never read (they hold NaN here)."""
import numpy as np
import pytest
import torch

import paella_amd
from oracle import golden_configs as G
from oracle import paella_oracle as O
from paella_amd import _lib, sampling
from paella_amd.modules import CondCache
from tests import counter_noise as C
from tests import test_gpu_counter_noise as CN
from tests.helpers import cond_for, to_dev, weights_for

pytestmark = pytest.mark.gpu
DEV = "cuda"

NHEAD, S_SLOT = 4, 40
COND_LEN = [40, 1, 16, 17, 32, 33]      # one count on each side of the 16-key tile and the 32-key stage boundaries
COND_LEN_KW = [40, 4, 16, 17, 32, 33]   # with key weights (n_kw = 4 must fit every sample's own keys, also with no self keys)
N_KW = 4


def _stream():
    return _lib.stream_ptr(torch.device(DEV))


def _variants(Lq):
    """the dispatch variants paella_test_attention_variant can force at this query count (attention.hip: launch_attention)"""
    if Lq < 64:
        return [0]                 # always the key-split kernel
    if Lq < 256:
        return [0, 20, 21, 22]     # key-split / LDS-staged / register-fed 64-query forms
    return [0, 10, 11, 22]         # LDS staging 0 / 1 instead of the default, or the register-fed kernel


def _attn_inputs(D, Lq, Lself, lens, seed):
    B, ld = len(lens), NHEAD * D
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B * Lq, ld, generator=g).to(DEV)
    ks = torch.randn(B * max(Lself, 1), ld, generator=g).to(DEV)
    vs = torch.randn(B * max(Lself, 1), ld, generator=g).to(DEV)
    kc = torch.randn(B, S_SLOT, ld, generator=g).to(DEV)
    vc = torch.randn(B, S_SLOT, ld, generator=g).to(DEV)
    for b, n in enumerate(lens):      # the padding rows of every slot: never read
        kc[b, n:] = float("nan")
        vc[b, n:] = float("nan")
    kw = (torch.rand(N_KW, generator=g) + 0.5).to(DEV)
    return q, ks, vs, kc, vc, kw, torch.tensor(lens, dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("Lq,Lself", [(16, 16), (64, 64), (64, 0), (256, 256)])
@pytest.mark.parametrize("D", [16, 64, 80])
def test_attention_ragged_is_bit_identical_to_each_sample_alone(built_lib, D, Lq, Lself):
    lib = built_lib
    try:
        for variant in _variants(Lq):
            lib.paella_test_attention_variant(variant)
            for lens, weighted in ((COND_LEN, False), (COND_LEN_KW, True)):
                B, ld = len(lens), NHEAD * D
                q, ks, vs, kc, vc, kw, lens_d = _attn_inputs(D, Lq, Lself, lens, 100 * D + Lq + Lself)
                kwp, nkw = (_lib.ptr(kw), N_KW) if weighted else (None, 0)
                out = torch.full((B * Lq, ld), float("nan"), device=DEV)
                _lib.check(lib.paella_op_attention_ragged(_lib.ptr(q), _lib.ptr(ks) if Lself else None, _lib.ptr(vs) if Lself else None, _lib.ptr(kc), _lib.ptr(vc),
                                                          _lib.ptr(out), B, NHEAD, D, Lq, Lself, S_SLOT, _lib.ptr(lens_d), kwp, nkw, _stream()))
                torch.cuda.synchronize()
                assert torch.isfinite(out).all(), "a padding row (NaN) was read: variant %d, weighted %s" % (variant, weighted)
                for b, n in enumerate(lens):
                    qb = q[b * Lq:(b + 1) * Lq].contiguous()
                    ksb, vsb = ks[b * Lself:(b + 1) * Lself].contiguous(), vs[b * Lself:(b + 1) * Lself].contiguous()
                    kcb, vcb = kc[b, :n].contiguous(), vc[b, :n].contiguous()      # tightly packed
                    ref = torch.empty(Lq, ld, device=DEV)
                    _lib.check(lib.paella_op_attention(_lib.ptr(qb), _lib.ptr(ksb) if Lself else None, _lib.ptr(vsb) if Lself else None, _lib.ptr(kcb), _lib.ptr(vcb),
                                                       _lib.ptr(ref), 1, NHEAD, D, Lq, Lself, n, kwp, nkw, _stream()))
                    torch.cuda.synchronize()
                    assert torch.equal(out[b * Lq:(b + 1) * Lq], ref), "variant %d, sample %d (%d conditioning keys), weighted %s: %d values differ" % (
                        variant, b, n, weighted, int((out[b * Lq:(b + 1) * Lq] != ref).sum()))
    finally:
        lib.paella_test_attention_variant(0)


@pytest.mark.parametrize("D", [64, 80])
def test_attention_bf16_ragged_is_bit_identical_to_each_sample_alone(built_lib, D):
    lib, Lq, Lself = built_lib, 256, 256
    bits = lambda t: t.to(torch.bfloat16).contiguous().view(torch.int16)
    for lens, weighted in ((COND_LEN, False), (COND_LEN_KW, True)):
        B, ld = len(lens), NHEAD * D
        q, ks, vs, kc, vc, kw, lens_d = _attn_inputs(D, Lq, Lself, lens, 7 * D)
        q16, ks16, vs16 = bits(q), bits(ks), bits(vs)
        kwp, nkw = (_lib.ptr(kw), N_KW) if weighted else (None, 0)
        out = torch.full((B * Lq, ld), -1, dtype=torch.int16, device=DEV)
        _lib.check(lib.paella_test_attention_bf16_ragged(_lib.ptr(q16), _lib.ptr(ks16), _lib.ptr(vs16), _lib.ptr(kc), _lib.ptr(vc), _lib.ptr(out), B, NHEAD, D, Lq, Lself,
                                                         S_SLOT, _lib.ptr(lens_d), kwp, nkw, _stream()))
        torch.cuda.synchronize()
        assert torch.isfinite(out.view(torch.bfloat16).float()).all(), "a padding row (NaN) was read"
        for b, n in enumerate(lens):
            sl = slice(b * Lq, (b + 1) * Lq)
            kcb, vcb = kc[b, :n].contiguous(), vc[b, :n].contiguous()
            ref = torch.empty(Lq, ld, dtype=torch.int16, device=DEV)
            _lib.check(lib.paella_test_attention_bf16(_lib.ptr(q16[sl].contiguous()), _lib.ptr(ks16[sl].contiguous()), _lib.ptr(vs16[sl].contiguous()), _lib.ptr(kcb),
                                                      _lib.ptr(vcb), _lib.ptr(ref), 1, NHEAD, D, Lq, Lself, n, kwp, nkw, _stream()))
            torch.cuda.synchronize()
            assert torch.equal(out[sl], ref), "bf16 sample %d (%d conditioning keys), weighted %s: %d values differ" % (b, n, weighted, int((out[sl] != ref).sum()))


# ---------------------------------------------------------------------------------------------------------------- models
def _model(cfg):
    m = paella_amd.Paella(**cfg)
    sd = weights_for(m, sum(cfg["blocks"]))
    return m.to(DEV), sd


@pytest.fixture(scope="module")
def tiny(built_lib):
    return _model(G.UNET_TINY)


def _unequal(cfg, B=2):
    """13 conditioning rows (5 ByT5 + clip + one clip_image) against 6 (2 ByT5 + clip)"""
    return cond_for(cfg, B, 5, 1, G.COND_SEED), cond_for(cfg, B, 2, 0, G.COND_SEED + 5)


def test_cond_prepare_slots(tiny):
    """two groups of different S into one cache pre-filled with a byte pattern: the stored rows are the plain prepare_cond's bit for bit, every other byte is
    untouched, lens as specified; the C entry point's slot0 is exercised directly as well"""
    m, _ = tiny
    cfg, B = G.UNET_TINY, 2
    c, u = (to_dev(x, DEV) for x in _unequal(cfg, B))
    row = m.cond_bytes(1, 1)
    plan = sampling.ragged_slot_plan(13, 6, B, row)
    assert plan["pitch"] == 13 and plan["lens"] == [13, 13, 6, 6]
    guard = plan["slot_bytes"]                     # one more slot behind the cache: must stay untouched
    buf = torch.full((plan["nbytes"] + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    lens = torch.full((2 * B + 1,), -7, dtype=torch.int32, device=DEV)
    half = plan["group_offsets"][1]
    cc = m.prepare_cond(**c, out=buf[:half], slot_rows=13, lens_out=lens[:B])
    cu = m.prepare_cond(**u, out=buf[half:plan["nbytes"]], slot_rows=13, lens_out=lens[B:2 * B])
    assert (cc.B, cc.S, cu.B, cu.S) == (B, 13, B, 13) and cc.lens.data_ptr() == lens.data_ptr()
    pc, pu = m.prepare_cond(**c), m.prepare_cond(**u)
    torch.cuda.synchronize()
    assert lens.tolist() == [13, 13, 6, 6, -7]
    slots = buf[:plan["nbytes"]].view(2 * B, 13, row)
    assert torch.equal(slots[:B], pc.buf.view(B, 13, row))
    assert torch.equal(slots[B:, :6], pu.buf.view(B, 6, row))
    assert bool((slots[B:, 6:] == 0xA5).all()) and bool((buf[plan["nbytes"]:] == 0xA5).all())
    # slot0 through the C ABI: the unconditional group once more, into slots 1 and 2 of a fresh cache
    buf2 = torch.full((plan["nbytes"],), 0x5A, dtype=torch.uint8, device=DEV)
    lens2 = torch.full((2 * B,), -1, dtype=torch.int32, device=DEV)
    byt5, clip, images, arr, Bx, Sb, S = m._cond_args(**u)
    h, lib = m._engine(), _lib.load()
    ws = m.new_workspace(B, 16, 16, 13)
    _lib.check(lib.paella_unet_cond_prepare_slots(h, _lib.ptr(byt5), Sb, _lib.ptr(clip), arr, len(images), Bx, 13, 1, _lib.ptr(buf2), buf2.numel(), _lib.ptr(lens2),
                                                  _lib.ptr(ws), ws.numel(), _stream()))
    torch.cuda.synchronize()
    s2 = buf2.view(2 * B, 13, row)
    assert lens2.tolist() == [-1, 6, 6, -1]
    assert torch.equal(s2[1:3, :6], pu.buf.view(B, 6, row)) and bool((s2[0] == 0x5A).all()) and bool((s2[3] == 0x5A).all()) and bool((s2[1:3, 6:] == 0x5A).all())
    # a group that does not fit its slots is refused
    with pytest.raises(ValueError):
        m.prepare_cond(**c, out=buf[:half], slot_rows=12, lens_out=lens[:B])


# A convex mix: the tolerances of tests/test_gpu_unet.py bound ONE forward against the oracle, and |a e_c + b e_u| <= (a + b) max(|e_c|, |e_u|) = that bound when
# a, b >= 0 and a + b = 1 -- so the per-forward tolerance holds for the mixed logits with no new number.  (The extrapolating guidance pair (8, -7) is what the
# closed-loop sampler test below runs, with the near-tie method of tests/test_gpu_counter_noise.py.)  Both weights are exact in fp32.
MIX = (0.625, 0.375)


@pytest.mark.parametrize("cfg_name,grid,atol", [("UNET_TINY", 32, 2e-5), ("UNET_MID", 16, 3e-4)])  # the tolerances tests/test_gpu_unet.py applies to these models
def test_forward_ragged_against_oracle(built_lib, cfg_name, grid, atol):
    cfg = getattr(G, cfg_name)
    m, sd = _model(cfg)
    B, L = 2, cfg["num_labels"]
    c, u = _unequal(cfg, B)
    cd, ud = to_dev(c, DEV), to_dev(u, DEV)
    g = torch.Generator().manual_seed(3)
    x = torch.randint(0, L, (B, grid, grid), generator=g)
    r = torch.tensor([0.7, 0.3])
    with torch.no_grad():
        ref = O.unet_forward(sd, cfg, x, r, **c).float() * MIX[0] + O.unet_forward(sd, cfg, x, r, **u).float() * MIX[1]
    cache = sampling._prepare_ragged_pair(m, cd, ud, B, None)
    assert cache.B == 2 * B and cache.S == 13 and cache.lens.tolist() == [13, 13, 6, 6]
    got = m.forward_prepared(x.to(DEV), r.to(DEV), cache, cfg_mix=MIX)
    diff = float((got.cpu() - ref).abs().max())
    print("%s ragged 2B forward, mixed logits vs oracle: max |diff| %.3e (bound %.0e)" % (cfg_name, diff, atol))
    assert diff <= atol
    # NaN in the padding rows of the cache changes no bit
    nan = torch.full((cache.buf.numel(),), 0xFF, dtype=torch.uint8, device=DEV)       # every float 0xFFFFFFFF: NaN
    lens = torch.empty(2 * B, dtype=torch.int32, device=DEV)
    half = nan.numel() // 2
    m.prepare_cond(**cd, out=nan[:half], slot_rows=13, lens_out=lens[:B])
    m.prepare_cond(**ud, out=nan[half:], slot_rows=13, lens_out=lens[B:])
    assert bool(torch.isnan(nan.view(torch.float32).view(2 * B, 13, -1)[B:, 6:]).all())
    got_nan = m.forward_prepared(x.to(DEV), r.to(DEV), CondCache(nan, 2 * B, 13, lens), cfg_mix=MIX)
    assert torch.equal(got, got_nan), "NaN padding rows changed %d logits" % int((got != got_nan).sum())
    # all lengths equal to the slot pitch: the ragged entry point is the existing one, bit for bit (mixed, unmixed and the fused tail)
    both = {k: (None if cd[k] is None else torch.cat([cd[k], cd[k].flip(0)])) for k in cd}
    plain = m.prepare_cond(**both)
    full = CondCache(plain.buf, plain.B, plain.S, torch.full((plain.B,), plain.S, dtype=torch.int32, device=DEV))
    xd, rd = x.to(DEV), r.to(DEV)
    assert torch.equal(m.forward_prepared(xd, rd, plain, cfg_mix=MIX), m.forward_prepared(xd, rd, full, cfg_mix=MIX))
    assert torch.equal(m.forward_prepared(xd, rd, plain), m.forward_prepared(xd, rd, full))
    ta, tb = torch.empty_like(xd), torch.empty_like(xd)
    kw = dict(temperature=0.8, seed=77, offset=2, cfg_mix=(8.0, -7.0))
    m.forward_sample(xd, rd, plain, ta, **kw)
    m.forward_sample(xd, rd, full, tb, **kw)
    assert torch.equal(ta, tb)


# ---------------------------------------------------------------------------------------------------------------- sample()
def _count_calls(m, fn):
    """run fn() with forward_sample / forward_prepared of the model counted"""
    n = {"sample": 0, "prepared": 0}
    fs, fp = m.forward_sample, m.forward_prepared

    def cs(*a, **k):
        n["sample"] += 1
        return fs(*a, **k)

    def cp(*a, **k):
        n["prepared"] += 1
        return fp(*a, **k)
    m.forward_sample, m.forward_prepared = cs, cp
    try:
        out = fn()
    finally:
        del m.forward_sample, m.forward_prepared
    return out, n


def test_sample_philox_unequal_layouts_is_one_forward_per_step(tiny):
    """fused == unfused, graph == eager, shard == unsharded, bit for bit; one forward_sample call per step (two forward_prepared calls per step without the
    feature); noise="torch" keeps the two-forward path"""
    m, _ = tiny
    cfg, total, Bs, H = G.UNET_TINY, 4, 2, 16
    c, u = _unequal(cfg, total)
    cs, us = to_dev(c, DEV), to_dev(u, DEV)
    kw = dict(steps=3, renoise_steps=2, temperature=(1.0, 0.3), cfg=8.0)
    run = lambda **x: paella_amd.sample(m, cs, (total, H, H), unconditional_inputs=us, device=DEV, noise="philox", seed=99, **kw, **x)
    full, n = _count_calls(m, run)
    assert n == {"sample": kw["steps"], "prepared": 0}, "forward calls over %d steps: %r (one forward_sample per step expected)" % (kw["steps"], n)
    unf, n = _count_calls(m, lambda: run(fused_tail=False))
    assert n == {"sample": 0, "prepared": kw["steps"]}
    assert torch.equal(full, unf), "fused and two-kernel tails disagree at %d positions" % int((full != unf).sum())
    assert int(full.min()) >= 0 and int(full.max()) < cfg["num_labels"]
    from paella_amd.dist import shard_inputs
    gs = paella_amd.GraphSampler(m, to_dev(shard_inputs(c, 0, Bs), DEV), to_dev(shard_inputs(u, 0, Bs), DEV), (Bs, H, H), device=DEV, **kw)
    for lo in (0, 2):
        ci, ui = to_dev(shard_inputs(c, lo, lo + Bs), DEV), to_dev(shard_inputs(u, lo, lo + Bs), DEV)
        eager = paella_amd.sample(m, ci, (Bs, H, H), unconditional_inputs=ui, device=DEV, noise="philox", seed=99, shard=(lo, total), **kw)
        assert torch.equal(eager, full[lo:lo + Bs]), "shard at row %d differs from the unsharded call at %d positions" % (lo, int((eager != full[lo:lo + Bs]).sum()))
        out = gs(ci, ui, seed=99, shard=(lo, total)).clone()
        assert torch.equal(out, eager), "graph replay differs from the eager call at %d positions" % int((out != eager).sum())
    assert gs.captures == 1
    _, n = _count_calls(m, lambda: paella_amd.sample(m, cs, (total, H, H), unconditional_inputs=us, device=DEV, noise="torch", **kw))
    assert n == {"sample": 0, "prepared": 2 * kw["steps"]}


def test_sample_unequal_layouts_closed_loop_against_oracle(tiny):
    """the method of tests/test_gpu_counter_noise.py (closed loop): at every step the oracle's two forwards on the DEVICE's input tokens and the numpy Philox model's
    draws must give the device's tokens, except where the model's margin is below eps = 2 (max |oracle - device mixed logit| / T + delta) + ulp; counted, printed"""
    m, sd = tiny
    cfg = G.UNET_TINY
    L, B, H = cfg["num_labels"], 2, 16
    seed, steps, renoise_steps = 0xF00DFACE00C0FFEE, 4, 3
    kw = dict(steps=steps, renoise_steps=renoise_steps, temperature=(1.0, 0.3), cfg=8.0)
    c, u = _unequal(cfg, B)
    cs, us = to_dev(c, DEV), to_dev(u, DEV)
    toks, rec = CN._record_sample(m, "fused", cs, us, (B, H, H), seed, None, kw)
    assert len(rec) == steps, "%d forward_sample calls over %d steps" % (len(rec), steps)
    rows = B * H * H
    start = C.start_tokens(seed, rows, L)
    assert np.array_equal(rec[0][0].numpy().reshape(-1), start)
    t_list = [float(v) for v in torch.linspace(1.0, 0.0, steps + 1)]
    temps = [float(v) for v in torch.linspace(1.0, 0.3, steps)]
    pair = (float(torch.tensor(8.0)), float(torch.tensor(1.0 - 8.0)))
    cache = sampling._prepare_ragged_pair(m, cs, us, B, None)
    near_total = 0
    for i in range(steps):
        x_i, got = rec[i]
        if i:
            assert torch.equal(x_i, rec[i - 1][1])
        r = torch.ones(B) * t_list[i]
        with torch.no_grad():
            lc = O.unet_forward(sd, cfg, x_i, r, **c).permute(0, 2, 3, 1).reshape(rows, L).numpy()
            lu = O.unet_forward(sd, cfg, x_i, r, **u).permute(0, 2, 3, 1).reshape(rows, L).numpy()
        dev_logits = m._forward_prepared_raw(x_i.to(DEV), r.to(DEV), cache, cfg_mix=pair).reshape(rows, L).cpu().numpy()
        mix = C.mix_logits(lc, lu, *pair)
        diff = float(np.abs(dev_logits.astype(np.float64) - mix).max())
        renoise = i < renoise_steps
        t_next = t_list[i + 1] if renoise else 0.0
        pre, final, margin = C.sample_tail(lc, temps[i], seed, i, lu=lu, cfg=pair[0], omc=pair[1], init_noise=start if renoise else None, t_next=t_next)
        mask = C.renoise_mask(seed, rows, i, t_next, 0) if renoise else None
        top = float(np.abs(C.scaled_logits(mix, temps[i])).max()) + 17.0
        eps = CN._near_tie_eps(top, diff * float(C.inv_temperature(temps[i])))
        near_total += CN._compare_tokens("ragged step %d (max |oracle - device logit| %.2e)" % (i, diff), got.numpy().reshape(-1), pre, final, margin, eps, mask)
    assert torch.equal(toks.cpu(), rec[-1][1])
    print("ragged closed loop: %d differing tokens at model near-ties over %d steps" % (near_total, steps))


# ---------------------------------------------------------------------------------------------------------------- request stream
STREAM_SHAPE, STEPS = (3, 32, 32), 3


def _request(cfg, n_byt5, n_img, seed):
    """one request: n_byt5 ByT5 rows + clip (+ a CLIP image) against an unconditional side of 1 ByT5 row + clip"""
    return dict(model_inputs=to_dev(cond_for(cfg, 1, n_byt5, n_img, seed), DEV), unconditional_inputs=to_dev(cond_for(cfg, 1, 1, 0, seed + 100), DEV), seed=1000 + seed,
                steps=STEPS, cfg=6.0)


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


def test_request_stream_mixed_lengths(tiny):
    m, _ = tiny
    cfg = G.UNET_TINY
    reqs = [_request(cfg, 3, 0, 1), _request(cfg, 7, 1, 2), _request(cfg, 1, 0, 3)]     # 7, 15 and 5 conditional rows; 5 unconditional rows each
    st = paella_amd.RequestStream(m, reqs[0]["model_inputs"], reqs[0]["unconditional_inputs"], STREAM_SHAPE, max_steps=4, device=DEV, max_cond_rows=16)
    assert st.cache.S == 16 and st.cache.lens.tolist() == [16] * 6
    idle = lambda i: dict(_request(cfg, 2 + i, 0, 50 + i), steps=1)      # finishes with the first tick and keeps its slot (never collected): an idle mate
    alone = []
    for i, q in enumerate(reqs):
        others = [reqs[j] for j in range(3) if j != i]
        a = _serve(st, [idle(0), idle(1)], q, 1)                                        # slot 2, nobody else running
        lens = st.cache.lens.tolist()
        assert lens[2] == sampling._cond_seq_len(m, q["model_inputs"]) and lens[5] == 5
        b = _serve(st, others, q, 0)                                                    # slot 2, two running mates of other lengths, joined together
        d = _serve(st, [dict(o, steps=4) for o in others], q, 2)                        # slot 2, joins two ticks after its mates
        assert torch.equal(a, b), "request %d: tokens depend on its batch-mates (%d positions)" % (i, int((a != b).sum()))
        assert torch.equal(a, d), "request %d: tokens depend on the tick it joined at (%d positions)" % (i, int((a != d).sum()))
        assert int(a.min()) >= 0 and int(a.max()) < cfg["num_labels"]
        alone.append(a)
    assert not torch.equal(alone[0], alone[1])
    # request 2's two sides share a layout (1 ByT5 row + clip): a strict stream built on exactly that layout, same B and slot
    q = reqs[2]
    strict = paella_amd.RequestStream(m, q["model_inputs"], q["unconditional_inputs"], STREAM_SHAPE, max_steps=4, device=DEV)
    assert strict.cache.lens is None and strict.S == 5
    same = lambda i: dict(_request(cfg, 1, 0, 60 + i), steps=1)
    s = _serve(strict, [same(0), same(1)], q, 1)
    assert torch.equal(s, alone[2]), "ragged stream differs from the strict stream on the same layout at %d positions" % int((s != alone[2]).sum())
    # rows above max_cond_rows (13 ByT5 + clip = 17) are refused; so are 0 rows and two requests at once
    st.reset()
    with pytest.raises(ValueError, match="max_cond_rows"):
        st.admit(**_request(cfg, 13, 0, 9))
    with pytest.raises(ValueError, match="max_cond_rows"):
        st.admit(**dict(reqs[0], unconditional_inputs=to_dev(cond_for(cfg, 1, 9, 1, 9), DEV)))
    with pytest.raises(ValueError):
        st.admit(**dict(reqs[0], model_inputs=to_dev(cond_for(cfg, 2, 3, 0, 9), DEV)))
    with pytest.raises(ValueError, match="attn_weights"):
        paella_amd.RequestStream(m, q["model_inputs"], q["unconditional_inputs"], STREAM_SHAPE, max_steps=4, device=DEV, max_cond_rows=16,
                                 attn_weights=torch.ones(66, device=DEV))
