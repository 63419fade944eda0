"""GPU: editing requests in the request stream -- the pin of the sampling tail (scalar and stream forms, fused and unfused), the pin policy of
request_step_kernel, `inpaint(pin="step")` / `GraphInpainter(pin="step")` and `RequestStream(editing=True)`.  Every comparison is between identical arithmetic
and therefore exact: no tolerance anywhere in this file."""
import numpy as np
import pytest
import torch

import paella_amd
from oracle import golden_configs as G
from paella_amd import _lib, editing, sampling
from tests import counter_noise as C
from tests.helpers import cond_for, to_dev, weights_for
from tests.test_gpu_counter_noise import HEAD_8K, SEED_HI, _cfg_logits, _compare_tokens, _near_tie_eps, _stream, _tail_ex, _word
from tests.test_gpu_request_batch import SEEDS5, _conds, _tables, head8k, tiny_sd  # noqa: F401  (fixtures)
from tests.test_gpu_request_stream import SENTINEL, _f32, _i32, _one, _request, _tail_stream
from tests.test_request_edit import request_step_pin_model

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _tail_stream_pin(lc, lu, L, hw, pairs, temps, seeds, step, t_next, active, init, keep, known, pin_on, out, sampled=None):
    _lib.check(_lib.load().paella_sample_tail_stream_pin(_lib.ptr(lc), _lib.ptr(lu), lc.size(0), L, _lib.ptr(pairs), _lib.ptr(temps), _lib.ptr(seeds), hw, _lib.ptr(step),
                                                         _lib.ptr(t_next), _lib.ptr(active), _lib.ptr(init), _lib.ptr(keep), _lib.ptr(known), _lib.ptr(pin_on), _lib.ptr(out),
                                                         _lib.ptr(sampled), _stream()))
    torch.cuda.synchronize()


def _keep_grid(B, hw, seed, zero=0, one=2):
    """per slot a 0/1 mask over its hw rows: slot `zero` all known, slot `one` all regenerate, the others about half and half"""
    g = torch.Generator().manual_seed(seed)
    keep = torch.randint(0, 2, (B, hw), generator=g)
    keep[zero], keep[one] = 0, 1
    return keep


# ---------------------------------------------------------------------------------------------------------------- 1. the step kernel
def test_request_step_pin_kernel_against_its_model(built_lib):
    B, max_steps = 5, 4
    rng = np.random.default_rng(3)
    program = rng.standard_normal((B, max_steps, 5)).astype(np.float32)
    pos, length = np.int32([0, 0, 1, 0, 2]), np.int32([1, 4, 3, 0, 2])  # lengths 1 and max_steps, one mid-flight, an idle slot, a cursor already at its length
    policy = np.int32([2, 1, 2, 1, 1])
    d = lambda a: torch.from_numpy(a.copy()).to(DEV)
    d_prog, d_pos, d_len, d_pol = d(program), d(pos), d(length), d(policy)
    d_r, d_t, d_tn = (torch.full((B,), 99.0, device=DEV) for _ in range(3))
    d_pairs, d_step, d_act, d_on = torch.full((B, 2), 99.0, device=DEV), _i32([-1] * B), _i32([-1] * B), _i32([-1] * B)
    seen = []
    for tick in range(6):
        if tick == 3:  # slot 0 is reused by a request of max_steps steps under the other policy, slot 3 gets a one-step request under "final"
            length[0], pos[0], policy[0], length[3], pos[3], policy[3] = 4, 0, 1, 1, 0, 2
            d_pos.copy_(d(pos)), d_len.copy_(d(length)), d_pol.copy_(d(policy))
        # a null policy table: exactly the tables (and cursors) of paella_request_step on the same state
        p0, p1 = d_pos.clone(), d_pos.clone()
        o0 = [torch.full_like(t, 55) for t in (d_r, d_t, d_pairs, d_tn, d_step, d_act)]
        o1 = [torch.full_like(t, 55) for t in (d_r, d_t, d_pairs, d_tn, d_step, d_act)]
        _lib.check(built_lib.paella_request_step(_lib.ptr(d_prog), max_steps, _lib.ptr(p0), _lib.ptr(d_len), B, *(_lib.ptr(t) for t in o0), _stream()))
        _lib.check(built_lib.paella_request_step_pin(_lib.ptr(d_prog), max_steps, _lib.ptr(p1), _lib.ptr(d_len), B, *(_lib.ptr(t) for t in o1), None, None, _stream()))
        torch.cuda.synchronize()
        assert torch.equal(p0, p1) and all(torch.equal(a, b) for a, b in zip(o0, o1))
        want = request_step_pin_model(program, pos, length, policy)
        _lib.check(built_lib.paella_request_step_pin(_lib.ptr(d_prog), max_steps, _lib.ptr(d_pos), _lib.ptr(d_len), B, _lib.ptr(d_r), _lib.ptr(d_t), _lib.ptr(d_pairs),
                                                     _lib.ptr(d_tn), _lib.ptr(d_step), _lib.ptr(d_act), _lib.ptr(d_pol), _lib.ptr(d_on), _stream()))
        torch.cuda.synchronize()
        for name, g_, w_ in zip(("r", "temperature", "pairs", "t_next", "step", "active", "pin_on"), (d_r, d_t, d_pairs, d_tn, d_step, d_act, d_on), want):
            assert np.array_equal(g_.cpu().numpy(), w_), "tick %d: %s differs from the model" % (tick, name)
        assert np.array_equal(d_pos.cpu().numpy(), pos) and torch.equal(p0, d_pos), "tick %d: cursors differ" % tick
        seen.append(want[6].tolist())
    assert seen[0] == [1, 1, 0, 0, 0] and seen[1] == [0, 1, 1, 0, 0] and seen[3] == [1, 1, 0, 1, 0] and seen[5] == [1, 0, 0, 0, 0], seen


# ---------------------------------------------------------------------------------------------------------------- 2. the stream tail on materialised logits
@pytest.mark.parametrize("L,guided,model", [(12, True, True), (12, False, False), (8192, True, False), (8192, False, False)], ids=lambda v: str(v))
def test_stream_tail_pin(built_lib, L, guided, model):
    B, hw, i = 5, 32, 1
    rows = B * hw
    seeds = SEEDS5
    req = _tables(B, 3, seeds, [3.0, 8.0, (9.0, 5.0), 1.0, 7.5] if guided else None, [(1.0, 0.2), (0.7, 0.3), (0.9, 0.9), (0.05, 0.4), (1.3, 1.0)])
    lc, lu = _cfg_logits(rows, L, L + hw)
    g = torch.Generator().manual_seed(5)
    init = torch.randint(0, L, (rows,), generator=g).to(DEV)
    known_h = torch.randint(0, L, (rows,), generator=g)
    keep_h = _keep_grid(B, hw, 11).reshape(-1)
    known, keep = known_h.to(DEV), keep_h.to(DEV)
    lcd, lud = lc.to(DEV), (lu.to(DEV) if guided else None)
    pairs = req.pairs[i] if guided else None
    step_b, t_b, act_b, on_b = [3, 0, 7, 1, 2], [0.45, -1.0, 0.9, 0.05, 0.3], [1, 1, 1, 0, 1], [1, 0, 1, 1, 1]  # slot 3 is inactive although its pin_on is 1
    step, t_next, active, pin_on = _i32(step_b), _f32(t_b), _i32(act_b), _i32(on_b)
    new = lambda: torch.full((rows,), SENTINEL, dtype=torch.int64, device=DEV)
    base, base_pre, got, got_pre, null, null_pre = new(), new(), new(), new(), new(), new()
    _tail_stream(lcd, lud, L, hw, pairs, req.temps[i], req.seeds, step, t_next, active, init, base, base_pre)
    _tail_stream_pin(lcd, lud, L, hw, pairs, req.temps[i], req.seeds, step, t_next, active, init, keep, known, pin_on, got, got_pre)
    _tail_stream_pin(lcd, lud, L, hw, pairs, req.temps[i], req.seeds, step, t_next, active, init, None, None, None, null, null_pre)
    assert torch.equal(null, base) and torch.equal(null_pre, base_pre), "null pin tables are not the unpinned stream tail"
    slot = torch.arange(rows, device=DEV) // hw
    pinned = (pin_on[slot] != 0) & (active[slot] != 0) & (keep == 0)
    assert torch.equal(got, torch.where(pinned, known, base)), "pinned tokens differ from the unpinned tail + where at %d rows" % int((got != torch.where(pinned, known, base)).sum())
    assert torch.equal(got_pre, base_pre), "sampled_out is not the raw draw"
    assert bool((got[3 * hw:4 * hw] == SENTINEL).all()) and bool((got_pre[3 * hw:4 * hw] == SENTINEL).all()), "the inactive slot's rows were written"
    assert torch.equal(got[:hw], known[:hw]) and torch.equal(got[2 * hw:3 * hw], base[2 * hw:3 * hw]) and torch.equal(got[hw:2 * hw], base[hw:2 * hw])
    assert 0 < int(pinned[4 * hw:].sum()) < hw
    # a null pin_on with the row tables: the pin applies to every (active) slot
    allp = new()
    _tail_stream_pin(lcd, lud, L, hw, pairs, req.temps[i], req.seeds, step, t_next, active, init, keep, known, None, allp)
    assert torch.equal(allp, torch.where((active[slot] != 0) & (keep == 0), known, base))
    if model:  # the numpy model of the counter-based tail, per request at its own step, plus the same where
        temps, pairs_h = req.temps.cpu(), req.pairs.cpu()
        for b in range(B):
            if not act_b[b]:
                continue
            sl = slice(b * hw, (b + 1) * hw)
            cfg, omc, T = float(pairs_h[i, b, 0]), float(pairs_h[i, b, 1]), float(temps[i, b])
            renoise = t_b[b] >= 0
            mp, mf, margin = C.sample_tail(lc[sl].numpy(), T, seeds[b], step_b[b], lu=lu[sl].numpy(), cfg=cfg, omc=omc, init_noise=init[sl].cpu().numpy() if renoise else None,
                                           t_next=t_b[b] if renoise else 0.0)
            mask = C.renoise_mask(seeds[b], hw, step_b[b], t_b[b]) if renoise else None
            top = float(np.abs(C.scaled_logits(C.mix_logits(lc[sl].numpy(), lu[sl].numpy(), cfg, omc), T)).max()) + 17.0
            dev_pre = got_pre[sl].cpu().numpy()
            unpinned = np.where(mask, mf, dev_pre) if mask is not None else dev_pre
            _compare_tokens("pinned stream tail, request %d" % b, unpinned, mp, mf, margin, _near_tie_eps(top), mask, dev_pre)
            want = np.where((keep_h[sl].numpy() == 0) & bool(on_b[b]), known_h[sl].numpy(), unpinned)
            assert np.array_equal(got[sl].cpu().numpy(), want), "request %d: pinned tokens differ from the model + where" % b


# ---------------------------------------------------------------------------------------------------------------- 3. the scalar tail
@pytest.mark.parametrize("L,guided", [(12, True), (8192, False)], ids=lambda v: str(v))
def test_scalar_tail_pin(built_lib, L, guided):
    rows = 3 * 32 + 5  # not a multiple of anything the kernels tile by
    lc, lu = _cfg_logits(rows, L, L + 1)
    g = torch.Generator().manual_seed(6)
    init, known, keep = (torch.randint(0, n, (rows,), generator=g).to(DEV) for n in (L, L, 2))
    lcd, lud = lc.to(DEV), (lu.to(DEV) if guided else None)
    cfg, omc = (float(torch.tensor(3.5)), float(torch.tensor(1.0 - 3.5))) if guided else (1.0, 0.0)
    seed_word, row_off, row_word = (1 << 64) - 9, 7, (1 << 21) + 3
    base, base_pre, got, got_pre, null = (torch.full((rows,), SENTINEL, dtype=torch.int64, device=DEV) for _ in range(5))
    _tail_ex(lcd, lud, L, cfg, omc, 0.6, 0, SEED_HI, 4, base, base_pre, seed_word=seed_word, row_offset=row_off, row_word=row_word, init=init, t_next=0.4)
    sw, rw = _word(seed_word), _word(row_word)
    call = lambda k, t, out, pre: _lib.check(built_lib.paella_sample_tail_pin(_lib.ptr(lcd), _lib.ptr(lud), rows, L, cfg, omc, 0.6, 0, SEED_HI, _lib.ptr(sw), 4, row_off,
                                                                              _lib.ptr(rw), _lib.ptr(init), 0.4, _lib.ptr(k), _lib.ptr(t), _lib.ptr(out), _lib.ptr(pre), _stream()))
    call(keep, known, got, got_pre)
    call(None, None, null, None)
    torch.cuda.synchronize()
    assert torch.equal(null, base), "null pin tables are not the unpinned scalar tail"
    assert torch.equal(got, torch.where(keep == 0, known, base)) and torch.equal(got_pre, base_pre)
    assert 0 < int((keep == 0).sum()) < rows and not torch.equal(got, base)


# ---------------------------------------------------------------------------------------------------------------- 4. fused == unfused
def _fused_vs_unfused_pin(m, cfg, B, H, W, what, guided=True, ragged=False):
    L, hw = cfg["num_labels"], H * W
    rows = B * hw
    seeds = (SEEDS5 * 2)[:B]
    req = _tables(B, 3, seeds, ([3.0, 8.0, (9.0, 5.0), 1.0] * 2)[:B] if guided else None, ([(1.0, 0.2), (0.7, 0.3), (0.4, 0.9), (1.2, 1.0)] * 2)[:B])
    if ragged:  # unequal conditioning lengths on the two sides: 7 + clip against 1 + clip rows
        cs, us = to_dev(cond_for(cfg, B, 7, 0, 1), DEV), to_dev(cond_for(cfg, B, 1, 0, 2), DEV)
        cache = sampling._prepare_ragged_pair(m, cs, us, B, None)
        assert cache.lens is not None and len(set(cache.lens.tolist())) == 2
    else:
        cs, us = _conds(cfg, B)
        both = {k: (torch.cat([cs[k], us[k]]) if cs[k] is not None else None) for k in cs}
        cache = m.prepare_cond(**(both if guided else cs))
    g = torch.Generator().manual_seed(9)
    x = torch.randint(0, L, (B, H, W), generator=g).to(DEV)
    init = torch.randint(0, L, (B, H, W), generator=g).to(DEV)
    known = torch.randint(0, L, (B, H, W), generator=g).to(DEV)
    keep = _keep_grid(B, hw, 12, zero=0, one=B - 1).reshape(B, H, W).to(DEV)
    r = _f32([0.6, 0.3, 0.9, 0.1, 0.5, 0.7][:B])
    step = _i32([5, 0, 2, 9, 1, 3][:B])
    t_next = _f32([0.55, -1.0, 0.2, 0.8, -1.0, 0.4][:B])
    active = _i32([1, 0, 1, 1, 1, 1][:B])        # slot 1 is inactive
    pin_on = _i32([1, 1, 0, 1, 0, 1][:B])        # mixed; the inactive slot's flag is set
    fused = torch.full((B, H, W), SENTINEL, dtype=torch.int64, device=DEV)
    unfused, plain = fused.clone(), fused.clone()
    row = 1
    m.forward_sample(x, r, cache, fused, temperature=1.0, init_noise=init, req=req.step(row), stream=(step, t_next, active), pin=(keep, known, pin_on))
    m.forward_sample(x, r, cache, plain, temperature=1.0, init_noise=init, req=req.step(row), stream=(step, t_next, active))
    logits = m._forward_prepared_raw(x, r, cache, req_mix=req.pairs[row]) if guided else m._forward_prepared_raw(x, r, cache)
    _tail_stream_pin(logits.reshape(rows, L), None, L, hw, None, req.temps[row], req.seeds, step, t_next, active, init.view(-1), keep.view(-1), known.view(-1), pin_on,
                     unfused.view(-1))
    assert torch.equal(fused, unfused), "%s: fused pinned step differs from forward_shared_req + the pinned stream tail at %d positions" % (what, int((fused != unfused).sum()))
    slot_on = ((pin_on != 0) & (active != 0))[:, None, None]
    assert torch.equal(fused, torch.where(slot_on & (keep == 0), known, plain)), "%s: the pinned step is not the unpinned step + where" % what
    assert bool((fused[1] == SENTINEL).all()) and torch.equal(fused[0], known[0]) and not torch.equal(fused, plain)


@pytest.mark.parametrize("grid", [(4, 8, 8), (3, 24, 8), (2, 16, 16)], ids=lambda g: "%dx%dx%d" % g)
def test_fused_pinned_stream_step_tiny(tiny_sd, grid):
    _fused_vs_unfused_pin(tiny_sd[0], G.UNET_TINY, grid[0], grid[1], grid[2], "UNET_TINY %s" % (grid,))
    _fused_vs_unfused_pin(tiny_sd[0], G.UNET_TINY, grid[0], grid[1], grid[2], "UNET_TINY %s unguided" % (grid,), guided=False)


def test_fused_pinned_stream_step_ragged(tiny_sd):
    _fused_vs_unfused_pin(tiny_sd[0], G.UNET_TINY, 3, 24, 8, "UNET_TINY ragged", ragged=True)


@pytest.mark.parametrize("tile", [9, 14, 18])
def test_fused_pinned_stream_step_large_head(built_lib, head8k, tile):
    built_lib.paella_test_gemm_tail_tile(tile)
    try:
        _fused_vs_unfused_pin(head8k, HEAD_8K, 2, 32, 32, "8192-label head, tile %d" % tile)
        _fused_vs_unfused_pin(head8k, HEAD_8K, 6, 24, 8, "8192-label head, tile %d, 24x8" % tile)
    finally:
        built_lib.paella_test_gemm_tail_tile(18)


# ---------------------------------------------------------------------------------------------------------------- 5. eager and captured pin="step"
@pytest.fixture(scope="module")
def tiny_vq(built_lib):
    vc = dict(G.VQ_TINY_F8, codebook_size=G.UNET_TINY["num_labels"])
    vq = paella_amd.VQModel(**vc)
    weights_for(vq, vc["bottleneck_blocks"])
    return vq.to(DEV)


def _edit_loop(m, vq, img, mask, cs, us, seed, steps, t_start, temperature=(0.7, 0.3), cfg=(8.0, 8.0), every_step=True, check_pin=False):
    """inpaint(noise="philox") written out from public pieces, one unpinned forward_sample per step; every_step: select_tokens(out, known, mask) after each one.
    Returns (tokens before any final select, known, the tokens after every step)."""
    L = m.num_labels
    known = vq.encode(img)[2]
    shape = tuple(known.shape)
    B = shape[0]
    mask = mask.to(DEV)
    noised, _ = m.add_noise(known, torch.full((B,), float(t_start), device=DEV), mask=mask, random_x=editing._philox_random_x(m, shape, seed, DEV))
    init = sampling.start_tokens(L, shape, seed, DEV)
    cache = m.prepare_cond(**{k: (torch.cat([cs[k], us[k]]) if cs[k] is not None else None) for k in cs})
    t_list = sampling.linspace_schedule(t_start, 0.0, steps + 1)
    temps = sampling.linspace_schedule(temperature[0], temperature[1], steps)
    sched = torch.linspace(cfg[0], cfg[1], steps)
    r_all = sampling.timestep_table(t_list, steps, B, DEV)
    x, trace = noised, []
    for i in range(steps):
        renoise = i < steps - 1
        kw = dict(temperature=temps[i], seed=seed, offset=i, init_noise=init if renoise else None, t_next=t_list[i + 1] if renoise else 0.0,
                  cfg_mix=(float(sched[i]), float(1 - sched[i])))
        out = m.forward_sample(x, r_all[i], cache, torch.empty_like(x), **kw)
        if every_step:
            out = paella_amd.select_tokens(out, known, mask)
            if check_pin:  # the same step through the pinned scalar entry point
                pinned = m.forward_sample(x, r_all[i], cache, torch.empty_like(x), pin=(mask, known), **kw)
                assert torch.equal(pinned, out), "step %d: forward_sample(pin=) differs from forward_sample + select_tokens" % i
            assert torch.equal(out[mask == 0], known[mask == 0]), "step %d: a known position does not hold its token" % i
        trace.append(out)
        x = out
    return x, known, trace


def test_inpaint_pin_step_eager_and_captured(tiny_sd, tiny_vq):
    m, vq, cfg = tiny_sd[0], tiny_vq, G.UNET_TINY
    g = torch.Generator().manual_seed(4)
    B, H, W, steps, t_start = 2, 8, 16, 4, 0.7
    img = torch.rand(B, 3, H * 8, W * 8, generator=g).to(DEV)
    mask = torch.zeros(B, H, W, dtype=torch.int64)
    mask[:, 2:6, 3:13] = 1
    cs, us = to_dev(cond_for(cfg, B, 3, 0, 1), DEV), to_dev(cond_for(cfg, B, 3, 0, 2), DEV)
    kw = dict(steps=steps, t_start=t_start, noise="philox", decode=False)
    want, known, _ = _edit_loop(m, vq, img, mask, cs, us, 21, steps, t_start, check_pin=True)
    got, _ = paella_amd.inpaint(m, vq, img, mask, cs, us, pin="step", seed=21, **kw)
    assert torch.equal(got, want), "inpaint(pin='step') differs from the per-step select loop at %d positions" % int((got != want).sum())
    unfused, _ = paella_amd.inpaint(m, vq, img, mask, cs, us, pin="step", seed=21, fused_tail=False, **kw)
    assert torch.equal(unfused, want), "the unfused pinned tail differs"
    # pin="final" is the recipe as it was: the unpinned loop, the known tokens re-imposed once
    free, _, _ = _edit_loop(m, vq, img, mask, cs, us, 21, steps, t_start, every_step=False)
    final, _ = paella_amd.inpaint(m, vq, img, mask, cs, us, pin="final", seed=21, **kw)
    assert torch.equal(final, paella_amd.select_tokens(free, known, mask.to(DEV))) and torch.equal(final, paella_amd.inpaint(m, vq, img, mask, cs, us, seed=21, **kw)[0])
    assert not torch.equal(final, got), "pinning every step changed nothing: the case is vacuous"
    loose, _ = paella_amd.inpaint(m, vq, img, mask, cs, us, keep_known=False, seed=21, **kw)
    assert torch.equal(loose, free)
    with pytest.raises(ValueError, match="philox"):
        paella_amd.inpaint(m, vq, img, mask, cs, us, pin="step", steps=steps, t_start=t_start)
    # captured
    gi = paella_amd.GraphInpainter(m, vq, img, mask, cs, us, steps=steps, t_start=t_start, device=DEV, pin="step")
    gt, go = gi(img, mask, cs, us, seed=21)
    assert torch.equal(gt, want) and torch.equal(go, vq.decode_indices(want))
    img2 = torch.rand(B, 3, H * 8, W * 8, generator=g).to(DEV)
    mask2 = torch.zeros_like(mask)
    mask2[:, :, :5] = 1
    want2, _ = paella_amd.inpaint(m, vq, img2, mask2, cs, us, pin="step", seed=22, **kw)
    gt, _ = gi(img2, mask2, cs, us, seed=22)
    assert torch.equal(gt, want2) and gi.captures == 1
    assert torch.equal(want2[mask2.to(DEV) == 0], vq.encode(img2)[2][mask2.to(DEV) == 0])


# ---------------------------------------------------------------------------------------------------------------- 6. the stream end to end
H6, STEPS6, T0 = 32, 4, 0.7   # 32 x 32 tokens: whole 16-row blocks per sample at every level, the condition of the bit-for-bit contract (as the existing stream tests)
KW6 = dict(steps=STEPS6, temperature=(0.7, 0.3), cfg=(8.0, 8.0), t_start=T0)


@pytest.fixture(scope="module")
def edit_case(tiny_sd, tiny_vq):
    """one image, its tokens and a mask; and proof, on the eager unpinned path, that the first step rewrites known positions (so "final differs mid-flight" can hold)"""
    m, vq, cfg = tiny_sd[0], tiny_vq, G.UNET_TINY
    g = torch.Generator().manual_seed(31)
    img = torch.rand(3, H6 * 8, H6 * 8, generator=g).to(DEV)
    mask = torch.zeros(H6, H6, dtype=torch.int64)
    mask[8:24, 4:20] = 1
    mask = mask.to(DEV)
    known = vq.encode(img[None])[2][0]
    c, u = _one(cfg, 50)
    _, _, trace = _edit_loop(m, vq, img[None], mask[None], c, u, SEED_HI, STEPS6, T0, every_step=False)
    assert bool((trace[0][0] != known)[mask == 0].any()), "the unpinned run keeps every known token after its first step: pick another seed / mask"
    return dict(img=img, mask=mask, known=known, c=c, u=u, seed=SEED_HI)


def _edit_stream(m, cfg, B, vq=None, editing=True, **kw):
    ex_c, ex_u = _one(cfg, 1)
    return paella_amd.RequestStream(m, ex_c, ex_u, (B, H6, H6), max_steps=6, device=DEV, vqgan=vq, editing=editing, **kw)


def _run_slot(st, slot, graph=True, watch=None):
    for _ in range(16):
        done = st.tick(graph=graph)
        if watch is not None:
            watch(st)
        for b in done:
            res = st.result(b)
            if b == slot:
                return res
    raise AssertionError("the request did not finish")


def _xreq(case, pin, **over):
    return dict(dict(model_inputs=case["c"], unconditional_inputs=case["u"], seed=case["seed"], known=case["known"], mask=case["mask"], pin=pin, **KW6), **over)


@pytest.mark.parametrize("pin", ["final", "step"])
def test_stream_editing_request_equals_inpaint(tiny_sd, tiny_vq, edit_case, pin):
    """(a), (b): a stream of ONE slot runs the batch the eager recipe runs at batch 1, so its editing request is `inpaint` bit for bit.  In a larger stream the logits
    of a request may differ in their last bits (the GEMMs split their work by tile index: the request-batch contract), which is why this comparison
    is made at B = 1; (d) below holds the B = 3 stream to the stream's own contract."""
    m, vq, case = tiny_sd[0], tiny_vq, edit_case
    want, _ = paella_amd.inpaint(m, vq, case["img"][None], case["mask"][None], case["c"], case["u"], keep_known=True, noise="philox", seed=case["seed"], decode=False,
                                 pin=pin, **{k: KW6[k] for k in ("steps", "temperature", "cfg", "t_start")})
    st = _edit_stream(m, G.UNET_TINY, 1)
    slot = st.admit(**_xreq(case, pin))
    got = _run_slot(st, slot)
    assert torch.equal(got, want[0]), "pin=%s: the stream's editing request differs from inpaint at %d positions" % (pin, int((got != want[0]).sum()))
    assert torch.equal(got[case["mask"] == 0], case["known"][case["mask"] == 0]) and st.captures == 1


def test_stream_editing_independence_policies_and_one_capture(tiny_sd, tiny_vq, edit_case):
    """(c) - (g) on one B = 3 editing stream and one plain stream"""
    m, cfg, case = tiny_sd[0], G.UNET_TINY, edit_case
    st = _edit_stream(m, cfg, 3)
    known, keep0 = case["known"], case["mask"] == 0
    # (c) a plain request in an editing stream == the same request in a non-editing stream (same slot, alone)
    plain = _request(cfg, 60, seed=5, steps=3, cfg=3.0)
    a = _run_slot(st, st.admit(**plain))
    b_st = _edit_stream(m, cfg, 3, editing=False)
    b = _run_slot(b_st, b_st.admit(**plain))
    assert torch.equal(a, b), "a plain request differs between an editing and a non-editing stream at %d positions" % int((a != b).sum())
    assert st.keep is not None and b_st.keep is None and bool((st.keep == 1).all())
    idle = lambda i: _request(cfg, 70 + i, seed=40 + i, steps=1)
    alone = {}
    for pin in ("step", "final"):
        # (d)/(f): alone in slot 2 (two finished, uncollected one-step requests hold slots 0 and 1), watched after every tick
        st.reset()
        st.admit(**idle(0)), st.admit(**idle(1))
        st.tick()
        slot = st.admit(**_xreq(case, pin))
        assert slot == 2
        kept = []
        alone[pin] = _run_slot(st, slot, watch=lambda s: kept.append(bool((s.tokens[2][keep0] == known[keep0]).all())))
        assert len(kept) == STEPS6 and kept[-1], "pin=%s: a known position differs at the end" % pin
        assert all(kept) if pin == "step" else not all(kept[:-1]), "pin=%s: known positions after each tick: %s" % (pin, kept)
        # (e) the same ticks launched eagerly
        st.reset()
        st.admit(**idle(0)), st.admit(**idle(1))
        st.tick(graph=False)
        assert torch.equal(_run_slot(st, st.admit(**_xreq(case, pin)), graph=False), alone[pin]), "pin=%s: eager ticks differ from the graph replay" % pin
        # (d) admitted two ticks later, next to a running text-to-image request and a running editing request of the OTHER policy and another step count
        other = "final" if pin == "step" else "step"
        g = torch.Generator().manual_seed(77)
        mate_mask = (torch.rand(H6, H6, generator=g) < 0.5).to(DEV)
        st.reset()
        st.admit(**_request(cfg, 61, seed=6, steps=6, cfg=(2.0, 6.0)))
        st.admit(**_xreq(case, other, seed=99, steps=5, mask=mate_mask, known=torch.randint(0, cfg["num_labels"], (H6, H6), generator=g).to(DEV)))
        st.tick(), st.tick()
        assert st.active == [0, 1] and st.admit(**_xreq(case, pin)) == 2
        late = _run_slot(st, 2)
        assert torch.equal(late, alone[pin]), "pin=%s: the editing request depends on its batch-mates / admission tick at %d positions" % (pin, int((late != alone[pin]).sum()))
    assert not torch.equal(alone["step"], alone["final"])
    assert st.captures == 1 and b_st.captures == 1  # (g)
    st.reset()
    assert st.pin_policy.tolist() == [0, 0, 0]


def test_stream_admit_image_and_decoded_result(tiny_sd, tiny_vq, edit_case):
    """(h)"""
    m, vq, case = tiny_sd[0], tiny_vq, edit_case
    st = _edit_stream(m, G.UNET_TINY, 2, vq=vq)
    q = _xreq(case, "step", steps=2)
    toks_k, img_k = _run_slot(st, st.admit(**q))
    st.reset()
    q.pop("known")
    toks_i, img_i = _run_slot(st, st.admit(image=case["img"], **q))
    assert torch.equal(toks_i, toks_k) and torch.equal(img_i, img_k) and torch.equal(img_i, vq.decode_indices(toks_i[None])[0])
    assert tuple(img_i.shape) == (3, H6 * 8, H6 * 8) and st.captures == 1


def test_stream_editing_ragged(tiny_sd, edit_case):
    """(i): an editing request with a short prompt (1 ByT5 row + clip on both sides) among longer ones in a max_cond_rows stream == the same request, same B and slot,
    in a strict stream built on exactly its layout"""
    m, cfg, case = tiny_sd[0], G.UNET_TINY, edit_case
    short = dict(_xreq(case, "step", steps=3), model_inputs=to_dev(cond_for(cfg, 1, 1, 0, 3), DEV), unconditional_inputs=to_dev(cond_for(cfg, 1, 1, 0, 103), DEV))
    longer = lambda i, n, img: dict(model_inputs=to_dev(cond_for(cfg, 1, n, img, 10 + i), DEV), unconditional_inputs=to_dev(cond_for(cfg, 1, 1, 0, 110 + i), DEV), seed=20 + i,
                                    steps=4, cfg=6.0)
    rag = paella_amd.RequestStream(m, short["model_inputs"], short["unconditional_inputs"], (3, H6, H6), max_steps=4, device=DEV, max_cond_rows=16, editing=True)
    rag.admit(**longer(0, 3, 0)), rag.admit(**dict(longer(1, 7, 1), known=case["known"], mask=case["mask"], pin="final"))
    slot = rag.admit(**short)
    assert slot == 2 and rag.cache.lens.tolist()[:3] == [7, 15, 5]
    got = _run_slot(rag, slot)
    strict = paella_amd.RequestStream(m, short["model_inputs"], short["unconditional_inputs"], (3, H6, H6), max_steps=4, device=DEV, editing=True)
    same = lambda i: dict(model_inputs=to_dev(cond_for(cfg, 1, 1, 0, 30 + i), DEV), unconditional_inputs=to_dev(cond_for(cfg, 1, 1, 0, 130 + i), DEV), seed=50 + i, steps=4, cfg=6.0)
    strict.admit(**same(0)), strict.admit(**same(1))
    want = _run_slot(strict, strict.admit(**short))
    assert torch.equal(got, want), "the ragged editing stream differs from the strict one at %d positions" % int((got != want).sum())
    assert torch.equal(got[case["mask"] == 0], case["known"][case["mask"] == 0]) and rag.captures == 1


def test_editing_error_paths(tiny_sd, tiny_vq, edit_case, built_lib):
    """(j)"""
    m, vq, cfg, case = tiny_sd[0], tiny_vq, G.UNET_TINY, edit_case
    q = _xreq(case, "step")
    plain_st = _edit_stream(m, cfg, 1, editing=False)
    for extra in (dict(known=case["known"], mask=case["mask"]), dict(mask=case["mask"]), dict(image=case["img"])):
        with pytest.raises(ValueError, match="editing=True"):
            plain_st.admit(**dict(_request(cfg, 5, seed=1, steps=2), **extra))
    st = _edit_stream(m, cfg, 1)
    no = lambda *names: {k: v for k, v in q.items() if k not in names}
    bad = [(no("known"), "mask"), (no("mask"), "mask"), (dict(no("known"), image=case["img"]), "VQGAN"), (dict(q, pin="always"), "pin must be"), (dict(q, pin="never"), "pin must be"),
           (dict(q, known=case["known"][:, :-1]), "known must be"), (dict(q, known=case["known"].int()), "known must be"), (dict(q, mask=case["mask"][1:]), "mask must be"),
           (dict(q, mask=case["mask"].float()), "mask must be")]
    for args, msg in bad:
        with pytest.raises(ValueError, match=msg):
            st.admit(**args)
    with_vq = _edit_stream(m, cfg, 1, vq=vq)
    with pytest.raises(ValueError, match="mutually exclusive"):
        with_vq.admit(**dict(q, image=case["img"]))
    with pytest.raises(ValueError, match="image must be"):
        with_vq.admit(**dict(no("known"), image=case["img"][:, :-8]))
    assert st.free_slots == [0] and with_vq.free_slots == [0] and plain_st.free_slots == [0]
    # forward_sample(pin=...)
    x = torch.zeros(1, 8, 8, dtype=torch.int64, device=DEV)
    c, _u = _one(cfg, 1)
    cache = m.prepare_cond(**c)
    for pin in ((x, x, _i32([1])), (x,), (x, x.int()), (x[:, :4], x)):
        with pytest.raises(ValueError):
            m.forward_sample(x, _f32([0.5]), cache, x.clone(), temperature=1.0, pin=pin)
    with pytest.raises(ValueError, match="categorical"):
        m.forward_sample(x, _f32([0.5]), cache, x.clone(), temperature=1.0, argmax=True, pin=(x, x))
    # the C ABI
    lib, p = built_lib, _lib.ptr
    lg = torch.zeros(64, 12, device=DEV)
    out = torch.zeros(64, dtype=torch.int64, device=DEV)
    req = _tables(2, 1, [1, 2], None, (1.0, 1.0))
    stp, tn, ac = _i32([0, 0]), _f32([0.5, 0.5]), _i32([1, 1])
    tail = lambda keep, known, on, o=out: lib.paella_sample_tail_stream_pin(p(lg), None, 64, 12, None, p(req.temps[0]), p(req.seeds), 32, p(stp), p(tn), p(ac), p(out), p(keep),
                                                                          p(known), p(on), p(o), None, _stream())
    assert tail(out, out, ac) == 0 and tail(None, None, None) == 0
    for args, msg in (((out, None, None), b"together"), ((None, out, ac), b"together"), ((None, None, ac), b"pin_on without"), ((out, out, ac, None), b"null argument")):
        assert tail(*args) == -1 and msg in lib.paella_last_error(), args
    scalar = lambda keep, known, mode=0, o=out: lib.paella_sample_tail_pin(p(lg), None, 64, 12, 1.0, 0.0, 1.0, mode, 3, None, 0, 0, None, None, 0.0, p(keep), p(known), p(o), None, _stream())
    assert scalar(out, out) == 0
    for args, msg in (((out, None), b"together"), ((None, out), b"together"), ((out, out, 1), b"argmax"), ((out, out, 0, None), b"null argument")):
        assert scalar(*args) == -1 and msg in lib.paella_last_error(), args
    fl = torch.zeros(2, device=DEV)
    prog, pos, ln = torch.zeros(2, 4, 5, device=DEV), _i32([0, 0]), _i32([0, 0])
    step_pin = lambda pol, on: lib.paella_request_step_pin(p(prog), 4, p(pos), p(ln), 2, p(fl), p(fl.clone()), None, p(fl.clone()), p(stp), p(ac), p(pol), p(on), _stream())
    pol, on = _i32([1, 2]), _i32([-1, -1])
    assert step_pin(pol, on) == 0 and step_pin(None, None) == 0
    assert step_pin(pol, None) == -1 and b"together" in lib.paella_last_error()
    assert step_pin(None, on) == -1
    h = m._engine()
    ws = m.new_workspace(1, 8, 8, cache.S)
    fwd = lambda keep, known, on, o: lib.paella_unet_forward_sample_stream_pin(h, p(x), p(_f32([0.5])), p(cache.buf), 1, 1, None, 8, 8, cache.S, None, None, 0, p(req.seeds), p(req.temps[0]),
                                                                              64, p(stp), p(tn), p(ac), p(out), p(keep), p(known), p(on), p(o), p(ws), ws.numel(), _stream())
    for args, msg in (((out, None, None, out), b"together"), ((None, None, ac, out), b"pin_on without"), ((out, out, ac, None), b"null argument")):
        assert fwd(*args) == -1 and msg in lib.paella_last_error(), args
    sfwd = lambda keep, known, o: lib.paella_unet_forward_sample_pin(h, p(x), p(_f32([0.5])), p(cache.buf), 1, 1, 0.0, 0.0, 8, 8, cache.S, None, None, 0, 1.0, 0, 3, None, 0, 0, None, None,
                                                                    0.0, p(keep), p(known), p(o), p(ws), ws.numel(), _stream())
    for args, msg in (((out, None, out), b"together"), ((None, out, out), b"together"), ((out, out, None), b"null argument")):
        assert sfwd(*args) == -1 and msg in lib.paella_last_error(), args
    torch.cuda.synchronize()
