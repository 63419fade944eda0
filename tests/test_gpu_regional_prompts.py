"""GPU: regional prompts -- per-query key groups in the attention kernels (paella_op_attention_rg), in the forward (forward_prepared(regions=)) and in the
request stream (RequestStream(max_regions=), admit(regions=)).

The kernel properties (include/paella_hip.h, "Regional prompts"): all visible == the launch without the tables, bit for bit, in every dispatch form; conditioning
keys [n, cond_len) invisible to every query == cond_len = n, bit for bit; a query with no visible key in a tile, a stage, a wave's share or at all never produces
NaN (a zero row in the last case); k_groups entries beyond cond_len are without effect.  The fp64 specification is tests/region_model.py."""
import pytest
import torch

import paella_amd
from oracle import golden_configs as G
from paella_amd import _lib
from paella_amd.modules import CondCache
from tests import region_model as RM
from tests.helpers import cond_for, to_dev, weights_for
from tests.test_gpu_ragged_conditioning import COND_LEN, COND_LEN_KW, N_KW, NHEAD, S_SLOT, _attn_inputs, _variants

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(16, 16), (64, 64), (64, 0), (256, 256)]
DIMS = [16, 64, 80]
# test_gpu_ops.py::test_attention holds the unmasked kernels to these on the same randn inputs; a masked softmax is an unmasked softmax over a subset of keys
ATOL, RTOL = 2e-5, 1e-4


def _stream():
    return _lib.stream_ptr(torch.device(DEV))


def _i32(t):
    return torch.as_tensor(t, dtype=torch.int32).contiguous().to(DEV)


def _launch(lib, inp, D, Lq, Lself, lens_d=None, qg=None, kg=None, kw=None, kw_len=None):
    q, ks, vs, kc, vc = inp[:5]
    B, ld = kc.size(0), NHEAD * D
    out = torch.full((B * Lq, ld), float("nan"), device=DEV)
    _lib.check(lib.paella_op_attention_rg(_lib.ptr(q), _lib.ptr(ks) if Lself else None, _lib.ptr(vs) if Lself else None, _lib.ptr(kc), _lib.ptr(vc), _lib.ptr(out), B, NHEAD,
                                          D, Lq, Lself, S_SLOT, _lib.ptr(inp[6] if lens_d is None else lens_d), _lib.ptr(kw), _lib.ptr(kw_len),
                                          0 if kw is None else kw.size(1), _lib.ptr(qg), 0 if qg is None else qg.size(1), _lib.ptr(kg), 0 if kg is None else kg.size(1),
                                          _stream()))
    torch.cuda.synchronize()
    return out


def _kw_table(B, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, N_KW, generator=g) + 0.5).to(DEV), torch.full((B,), N_KW, dtype=torch.int32, device=DEV)


def _model_out(inp, lens, Lq, Lself, qg, kg, kw=None, kw_len=None):
    q, ks, vs, kc, vc = (t.cpu() for t in inp[:5])
    return RM.attention_batch(q, ks, vs, kc, vc, lens, NHEAD, Lq, Lself, qg.cpu(), kg.cpu(), None if kw is None else kw.cpu(), None if kw_len is None else kw_len.cpu())


def _assert_close(got, ref, what):
    assert torch.isfinite(got).all(), "%s: non-finite output" % what
    err = (got.cpu().double() - ref).abs()
    bound = ATOL + RTOL * ref.abs()
    worst = float((err - bound).max())
    print("%s: max |diff| %.3e" % (what, float(err.max())))
    assert worst <= 0, "%s: max |diff| %.3e, %.3e beyond atol %.0e + rtol %.0e |ref|" % (what, float(err.max()), worst, ATOL, RTOL)


@pytest.mark.parametrize("Lq,Lself", SHAPES)
@pytest.mark.parametrize("D", DIMS)
def test_all_visible_is_bit_identical_to_no_tables(built_lib, D, Lq, Lself):
    """1. every conditioning key visible to every query (by one shared bit among random others) == both tables null, without and with key weights"""
    lib = built_lib
    try:
        for variant in _variants(Lq):
            lib.paella_test_attention_variant(variant)
            for lens, weighted in ((COND_LEN, False), (COND_LEN_KW, True)):
                B = len(lens)
                inp = _attn_inputs(D, Lq, Lself, lens, 100 * D + Lq + Lself)
                g = torch.Generator().manual_seed(D + Lq)
                qg = _i32(torch.randint(0, 1 << 30, (B, Lq + 3), generator=g) | 4)
                kg = _i32(torch.randint(0, 1 << 30, (B, S_SLOT + 2), generator=g) | 4)
                kw, kw_len = _kw_table(B, 5) if weighted else (None, None)
                ref = _launch(lib, inp, D, Lq, Lself, kw=kw, kw_len=kw_len)
                got = _launch(lib, inp, D, Lq, Lself, qg=qg, kg=kg, kw=kw, kw_len=kw_len)
                assert torch.isfinite(ref).all()
                assert torch.equal(got, ref), "variant %d, weighted %s: %d values differ from the launch without the tables" % (variant, weighted, int((got != ref).sum()))
    finally:
        lib.paella_test_attention_variant(0)


@pytest.mark.parametrize("Lq,Lself", SHAPES)
@pytest.mark.parametrize("D", DIMS)
def test_invisible_behind_is_bit_identical_to_absent(built_lib, D, Lq, Lself):
    """2. the keys from n_vis on (clamped to the sample's length) carry a group no query has == the ragged launch at cond_len = n_vis"""
    lib = built_lib
    try:
        for variant in _variants(Lq):
            lib.paella_test_attention_variant(variant)
            inp = _attn_inputs(D, Lq, Lself, COND_LEN, 7 * D + Lq + Lself)
            B = len(COND_LEN)
            qg = _i32(torch.ones(B, Lq))
            for n_vis in (1, 15, 16, 17, 31, 32):
                cut = [min(n_vis, n) for n in COND_LEN]
                kg = torch.full((B, S_SLOT), 2, dtype=torch.int32)
                for b, n in enumerate(cut):
                    kg[b, :n] = 1
                got = _launch(lib, inp, D, Lq, Lself, qg=qg, kg=_i32(kg))
                ref = _launch(lib, inp, D, Lq, Lself, lens_d=_i32(cut))
                assert torch.isfinite(ref).all()
                assert torch.equal(got, ref), "variant %d, n_vis %d: %d values differ from cond_len = n_vis" % (variant, n_vis, int((got != ref).sum()))
    finally:
        lib.paella_test_attention_variant(0)


def _constructed_groups(B, Lq, lens, seed):
    """random 3-bit groups with per-query different masks, plus, in every sample: query 0 sees only the conditioning keys from 32 on (its first 16-key tile and
    first 32-key stage of conditioning keys are invisible; nothing at all where the sample has <= 32 rows), query 1 only the LAST key, query 2 no conditioning key
    (with Lself == 0: nothing -> a zero row), query 3 only the FIRST key.  With Lself == 0 and 40 rows the key-split waves own tiles 0 / 1 / 2: query 1 leaves
    waves 0 and 1 with invisible tiles only, query 3 waves 1 and 2, query 2 all of them"""
    g = torch.Generator().manual_seed(seed)
    qg = torch.randint(0, 8, (B, Lq), generator=g, dtype=torch.int32)
    kg = torch.randint(1, 8, (B, S_SLOT), generator=g, dtype=torch.int32)
    qg[:, 0], qg[:, 1], qg[:, 2], qg[:, 3] = 8, 16, 0, 32
    kg[:, 32:] |= 8
    for b, n in enumerate(lens):
        kg[b, n - 1] |= 16
    kg[:, 0] |= 32
    return qg, kg


@pytest.mark.parametrize("Lq,Lself", SHAPES)
@pytest.mark.parametrize("D", DIMS)
def test_masked_attention_against_the_fp64_model(built_lib, D, Lq, Lself):
    """3. (+ 4. and 5.) random and constructed groups against tests/region_model.py in every dispatch form; k_groups entries beyond cond_len are without effect;
    one case with the key-weight table on top"""
    lib = built_lib
    B = len(COND_LEN)
    inp = _attn_inputs(D, Lq, Lself, COND_LEN, 3 * D + Lq + Lself)              # cond_len = [40, 1, 16, 17, 32, 33]
    inp_kw = _attn_inputs(D, Lq, Lself, COND_LEN_KW, 5 * D + Lq + Lself)        # with the key-weight table: 4 weights must fit every sample's own keys
    qg, kg = _constructed_groups(B, Lq, COND_LEN, D + Lq + Lself)
    qg_kw, kg_kw = _constructed_groups(B, Lq, COND_LEN_KW, D + Lq + Lself + 1)
    ref = _model_out(inp, COND_LEN, Lq, Lself, qg, kg)
    if Lself == 0:
        assert bool((ref.view(B, Lq, -1)[:, 2] == 0).all()) and bool((ref.view(B, Lq, -1)[1:5, 0] == 0).all())   # the model's zero rows (samples of <= 32 rows: query 0 too)
    kw, kw_len = _kw_table(B, 9)
    ref_kw = _model_out(inp_kw, COND_LEN_KW, Lq, Lself, qg_kw, kg_kw, kw, kw_len)
    beyond0, beyond1 = kg.clone(), kg.clone()
    for b, n in enumerate(COND_LEN):
        beyond0[b, n:], beyond1[b, n:] = 0, -1
    try:
        for variant in _variants(Lq):
            lib.paella_test_attention_variant(variant)
            got = _launch(lib, inp, D, Lq, Lself, qg=_i32(qg), kg=_i32(kg))
            _assert_close(got, ref, "D %d Lq %d Lself %d variant %d" % (D, Lq, Lself, variant))
            if Lself == 0:
                assert bool((got.view(B, Lq, -1)[:, 2] == 0).all()), "a query that sees no key must give a zero row"
            a, b_ = _launch(lib, inp, D, Lq, Lself, qg=_i32(qg), kg=_i32(beyond0)), _launch(lib, inp, D, Lq, Lself, qg=_i32(qg), kg=_i32(beyond1))
            assert torch.equal(a, got) and torch.equal(b_, got), "variant %d: k_groups entries beyond cond_len changed the output" % variant
            got_kw = _launch(lib, inp_kw, D, Lq, Lself, qg=_i32(qg_kw), kg=_i32(kg_kw), kw=kw, kw_len=kw_len)
            _assert_close(got_kw, ref_kw, "D %d Lq %d Lself %d variant %d with the key-weight table" % (D, Lq, Lself, variant))
    finally:
        lib.paella_test_attention_variant(0)


# ---------------------------------------------------------------------------------------------------------------- models
def _model(cfg):
    m = paella_amd.Paella(**cfg)
    sd = weights_for(m, sum(cfg["blocks"]))
    return m.to(DEV), sd


@pytest.fixture(scope="module")
def tiny(built_lib):
    return _model(G.UNET_TINY)


def _prompt(cfg, n_byt5, seed, n_img=0):
    return cond_for(cfg, 1, n_byt5, n_img, seed)


def _rows(cfg, p):
    ci = p.get("clip_image")
    return p["byt5"].size(1) + cfg["clip_seq_len"] * (1 + (0 if ci is None else len(ci) if isinstance(ci, (list, tuple)) else 1))


@pytest.mark.parametrize("cfg_name,grid,atol", [("UNET_TINY", 32, 2e-5), ("UNET_VARIANT", 8, 2e-5)])   # the bounds test_gpu_ragged_conditioning / test_gpu_unet apply
def test_forward_prepared_regions_against_the_model(built_lib, monkeypatch, cfg_name, grid, atol):
    """6. a guided 2B-slot ragged forward: sample 0 = base + two regions (left / right halves), sample 1 = base + one region whose mask cuts through 2x2 blocks;
    the unconditional side is plain.  Mixed logits against the masked oracle."""
    cfg = getattr(G, cfg_name)
    m, sd = _model(cfg)
    B, L, H, W, S = 2, cfg["num_labels"], grid, grid, 24
    mix = (0.625, 0.375)                                    # a convex mix: the per-forward bound holds for the mixed logits (test_gpu_ragged_conditioning.py)
    left = torch.zeros(H, W, dtype=torch.bool)
    left[:, : W // 2] = True
    cut = torch.zeros(H, W, dtype=torch.bool)
    cut[1:H - 3, 3:W - 2] = True
    samples = [([_prompt(cfg, 3, 1), _prompt(cfg, 2, 2), _prompt(cfg, 5, 3)], torch.stack([left, ~left])),
               ([_prompt(cfg, 4, 4, n_img=1), _prompt(cfg, 1, 5)], cut[None])]
    unc = [_prompt(cfg, 1, 6), _prompt(cfg, 2, 7)]
    g = torch.Generator().manual_seed(3)
    x = torch.randint(0, L, (B, H, W), generator=g)
    r = torch.tensor([0.7, 0.3])
    Qtot = paella_amd.modules.region_query_total(cfg, H, W)
    tables = paella_amd.RegionTables(2 * B, Qtot, S, DEV)
    buf = torch.zeros(m.cond_bytes(2 * B, S), dtype=torch.uint8, device=DEV)
    lens = torch.zeros(2 * B, dtype=torch.int32, device=DEV)
    row = m.cond_bytes(1, 1)
    scratch = torch.zeros(1, dtype=torch.int32, device=DEV)
    ref = []
    for b, (prompts, masks) in enumerate(samples):
        off, k_row = 0, []
        for i, p in enumerate(prompts):                     # prompt 0 = the base (bit 0), prompt i = region i - 1 (bit i)
            n = _rows(cfg, p)
            m.prepare_cond(**to_dev(p, DEV), out=buf[(b * S + off) * row:(b * S + off + n) * row], slot_rows=n, lens_out=scratch)
            k_row += [1 << i] * n
            off += n
        lens[b] = off
        q_row = paella_amd.region_query_groups(masks, cfg, H, W)
        tables.set(b, q_row.to(DEV), torch.tensor(k_row, dtype=torch.int32))
        u = unc[b]
        m.prepare_cond(**to_dev(u, DEV), out=buf[(B + b) * S * row:((B + b) * S + _rows(cfg, u)) * row], slot_rows=_rows(cfg, u), lens_out=lens[B + b:B + b + 1])
        lc = RM.regional_forward(monkeypatch, sd, cfg, x[b:b + 1], r[b:b + 1], prompts, q_row.tolist(), k_row)
        lu = RM.regional_forward(monkeypatch, sd, cfg, x[b:b + 1], r[b:b + 1], [u], [1] * Qtot, [1] * _rows(cfg, u))
        ref.append(lc * mix[0] + lu * mix[1])
    ref = torch.cat(ref)
    cache = CondCache(buf, 2 * B, S, lens)
    got = m.forward_prepared(x.to(DEV), r.to(DEV), cache, cfg_mix=mix, regions=tables)
    diff = float((got.cpu() - ref).abs().max())
    plain = m.forward_prepared(x.to(DEV), r.to(DEV), cache, cfg_mix=mix)
    print("%s regional 2B forward, mixed logits vs the masked oracle: max |diff| %.3e (bound %.0e); the regions move the logits by up to %.3e"
          % (cfg_name, diff, atol, float((got - plain).abs().max())))
    assert torch.isfinite(got).all() and diff <= atol
    assert float((got - plain).abs().max()) > 100 * atol, "the regions did not act"
    # everything visible == the forward without the tables, bit for bit
    assert torch.equal(m.forward_prepared(x.to(DEV), r.to(DEV), cache, cfg_mix=mix, regions=paella_amd.RegionTables(2 * B, Qtot, S, DEV)), plain)
    # the checks that need a model (the rest: tests/test_regional_prompts.py): a q_groups pitch below Qtot, and the bf16 precision mode
    lib, h = built_lib, m._engine()
    ws = m.new_workspace(2 * B, H, W, S)
    xd, rd, out = x.to(DEV), r.to(DEV), torch.empty(2 * B, H, W, L, device=DEV)
    call = lambda qp: lib.paella_unet_forward_shared_req_rg(h, _lib.ptr(xd), _lib.ptr(rd), _lib.ptr(buf), 2 * B, B, None, H, W, S, _lib.ptr(lens), None, None, 0,
                                                            _lib.ptr(tables.q_groups), qp, _lib.ptr(tables.k_groups), S, _lib.ptr(out), _lib.ptr(ws), ws.numel(), _stream())
    assert call(Qtot - 1) == -1 and b"qg_pitch" in lib.paella_last_error()
    assert call(Qtot) == 0
    m.set_gemm_precision("bf16")
    try:
        assert call(Qtot) == -1 and b"bf16" in lib.paella_last_error()
        with pytest.raises(ValueError, match="bf16"):
            m.forward_prepared(xd, rd, cache, cfg_mix=mix, regions=tables)
    finally:
        m.set_gemm_precision("fp32")
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- request stream
STREAM_SHAPE, STEPS = (4, 32, 32), 3
HALF = torch.zeros(32, 32, dtype=torch.bool)
HALF[:, :16] = True


def _request(cfg, n_byt5, seed, **over):
    return dict(dict(model_inputs=to_dev(_prompt(cfg, n_byt5, seed), DEV), unconditional_inputs=to_dev(_prompt(cfg, 1, seed + 100), DEV), seed=1000 + seed, steps=STEPS,
                     cfg=6.0), **over)


def _regions(cfg, seed, masks=(HALF, ~HALF)):
    return [(to_dev(_prompt(cfg, 2 + i, seed + 10 * i), DEV), mk) for i, mk in enumerate(masks)]


def _serve(st, before, req, pre_ticks):
    """admit `before` (they take the first slots), tick pre_ticks times, then admit `req` (the next slot) and run it to the end: its tokens"""
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


def test_request_stream_regions(tiny):
    """7. and 8. (a) - (d): fused == filtered with every filter off; independence of batch-mates and admission tick; regions=None == a stream without max_regions;
    an all-zero mask is a no-op; a reused slot inherits nothing, with and without reset()"""
    m, _ = tiny
    cfg = G.UNET_TINY
    base = _request(cfg, 3, 1)
    mk = lambda **k: paella_amd.RequestStream(m, base["model_inputs"], base["unconditional_inputs"], STREAM_SHAPE, max_steps=4, device=DEV, max_cond_rows=24, **k)
    st, plain, filt = mk(max_regions=2), mk(), mk(max_regions=2, filtering=True)
    assert tuple(st.regions.q_groups.shape) == (8, 256 + 64 + 16) and tuple(st.regions.k_groups.shape) == (8, 24) and bool((st.regions.q_groups == 1).all())
    regional = dict(base, regions=_regions(cfg, 20))                                                   # 7 base rows + 6 + 7
    idle = lambda i, **k: dict(_request(cfg, 2 + i, 50 + i, **k), steps=1)                             # finishes with the first tick and keeps its slot
    mates = [idle(0), idle(1, regions=_regions(cfg, 30, masks=(~HALF,)))]
    a = _serve(st, mates, regional, 1)                                                                 # (a) slot 2, nobody else running
    assert st.cache.lens.tolist()[2] == 7 + 6 + 7 and st.regions.k_groups[2, :20].tolist() == [1] * 7 + [2] * 6 + [4] * 7
    assert sorted(set(st.regions.q_groups[2].tolist())) == [3, 5] and bool((st.regions.q_groups[6] == 1).all()) and bool((st.regions.k_groups[6] == 1).all())
    running = [dict(_request(cfg, 4, 60), steps=4, regions=_regions(cfg, 40)), dict(_request(cfg, 1, 61), steps=4)]
    b = _serve(st, running, regional, 0)                                                               # a regional and a plain mate, joined together
    d = _serve(st, running, regional, 2)                                                               # joins two ticks after its mates
    assert torch.equal(a, b), "tokens depend on the batch-mates (%d positions)" % int((a != b).sum())
    assert torch.equal(a, d), "tokens depend on the tick the request joined at (%d positions)" % int((a != d).sum())
    f = _serve(filt, mates, regional, 1)                                                               # 7. the filtered tick with every filter off
    assert torch.equal(a, f), "fused and unfused ticks disagree at %d positions" % int((a != f).sum())
    p = _serve(plain, [idle(0), idle(1)], base, 1)
    assert not torch.equal(a, p), "the regions did not act"
    n = _serve(st, mates, base, 1)                                                                     # (b) regions=None on a max_regions stream
    assert torch.equal(n, p), "regions=None differs from a stream without max_regions at %d positions" % int((n != p).sum())
    z = _serve(st, mates, dict(base, regions=[(_regions(cfg, 20)[0][0], torch.zeros(32, 32, dtype=torch.int64))]), 1)   # (c) an all-zero mask
    assert torch.equal(z, p), "a region with an all-zero mask changed %d positions" % int((z != p).sum())
    # (d) slot 2 reused WITHOUT a reset by a plain request right after a regional one, and the same after reset()
    assert torch.equal(_serve(st, mates, regional, 1), a)
    assert st.admit(**base) == 2 and st.cache.lens.tolist()[2] == 7 and bool((st.regions.q_groups[2] == 1).all()) and bool((st.regions.k_groups[2] == 1).all())
    for _ in range(STEPS):
        done = st.tick()
    assert done == [2]
    reused = st.result(2)
    assert torch.equal(reused, p), "a reused slot inherits its predecessor's regions: %d positions differ" % int((reused != p).sum())
    st.reset()
    assert bool((st.regions.q_groups == 1).all()) and bool((st.regions.k_groups == 1).all())
    assert torch.equal(_serve(st, mates, base, 1), p)
    assert st.captures == 1 and plain.captures == 1 and filt.captures == 1                             # (e)
    with pytest.raises(ValueError, match="regions"):
        plain.admit(**regional)
    with pytest.raises(ValueError, match="regions"):
        st.admit(**dict(base, regions=_regions(cfg, 20, masks=(HALF, ~HALF, HALF))))
    with pytest.raises(ValueError, match="max_regions"):
        paella_amd.RequestStream(m, base["model_inputs"], base["unconditional_inputs"], STREAM_SHAPE, max_steps=4, device=DEV, max_regions=2)


def test_request_stream_editing_with_regions(tiny):
    """8. (e) one editing + regional request next to a plain one on an editing stream: one capture, the known tokens pinned, independent of the batch-mates"""
    m, _ = tiny
    cfg, (B, H, W) = G.UNET_TINY, STREAM_SHAPE
    g = torch.Generator().manual_seed(12)
    known = torch.randint(0, cfg["num_labels"], (H, W), generator=g).to(DEV)
    mask = torch.zeros(H, W, dtype=torch.int64)
    mask[8:24, 4:20] = 1
    base = _request(cfg, 3, 1)
    edit = dict(base, known=known, mask=mask.to(DEV), pin="step", t_start=0.7, temperature=(0.7, 0.3))
    st = paella_amd.RequestStream(m, base["model_inputs"], base["unconditional_inputs"], STREAM_SHAPE, max_steps=4, device=DEV, editing=True, max_cond_rows=24,
                                  max_regions=2, max_attn_weights=4)
    mate = lambda i, **k: dict(_request(cfg, 3, 50 + i, **k), steps=1)
    both = dict(edit, regions=_regions(cfg, 20), attn_weights=torch.tensor([1.5, 0.5], device=DEV))
    a = _serve(st, [mate(0), mate(1)], both, 1)
    b = _serve(st, [dict(_request(cfg, 2, 70), steps=4, regions=_regions(cfg, 40)), dict(_request(cfg, 1, 71), steps=4)], both, 2)
    keep0 = mask.to(DEV) == 0
    assert torch.equal(a, b) and torch.equal(a[keep0], known[keep0]) and st.captures == 1
    assert not torch.equal(_serve(st, [mate(0), mate(1)], dict(edit, attn_weights=both["attn_weights"]), 1), a), "the regions did not act"
