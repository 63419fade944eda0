"""GPU: the argument blocks (include/paella_hip.h: paella_unet_step / paella_sample_tail_args) against every fixed-form entry point over them.  Each case calls the
fixed-form entry point and the block entry point with the same inputs into separate outputs and compares every output bit for bit: both must reach the same launch
with the same arguments, so any difference is a field of the block mapped wrongly.  No tolerance anywhere.

UNET_TINY on an 8 x 16 grid (8 is the smallest side three levels of patch 2 admit; not square, so an H / W swap shows), 2 guided samples = 4 conditioning slots
with ragged ByT5 lengths 3 and 5, num_labels 64, one step; the stream forms hold one inactive slot, so "stores nothing" is compared as well."""
import ctypes
import types

import pytest
import torch

import paella_amd
from oracle import golden_configs as G
from paella_amd import _lib, synth
from tests.helpers import cond_for, to_dev

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, W, NU, B = 8, 16, 2, 4
HW, ROWS = H * W, NU * H * W
FILL = -7  # what every output holds before a call: rows that are not stored (an inactive slot) compare as well


@pytest.fixture(scope="module")
def ctx(built_lib):
    cfg = G.UNET_TINY
    m = paella_amd.Paella(**cfg)
    synth.randomize_(m, seed=0)
    m = m.to(DEV)
    L, n_clip = cfg["num_labels"], cfg["clip_seq_len"]
    S = 5 + n_clip
    row = m.cond_bytes(1, 1)
    buf = torch.zeros(m.cond_bytes(B, S), dtype=torch.uint8, device=DEV)
    lens = torch.zeros(B, dtype=torch.int32, device=DEV)
    for slot, n_byt5 in enumerate((3, 5, 5, 3)):  # conditional slots 0, 1 (ByT5 lengths 3 and 5), then the unconditional ones
        n = n_byt5 + n_clip
        m.prepare_cond(**to_dev(cond_for(cfg, 1, n_byt5, 0, 10 + slot), DEV), out=buf[slot * S * row:(slot * S + n) * row], slot_rows=n, lens_out=lens[slot:slot + 1])
    g = torch.Generator().manual_seed(5)
    i64 = lambda *shape, hi=L: torch.randint(0, hi, shape, generator=g).to(DEV)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)
    f32 = lambda v: torch.tensor(v, dtype=torch.float32, device=DEV)
    kw = paella_amd.KeyWeights(B, 3, DEV)
    for slot, w in enumerate(([1.5, 0.5], None, [0.25, 2.0, 1.0], [0.75])):
        kw.set(slot, w)
    Qtot = paella_amd.modules.region_query_total(cfg, H, W)
    rg = paella_amd.RegionTables(B, Qtot, S, DEV)
    rg.q_groups.copy_(torch.randint(1, 4, (B, Qtot), generator=g).int())  # bits 0 and 1: every query sees the rows of one or both groups
    rg.k_groups.copy_(torch.randint(1, 4, (B, S), generator=g).int())
    c = types.SimpleNamespace(
        lib=built_lib, m=m, h=m._engine(), L=L, S=S, buf=buf, lens=lens, kw=kw, rg=rg, Qtot=Qtot, ws=m.new_workspace(B, H, W, S), stream=_lib.stream_ptr(torch.device(DEV)),
        x=i64(NU, H, W), r=f32([0.7, 0.3]), aw=f32([1.25, 0.5]), pairs=f32([[1.5, -0.5], [3.0, -2.0]]),
        lc=torch.randn(ROWS, L, generator=g).to(DEV), lu=torch.randn(ROWS, L, generator=g).to(DEV),
        noise_q=torch.empty(ROWS, L).exponential_(1, generator=g).to(DEV), mask_u=torch.rand(ROWS, generator=g).to(DEV),
        seeds=torch.tensor([11, (1 << 62) + 5], dtype=torch.int64, device=DEV), temps=f32([0.9, 1.2]), step=i32([1, 2]), t_next=f32([0.5, 0.25]), active=i32([1, 0]),
        init=i64(ROWS), keep=i64(ROWS, hi=2), known=i64(ROWS), pin_on=i32([1, 1]), filter_k=i32([[5, 1], [0, 2]]), filter_mass=f32([[1.0, 1.0], [0.5, 1.0]]),
        seed_dev=torch.tensor([3], dtype=torch.int64, device=DEV), row_dev=torch.tensor([HW], dtype=torch.int64, device=DEV))
    torch.cuda.synchronize()
    return c


def _outputs(c):
    return types.SimpleNamespace(tok=torch.full((ROWS,), FILL, dtype=torch.int64, device=DEV), pre=torch.full((ROWS,), FILL, dtype=torch.int64, device=DEV),
                                 logits=torch.full((B * HW, c.L), float(FILL), device=DEV), lp=torch.full((ROWS,), float(FILL), device=DEV),
                                 ent=torch.full((ROWS,), float(FILL), device=DEV))


def _fill(block, fields):
    for k, v in fields.items():
        setattr(block, k, v.data_ptr() if torch.is_tensor(v) else v)
    return block


# ---- what the cases share.  Fixed-form argument lists are tuples in the header's order; block fields are dicts
def FWD(c):
    return (c.h, c.x, c.r, c.buf, B, NU)


def END(c):
    return (c.ws, c.ws.numel(), c.stream)


def STEP(c, **kw):
    return dict(dict(tokens=c.x, r=c.r, cond=c.buf, B=B, n_unique=NU, H=H, W=W, S=c.S), **kw)


def KW(c):
    return (c.kw.buf, c.kw.lens, c.kw.pitch)


def KWB(c):
    return dict(kw_table=c.kw.buf, kw_len=c.kw.lens, kw_pitch=c.kw.pitch)


def RG(c):
    return (c.rg.q_groups, c.Qtot, c.rg.k_groups, c.S)


def RGB(c):
    return dict(q_groups=c.rg.q_groups, qg_pitch=c.Qtot, k_groups=c.rg.k_groups, kg_pitch=c.S)


def REQ(c):
    return (c.seeds, c.temps, HW)


def REQB(c, o, **kw):
    return dict(dict(seeds=c.seeds, temperature_tab=c.temps, rows_per_sample=HW, init_noise=c.init, tokens_out=o.tok), **kw)


def STRM(c):
    return (c.step, c.t_next, c.active, c.init)


def STRMB(c):
    return dict(step=c.step, t_next_tab=c.t_next, active=c.active)


def PIN3(c):
    return (c.keep, c.known, c.pin_on)


def PIN3B(c):
    return dict(pin_keep=c.keep, pin_tokens=c.known, pin_on=c.pin_on)


def SCAL(c):  # temperature, mode, seed, seed_ptr, offset, row_offset, row_offset_ptr, init_noise, t_next
    return (0.8, 0, 77, c.seed_dev, 2, 3 * HW, c.row_dev, c.init, 0.4)


def SCALB(c, o, **kw):
    return dict(dict(temperature=0.8, mode=0, seed=77, seed_ptr=c.seed_dev, offset=2, row_offset=3 * HW, row_offset_ptr=c.row_dev, init_noise=c.init, t_next=0.4,
                     tokens_out=o.tok), **kw)


def TAIL(c):  # logits_c, logits_u, rows, L, cfg, one_minus_cfg
    return (c.lc, c.lu, ROWS, c.L, 4.0, -3.0)


def TAILB(c, **kw):
    return dict(dict(logits_c=c.lc, logits_u=c.lu, rows=ROWS, L=c.L, cfg=4.0, one_minus_cfg=-3.0), **kw)


def RTAIL(c):  # the request / stream tails: logits_c, logits_u, rows, L, cfg_pairs, temperature, seeds, rows_per_sample
    return (c.lc, c.lu, ROWS, c.L, c.pairs, c.temps, c.seeds, HW)


def RTAILB(c, o, **kw):
    return REQB(c, o, **dict(dict(logits_c=c.lc, logits_u=c.lu, rows=ROWS, L=c.L, cfg_pairs=c.pairs, sampled_out=o.pre), **kw))


# name -> (fixed-form entry point, its arguments, the step block's fields or None, the tail block's fields or None)
CASES = {
    # ---- logits forward
    "logits scalar mix": ("paella_unet_forward_shared", lambda c, o: FWD(c) + (1.5, -0.5, H, W, c.S, c.aw, 2, o.logits) + END(c),
                          lambda c, o: STEP(c, mix_c=1.5, mix_u=-0.5, attn_weights=c.aw, n_attn_weights=2, logits_out=o.logits), None),
    "logits unmixed": ("paella_unet_forward_shared", lambda c, o: FWD(c) + (0.0, 0.0, H, W, c.S, None, 0, o.logits) + END(c), lambda c, o: STEP(c, logits_out=o.logits), None),
    "logits pair table": ("paella_unet_forward_shared_req", lambda c, o: FWD(c) + (c.pairs, H, W, c.S, c.aw, 2, o.logits) + END(c),
                          lambda c, o: STEP(c, mix_pairs=c.pairs, attn_weights=c.aw, n_attn_weights=2, logits_out=o.logits), None),
    "logits ragged": ("paella_unet_forward_shared_ragged", lambda c, o: FWD(c) + (1.5, -0.5, H, W, c.S, c.lens, c.aw, 2, o.logits) + END(c),
                      lambda c, o: STEP(c, mix_c=1.5, mix_u=-0.5, cond_len=c.lens, attn_weights=c.aw, n_attn_weights=2, logits_out=o.logits), None),
    "logits pair table ragged": ("paella_unet_forward_shared_req_ragged", lambda c, o: FWD(c) + (c.pairs, H, W, c.S, c.lens, None, 0, o.logits) + END(c),
                                 lambda c, o: STEP(c, mix_pairs=c.pairs, cond_len=c.lens, logits_out=o.logits), None),
    "logits key weights": ("paella_unet_forward_shared_req_kw", lambda c, o: FWD(c) + (c.pairs, H, W, c.S, c.lens) + KW(c) + (o.logits,) + END(c),
                           lambda c, o: STEP(c, mix_pairs=c.pairs, cond_len=c.lens, logits_out=o.logits, **KWB(c)), None),
    "logits key groups": ("paella_unet_forward_shared_req_rg", lambda c, o: FWD(c) + (c.pairs, H, W, c.S, c.lens) + KW(c) + RG(c) + (o.logits,) + END(c),
                          lambda c, o: STEP(c, mix_pairs=c.pairs, cond_len=c.lens, logits_out=o.logits, **KWB(c), **RGB(c)), None),
    # ---- fused step
    "fused scalar": ("paella_unet_forward_sample", lambda c, o: FWD(c) + (1.5, -0.5, H, W, c.S, c.aw, 2) + SCAL(c) + (o.tok,) + END(c),
                     lambda c, o: STEP(c, mix_c=1.5, mix_u=-0.5, attn_weights=c.aw, n_attn_weights=2), lambda c, o: SCALB(c, o)),
    "fused scalar ragged": ("paella_unet_forward_sample_ragged", lambda c, o: FWD(c) + (1.5, -0.5, H, W, c.S, c.lens, None, 0) + SCAL(c) + (o.tok,) + END(c),
                            lambda c, o: STEP(c, mix_c=1.5, mix_u=-0.5, cond_len=c.lens), lambda c, o: SCALB(c, o)),
    "fused scalar pin": ("paella_unet_forward_sample_pin", lambda c, o: FWD(c) + (1.5, -0.5, H, W, c.S, c.lens, None, 0) + SCAL(c) + (c.keep, c.known, o.tok) + END(c),
                         lambda c, o: STEP(c, mix_c=1.5, mix_u=-0.5, cond_len=c.lens), lambda c, o: SCALB(c, o, pin_keep=c.keep, pin_tokens=c.known)),
    "fused request": ("paella_unet_forward_sample_req", lambda c, o: FWD(c) + (c.pairs, H, W, c.S, c.aw, 2) + REQ(c) + (2, c.init, 0.4, o.tok) + END(c),
                      lambda c, o: STEP(c, mix_pairs=c.pairs, attn_weights=c.aw, n_attn_weights=2), lambda c, o: REQB(c, o, offset=2, t_next=0.4)),
    "fused request ragged": ("paella_unet_forward_sample_req_ragged", lambda c, o: FWD(c) + (c.pairs, H, W, c.S, c.lens, None, 0) + REQ(c) + (2, c.init, 0.4, o.tok) + END(c),
                             lambda c, o: STEP(c, mix_pairs=c.pairs, cond_len=c.lens), lambda c, o: REQB(c, o, offset=2, t_next=0.4)),
    "fused request key weights": ("paella_unet_forward_sample_req_kw",
                                  lambda c, o: FWD(c) + (c.pairs, H, W, c.S, c.lens) + KW(c) + REQ(c) + (2, c.init, 0.4) + PIN3(c) + (o.tok,) + END(c),
                                  lambda c, o: STEP(c, mix_pairs=c.pairs, cond_len=c.lens, **KWB(c)), lambda c, o: REQB(c, o, offset=2, t_next=0.4, **PIN3B(c))),
    "fused stream": ("paella_unet_forward_sample_stream", lambda c, o: FWD(c) + (c.pairs, H, W, c.S, c.aw, 2) + REQ(c) + STRM(c) + (o.tok,) + END(c),
                     lambda c, o: STEP(c, mix_pairs=c.pairs, attn_weights=c.aw, n_attn_weights=2), lambda c, o: REQB(c, o, **STRMB(c))),
    "fused stream ragged": ("paella_unet_forward_sample_stream_ragged", lambda c, o: FWD(c) + (c.pairs, H, W, c.S, c.lens, None, 0) + REQ(c) + STRM(c) + (o.tok,) + END(c),
                            lambda c, o: STEP(c, mix_pairs=c.pairs, cond_len=c.lens), lambda c, o: REQB(c, o, **STRMB(c))),
    "fused stream pin": ("paella_unet_forward_sample_stream_pin", lambda c, o: FWD(c) + (c.pairs, H, W, c.S, c.lens, None, 0) + REQ(c) + STRM(c) + PIN3(c) + (o.tok,) + END(c),
                         lambda c, o: STEP(c, mix_pairs=c.pairs, cond_len=c.lens), lambda c, o: REQB(c, o, **STRMB(c), **PIN3B(c))),
    "fused stream key weights": ("paella_unet_forward_sample_stream_kw",
                                 lambda c, o: FWD(c) + (c.pairs, H, W, c.S, c.lens) + KW(c) + REQ(c) + STRM(c) + (None, None, None, o.tok) + END(c),
                                 lambda c, o: STEP(c, mix_pairs=c.pairs, cond_len=c.lens, **KWB(c)), lambda c, o: REQB(c, o, **STRMB(c))),
    "fused stream key groups": ("paella_unet_forward_sample_stream_rg",
                                lambda c, o: FWD(c) + (c.pairs, H, W, c.S, c.lens) + KW(c) + RG(c) + REQ(c) + STRM(c) + PIN3(c) + (o.tok,) + END(c),
                                lambda c, o: STEP(c, mix_pairs=c.pairs, cond_len=c.lens, **KWB(c), **RGB(c)), lambda c, o: REQB(c, o, **STRMB(c), **PIN3B(c))),
    # ---- materialised tail
    "tail explicit noise": ("paella_sample_tail", lambda c, o: TAIL(c) + (0.8, 0, c.noise_q, 0, 0, c.init, c.mask_u, 0.4, o.tok, o.pre, c.stream), None,
                            lambda c, o: TAILB(c, temperature=0.8, noise_q=c.noise_q, init_noise=c.init, mask_u=c.mask_u, t_next=0.4, tokens_out=o.tok, sampled_out=o.pre)),
    "tail argmax": ("paella_sample_tail", lambda c, o: TAIL(c) + (1.0, 1, None, 0, 0, None, None, 0.0, o.tok, o.pre, c.stream), None,
                    lambda c, o: TAILB(c, temperature=1.0, mode=1, tokens_out=o.tok, sampled_out=o.pre)),
    "tail philox": ("paella_sample_tail_ex", lambda c, o: TAIL(c) + (0.8, 0, None, 77, c.seed_dev, 2, 3 * HW, c.row_dev, c.init, None, 0.4, o.tok, o.pre, c.stream), None,
                    lambda c, o: TAILB(c, sampled_out=o.pre, **SCALB(c, o))),
    "tail pin": ("paella_sample_tail_pin", lambda c, o: TAIL(c) + SCAL(c) + (c.keep, c.known, o.tok, o.pre, c.stream), None,
                 lambda c, o: TAILB(c, sampled_out=o.pre, pin_keep=c.keep, pin_tokens=c.known, **SCALB(c, o))),
    "tail filter": ("paella_sample_tail_filter", lambda c, o: TAIL(c) + SCAL(c) + (c.keep, c.known, 7, 0.6, 1.0, 2, o.tok, o.pre, c.stream), None,
                    lambda c, o: TAILB(c, sampled_out=o.pre, pin_keep=c.keep, pin_tokens=c.known, top_k=7, top_p=0.6, typical_mass=1.0, min_tokens=2, **SCALB(c, o))),
    "tail statistics": ("paella_sample_tail_stats", lambda c, o: TAIL(c) + SCAL(c) + (None, None, 0, 1.0, 0.7, 1, o.tok, o.pre, o.lp, o.ent, c.stream), None,
                        lambda c, o: TAILB(c, sampled_out=o.pre, top_k=0, top_p=1.0, typical_mass=0.7, min_tokens=1, logprob_out=o.lp, entropy_out=o.ent, **SCALB(c, o))),
    "tail request": ("paella_sample_tail_req", lambda c, o: RTAIL(c) + (2, c.init, 0.4, o.tok, o.pre, c.stream), None, lambda c, o: RTAILB(c, o, offset=2, t_next=0.4)),
    "tail stream": ("paella_sample_tail_stream", lambda c, o: RTAIL(c) + STRM(c) + (o.tok, o.pre, c.stream), None, lambda c, o: RTAILB(c, o, **STRMB(c))),
    "tail stream pin": ("paella_sample_tail_stream_pin", lambda c, o: RTAIL(c) + STRM(c) + PIN3(c) + (o.tok, o.pre, c.stream), None,
                        lambda c, o: RTAILB(c, o, **STRMB(c), **PIN3B(c))),
    "tail stream filter": ("paella_sample_tail_stream_filter", lambda c, o: RTAIL(c) + STRM(c) + PIN3(c) + (c.filter_k, c.filter_mass, o.tok, o.pre, c.stream), None,
                           lambda c, o: RTAILB(c, o, filter_k=c.filter_k, filter_mass=c.filter_mass, **STRMB(c), **PIN3B(c))),
    "tail stream statistics": ("paella_sample_tail_stream_stats",
                               lambda c, o: RTAIL(c) + STRM(c) + (None, None, None, c.filter_k, c.filter_mass, o.tok, o.pre, o.lp, o.ent, c.stream), None,
                               lambda c, o: RTAILB(c, o, filter_k=c.filter_k, filter_mass=c.filter_mass, logprob_out=o.lp, entropy_out=o.ent, **STRMB(c))),
}


@pytest.mark.parametrize("case", list(CASES))
def test_block_equals_the_fixed_form_entry_point(ctx, case):
    c = ctx
    name, legacy_args, step_fields, tail_fields = CASES[case]
    a, b = _outputs(c), _outputs(c)
    _lib.check(getattr(c.lib, name)(*[_lib.ptr(v) if torch.is_tensor(v) else v for v in legacy_args(c, a)]))
    tail = None if tail_fields is None else _fill(_lib.TailArgs(), tail_fields(c, b))
    if step_fields is None:
        _lib.check(c.lib.paella_sample_tail_args(ctypes.byref(tail), ctypes.sizeof(tail), c.stream))
    else:
        step = _fill(_lib.StepArgs(), step_fields(c, b))
        if tail is not None:
            step.tail = ctypes.pointer(tail)
        _lib.check(c.lib.paella_unet_step(c.h, ctypes.byref(step), ctypes.sizeof(step), _lib.ptr(c.ws), c.ws.numel(), c.stream))
    torch.cuda.synchronize()
    written = 0
    for field in ("tok", "pre", "logits", "lp", "ent"):
        got, want = getattr(b, field), getattr(a, field)
        bits = torch.int64 if got.dtype == torch.int64 else torch.int32  # floats by bit pattern: exact, and a NaN statistic equals itself
        assert torch.equal(got.view(bits), want.view(bits)), "%s: %d of %d values of `%s` differ between the block and %s" % (
            case, int((got.view(bits) != want.view(bits)).sum()), got.numel(), field, name)
        written += int((want != FILL).sum())
    assert written > 0, "%s: the fixed-form entry point stored nothing" % case
    if "stream" in case:  # the inactive slot (sample 1) keeps what its rows held, the active one does not
        assert bool((a.tok[HW:] == FILL).all()) and bool((a.tok[:HW] != FILL).all())
