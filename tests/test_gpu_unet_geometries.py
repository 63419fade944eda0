"""GPU: the UNet against fp64 beyond the shipped geometries (tests/unet_cases.py): one to four levels, widths 32 ... 256 that are multiples of 8 only or shrink
going down, attention at level 0, head widths 16 ... 128, every block order the plan treats differently, patch 1, no TimestepBlock, no AttnBlock, grids where a
16-row block straddles two samples -- in eval mode (the HIP engine) and in train mode (the four training switches on "hip").

Eval mode, every float tensor compared with fp64: with e_hip = max|HIP - fp64| and e_cpu = max|fp32 CPU oracle - fp64| on the same inputs,
    e_hip <= max(4 * e_cpu, 2^-21 * max|ref|)
(tests/test_gpu_vqgan_geometries.py: 4 is the project's margin for another accumulation order, the floor of 4 ulp keeps a lucky e_cpu from failing a correct kernel),
for the whole tensor and for every sample on its own, so that a wrong sample cannot hide behind another sample's max|ref|.  Both references receive the fp32
timestep embedding (tests/unet_cases.py); the embedding itself is held to the same rule in test_timestep_embedding.  Every comparison prints one PARITY line
(profiles/unet_geometry_parity.txt is that output).

Train mode: tests/train_op_checks.py's step against the fp64 mirror of tests/train_step_model.py under the rule of tests/test_gpu_train_step_dropout.py,
e <= 4 max(e32, eT, ulp), plus what `run_level` must ask of `timestep_modulate` for the case's block order (tests/unet_cases.modulation_plan)."""
import math

import pytest
import torch

import paella_amd
from paella_amd import _lib, training
from paella_amd import modules as modules_module
from tests import train_op_checks as T
from tests import unet_cases as U
from tests.helpers import argmax_report, to_dev

pytestmark = pytest.mark.gpu
DEV = "cuda"
TAIL, PATTERN = 4096, 0xA5
HIP4 = ("hip", "hip", "hip", "hip")


def _parity(case, what, got, f64, f32, per_sample=True):
    """the module docstring's rule on the whole tensor and on every sample (dim 0): one PARITY line each -> list of failure messages"""
    fails = []
    assert tuple(got.shape) == tuple(f64.shape), "%s %s: shape %s, expected %s" % (case, what, tuple(got.shape), tuple(f64.shape))
    assert torch.isfinite(got).all(), "%s %s: non-finite output" % (case, what)
    parts = [("", slice(None))] + ([("[%d]" % b, slice(b, b + 1)) for b in range(f64.size(0))] if per_sample and f64.size(0) > 1 else [])
    for tag, sl in parts:
        ref = f64[sl].double()
        e_hip = float((got[sl].double().cpu() - ref).abs().max())
        e_cpu = float((f32[sl].double() - ref).abs().max())
        bound = max(4.0 * e_cpu, 2.0 ** -21 * float(ref.abs().max()))
        print("PARITY %-12s %-22s max|ref| %9.3e  e_cpu %9.3e  e_hip %9.3e  e_hip/e_cpu %6.2f  bound %9.3e  e_hip/bound %5.2f"
              % (case, what + tag, float(ref.abs().max()), e_cpu, e_hip, e_hip / e_cpu if e_cpu else float("inf"), bound, e_hip / bound))
        if not e_hip <= bound:
            fails.append("%s %s%s: e_hip %.3e > max(4 * e_cpu %.3e, floor) = %.3e" % (case, what, tag, e_hip, e_cpu, bound))
    return fails


class _NanTorch:
    """torch, as paella_amd/modules.py sees it, with empty returning NaN-filled tensors (ints: the most negative value)"""

    def __getattr__(self, attr):
        return getattr(torch, attr)

    def empty(self, *a, **k):
        t = torch.empty(*a, **k)
        return t.fill_(float("nan")) if t.is_floating_point() else t.fill_(torch.iinfo(t.dtype).min if t.dtype != torch.uint8 else 0xFF)


def _nan_filled_outputs(monkeypatch):
    """The wrapper allocates its outputs (and the conditioning cache) with torch.empty; inside paella_amd.modules they now come back pre-filled with NaN, so a
    kernel that leaves part of an output unwritten cannot pass by luck."""
    monkeypatch.setattr(modules_module, "torch", _NanTorch())


@pytest.fixture(scope="module")
def models(built_lib):
    """the case's network on the device, built once per module (eval mode: the HIP engine)"""
    made = {}

    def get(name):
        if name not in made:
            made[name] = U.new_model(name)[0].to(DEV)
        return made[name]

    yield get
    made.clear()
    torch.cuda.empty_cache()


def _dev_inputs(r):
    return r["x"].to(DEV), r["r"].to(DEV), to_dev(r["cond"], DEV), to_dev(r["uncond"], DEV)


def _both(c, u):
    """the conditional and the unconditional set as one conditioning batch of 2B rows, conditional rows first"""
    out = {}
    for k in c:
        if c[k] is None:
            out[k] = None
        elif isinstance(c[k], (list, tuple)):
            out[k] = [torch.cat([a, b]) for a, b in zip(c[k], u[k])]
        else:
            out[k] = torch.cat([c[k], u[k]])
    return out


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------------
# the timestep embedding on its own: the whole-network comparisons receive it as an input
# ---------------------------------------------------------------------------------------------------------------------
R_VALUES = {1: [0.37], 5: [0.0, 1.0, 0.001, 0.123456789, 0.9999]}


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("c_r", [8, 16, 17, 64])
def test_timestep_embedding(built_lib, monkeypatch, c_r, B):
    """m.gen_r_embedding(r) (the engine) and paella_amd.training.r_embedding on the device against fp64 sin / cos of the fp32 angle fl(fl(r * 1e4) * freq32);
    yardstick: torch's CPU fp32 sin / cos of the same angles.  r = 0, 1, 0.001 and values whose product with 1e4 is inexact; for odd c_r the pad column is 0."""
    r = torch.tensor(R_VALUES[B], dtype=torch.float32)
    assert bool(((r.double() * 10000.0) != (r * 10000.0).double()).any())
    half = c_r // 2
    freqs = torch.arange(half).float().mul(-math.log(10000) / (half - 1)).exp()
    angle = (r * 10000)[:, None] * freqs[None, :]                      # fp32: the two roundings every fp32 route makes
    assert angle.dtype == torch.float32 and float(angle.max()) <= 10000.0
    pad = [torch.zeros(B, 1)] if c_r % 2 else []
    f64 = torch.cat([angle.double().sin(), angle.double().cos()] + [p.double() for p in pad], dim=1)
    f32 = torch.cat([angle.sin(), angle.cos()] + pad, dim=1)
    m = paella_amd.Paella(c_in=4, c_out=4, num_labels=16, c_r=c_r, patch_size=1, c_cond=8, c_hidden=[8], nhead=[-1], blocks=[1], level_config=["T"], clip_embd=8,
                          byt5_embd=8, clip_seq_len=1).to(DEV)
    _nan_filled_outputs(monkeypatch)
    routes = {"engine": m.gen_r_embedding(r.to(DEV)), "training": training.r_embedding(r.to(DEV), c_r)}
    fails = []
    for route, got in routes.items():
        assert got.dtype == torch.float32
        fails += _parity("c_r=%d B=%d" % (c_r, B), "r_embed " + route, got, f64, f32, per_sample=False)
        if c_r % 2:
            assert bool((got[:, -1] == 0).all()), "%s: the pad column of an odd c_r is not exactly 0" % route
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------------------------------------------------
# eval mode: the engine
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", U.CASE_NAMES)
def test_forward_vs_fp64(models, monkeypatch, name):
    """m(x, r, **c) into a NaN-filled output against fp64: every logit finite and under the rule, whole and sample by sample; argmax equal to the fp64 argmax
    except at counted near-ties; a second call returns the same bits; gen_c_embeddings under the same rule."""
    r = U.reference(name)
    m = models(name)
    x, rr, c, _ = _dev_inputs(r)
    _nan_filled_outputs(monkeypatch)
    with torch.no_grad():
        got = m(x, rr, **c)
        again = m(x, rr, **c)
        c_embed = m.gen_c_embeddings(c["byt5"], c["clip"], c["clip_image"])
    torch.cuda.synchronize()
    f64, f32 = r["f64"], r["f32"]
    fails = _parity(name, "logits", got, f64["logits_c"], f32["logits_c"])
    fails += _parity(name, "c_embed", c_embed, f64["c_embed_c"], f32["c_embed_c"])
    clear, near_mism, n_near = argmax_report(f64["logits_c"], got.cpu().double())
    print("PARITY %-12s argmax                 %d of %d positions differ from fp64 with a clear margin, %d at the %d near-ties (margin < %g)"
          % (name, clear, r["near"].numel(), near_mism, n_near, U.NEAR_TIE_EPS))
    assert n_near == int(r["near"].sum()) and n_near <= U.NEAR_TIE_CAP * r["near"].numel()
    assert clear == 0, "%s: %d argmax positions differ from fp64 where the margin is clear" % (name, clear)
    assert torch.equal(_bits(got), _bits(again)), "%s: a second call returned other bits" % name
    assert not fails, "\n".join(fails)


def _exact_workspace(m, B, H, W, S):
    """workspace_bytes + TAIL bytes, all PATTERN, header initialised on the first workspace_bytes only: (the exact-size view, the tail view)"""
    n = m.workspace_bytes(B, H, W, S)
    buf = torch.full((n + TAIL,), PATTERN, dtype=torch.uint8, device=DEV)
    _lib.check(_lib.load().paella_workspace_init(_lib.ptr(buf), n, _lib.stream_ptr(buf.device)))
    return buf[:n], buf[n:]


@pytest.mark.parametrize("name", U.CASE_NAMES)
def test_shared_prefix_mix_and_exact_workspace(models, monkeypatch, name):
    """cache = prepare_cond of the conditional and the unconditional set together (2B rows).  forward_prepared(x2, r2, cache) evaluates 2B rows, and
    forward_prepared(x, r, cache) runs the conditioning-independent prefix once for the B distinct rows and replicates where the paths diverge: each under the rule
    against the fp64 logits of the 2B rows; cfg_mix = (8, -7) against 8 l_c - 7 l_u of the fp64 logits, with the same mix of the fp32 oracle's logits as e_cpu.
    Then all of it again in a workspace of exactly workspace_bytes with a patterned tail: the same bits, and the tail untouched."""
    r = U.reference(name)
    m = models(name)
    B, H, W = r["B"], r["H"], r["W"]
    x, rr, c, u = _dev_inputs(r)
    both = _both(c, u)
    x2, r2 = torch.cat([x, x]), torch.cat([rr, rr])
    f64 = torch.cat([r["f64"]["logits_c"], r["f64"]["logits_u"]])
    f32 = torch.cat([r["f32"]["logits_c"], r["f32"]["logits_u"]])
    mix64 = 8.0 * r["f64"]["logits_c"] - 7.0 * r["f64"]["logits_u"]
    mix32 = 8.0 * r["f32"]["logits_c"] - 7.0 * r["f32"]["logits_u"]
    _nan_filled_outputs(monkeypatch)

    def run(ws=None):
        with torch.no_grad():
            cache = m.prepare_cond(ws=ws, **both)
            # the shared prefix first: what it does not replicate is then whatever the workspace held (the pattern, in the exact-size run), not the 2B-row run's rows
            shared = m.forward_prepared(x, rr, cache, ws=ws).clone()
            full = m.forward_prepared(x2, r2, cache, ws=ws).clone()
            mixed = m.forward_prepared(x, rr, cache, cfg_mix=(8.0, -7.0), ws=ws).clone()
        return cache, dict(full=full, shared=shared, mixed=mixed)

    cache, got = run()
    torch.cuda.synchronize()
    assert cache.B == 2 * B
    fails = _parity(name, "2B rows", got["full"], f64, f32)
    fails += _parity(name, "shared prefix", got["shared"], f64, f32)
    fails += _parity(name, "cfg_mix (8, -7)", got["mixed"], mix64, mix32)
    if name == "no_attention":  # nothing reads the conditioning: both halves are the B-row evaluation, bit for bit
        with torch.no_grad():
            plain = m(x, rr, **c)
        for k in ("full", "shared"):
            assert torch.equal(_bits(got[k][:B]), _bits(got[k][B:])) and torch.equal(_bits(got[k][:B]), _bits(plain)), k
    else:
        for k in ("full", "shared"):
            assert not torch.equal(got[k][:B], got[k][B:]), "%s %s: the conditional and the unconditional half are equal" % (name, k)
    ws, tail = _exact_workspace(m, 2 * B, H, W, cache.S)
    _, again = run(ws)
    torch.cuda.synchronize()
    for k in got:
        assert torch.equal(_bits(again[k]), _bits(got[k])), "%s: %s differs with a workspace of exactly workspace_bytes" % (name, k)
    assert bool((tail == PATTERN).all()), "%s: %d byte(s) past workspace_bytes were written" % (name, int((tail != PATTERN).sum()))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("name", U.CASE_NAMES)
def test_bf16_mode(built_lib, monkeypatch, name):
    """The bf16 mode on the same inputs.  It is outside the parity contract, so no parity claim: the checks of tests/test_gpu_fastmode.py's
    test_bf16_forward_deviation_and_restore -- finite, run-to-run identical, max|diff| <= 0.08 max(1, std), and the exact bits back after the switch; the flip rate
    is printed, not asserted (as few as 48 positions).  `changed` holds where a block's own contraction has K % 64 == 0 (include/paella_hip.h,
    paella_unet_set_precision): a block of a width that is a multiple of 64, a down-sampler with 4 c_from % 64 == 0, the head with c_out % 64 == 0 -- the embedding
    GEMM and the conditioning mappers stay fp32 in either mode.  Where the configuration has none of them the mode must be the exact path, bit for bit."""
    r = U.reference(name)
    cfg = r["cfg"]
    m = U.new_model(name)[0].to(DEV)      # its own model: the switch must not leak into the module fixture
    x, rr, c, _ = _dev_inputs(r)
    _nan_filled_outputs(monkeypatch)
    with torch.no_grad():
        exact = m(x, rr, **c).clone()
        try:
            m.set_gemm_precision("bf16")
            assert m.get_gemm_precision() == "bf16"
            fast = m(x, rr, **c).clone()
            fast2 = m(x, rr, **c).clone()
        finally:
            m.set_gemm_precision("fp32")
        back = m(x, rr, **c)
    torch.cuda.synchronize()
    diff, std = float((fast - exact).abs().max()), float(exact.std())
    flips = float((fast.argmax(1) != exact.argmax(1)).float().mean())
    n = len(cfg["c_hidden"])
    served = any(w % 64 == 0 for w in cfg["c_hidden"]) or any((4 * cfg["c_hidden"][i - 1]) % 64 == 0 for i in range(1, n)) or cfg["c_out"] % 64 == 0
    print("PARITY %-12s bf16 mode              served %s  argmax-flip rate %.4f  max|logit diff| %.3e on logits of std %.3f" % (name, served, flips, diff, std))
    assert torch.isfinite(fast).all()
    assert torch.equal(_bits(fast), _bits(fast2))
    assert served == (not torch.equal(fast, exact)), "%s: bf16 mode %s the logits" % (name, "did not change" if served else "changed")
    assert diff <= 0.08 * max(1.0, std)
    assert torch.equal(_bits(back), _bits(exact)), "%s: the exact path is not back after set_gemm_precision('fp32')" % name


# ---------------------------------------------------------------------------------------------------------------------
# refusals: one per kind, with the library's message, before anything is enqueued
# ---------------------------------------------------------------------------------------------------------------------
def test_grid_that_does_not_divide_is_refused(models):
    """four_levels needs a multiple of 2 << 3 = 16 tokens per side: a 16 x 24 grid is refused by the forward, the NaN-filled output stays NaN, and the model
    serves the next call"""
    name = "four_levels"
    r = U.reference(name)
    m = models(name)
    B = r["B"]
    x, rr, c, _ = _dev_inputs(r)
    with torch.no_grad():
        cache = m.prepare_cond(**c)
        out = torch.full((B, 16, 24, r["cfg"]["num_labels"]), float("nan"), device=DEV)
        with pytest.raises(_lib.PaellaHipError, match="token grid 16x24 must be a positive multiple of 16"):
            m.forward_prepared(x[:, :, :24].contiguous(), rr, cache, out=out)
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), "a refused forward wrote to its output"
        ok = m.forward_prepared(x, rr, cache)
    assert torch.isfinite(ok).all()


@pytest.mark.parametrize("change,message", [(dict(c_hidden=[44]), "must be a multiple of 8"), (dict(nhead=[2]), "head_dim must be a multiple of 16")],
                         ids=["width-44", "head-width-24"])
def test_create_refuses_unsupported_configurations(built_lib, change, message):
    """one_level with a width that is no multiple of 8, and with nhead giving a head width of 24: refused when the engine is created, not later"""
    cfg = dict(U.CASES["one_level"]["cfg"], **change)
    m = paella_amd.Paella(**cfg).to(DEV)
    with pytest.raises(_lib.PaellaHipError, match=message):
        m._engine()
    assert m._handle is None


# ---------------------------------------------------------------------------------------------------------------------
# train mode: the four switches
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def train_cases(built_lib):
    made = {}

    def get(name):
        if name not in made:
            with T.deterministic_torch():      # eT, the torch route's error, is measured in the mode the steps run in
                made[name] = T.Case(name, dict(U.CASES[name], dropout=0.1))
        return made[name]

    yield get
    made.clear()
    torch.cuda.empty_cache()


class _Modulations:
    """While it is entered, every call of paella_amd.training.timestep_modulate is recorded as (residual given, LayerNorm rows asked for)"""

    def __enter__(self):
        self.calls, self.real = [], training.timestep_modulate

        def counting(x, ab, residual=None, layernorm=False, eps=1e-6):
            self.calls.append((residual is not None, bool(layernorm)))
            return self.real(x, ab, residual, layernorm, eps)

        training.timestep_modulate = counting
        return self

    def __exit__(self, *exc):
        training.timestep_modulate = self.real
        return False


@pytest.mark.parametrize("p", [0.0, 0.1], ids=["dropout-0", "dropout-0.1"])
@pytest.mark.parametrize("name", U.CASE_NAMES)
def test_train_step_with_all_four_switches(train_cases, name, p):
    """One step with injected seeds and all four switches on "hip", as model(...) + CrossEntropyLoss and as forward_loss, against the fp64 mirror under the ops' CPU
    masks: logits (per-position loss) and every gradient under the yardstick rule, the loss to rtol 2e-5, the library calls against the mirror's call plan, and the
    timestep_modulate calls against the plan derived from level_config.  At dropout 0.1, dropout visibly moves more than 90 % of the gradients.

    The steps run under torch's deterministic mode (train_op_checks.deterministic_torch), as test_step_with_default_seeds of tests/test_gpu_train_step_dropout.py
    does, and a second step under the same seeds must return the same bits.  In torch's default mode the same step differs from run to run, and at a level of one
    position per sample with B = 1 (no_timestep, down_blocks.2.1.channelwise.0.bias: that gradient is one row) it sat at 2.1 ... 4.3 x the yardstick over 36
    same-seed repeats; the activation op's own du on the captured inputs of that call is within its op rule (1.1e-9 against the torch chain's 3.0e-9), the excess
    arrives in dz, and in the deterministic mode the ratio is 0.78 in every repeat."""
    case = train_cases(name)
    cfg = case.cfg
    p_of_level = [p] * len(cfg["c_hidden"])
    seeds = T.injected(case) if p > 0 else []
    plan = U.modulation_plan(cfg)
    mods0 = training.MOD_COUNTERS["calls"]
    try:
        mode = T.deterministic_torch()
        mode.__enter__()
        with _Modulations() as mods:
            out = T.run_step(case, HIP4, dropout=p, seeds=iter(seeds))
        again = T.run_step(case, HIP4, dropout=p, seeds=iter(seeds))["values"]
        assert out["values"].keys() == again.keys()
        for k, v in out["values"].items():
            assert torch.equal(v, again[k]), "%s: a second step under the same seeds returned other bits in %s" % (name, k)
        mods0 += len(plan)
        assert mods.calls == plan, "%s: timestep_modulate was asked for %s, the block order needs %s" % (name, mods.calls, plan)
        assert training.MOD_COUNTERS["calls"] == mods0 + len(plan)
        ref = T.assert_step_against_mirror(case, out, seeds, "all four switches, dropout %g" % p, label="unet_geometry train parity", p_of_level=p_of_level)
        if p > 0:
            assert len(seeds) >= 3
            _, e32, _ = case.mirror(seeds, p_of_level)
            moved = [k for k in case.names if T.err(case.ref0[k], ref[k]) > 10 * T.FACTOR * max(e32[k], case.eT[k], T.ulp(ref[k]))]
            assert len(moved) > 0.9 * len(case.names), "dropout moved only %d of %d gradients clearly" % (len(moved), len(case.names))
        if cfg["c_out"] % 16 or cfg["num_labels"] % 16:
            # the fused loss head takes c_out and num_labels that are multiples of 16 (paella_amd/train_ops.py: refuse_head_widths): such a network trains through
            # model(...) + CrossEntropyLoss above, and forward_loss refuses it with the op's message BEFORE the network runs -- no seed is drawn, no op is called
            handed, mods1 = iter(seeds), training.MOD_COUNTERS["calls"]
            with pytest.raises(ValueError, match="the fused head takes a multiple of 16"):
                T.run_step(case, HIP4, dropout=p, seeds=handed, fused_loss=True)
            assert list(handed) == seeds and training.MOD_COUNTERS["calls"] == mods1, "the refused forward_loss ran part of the network"
            return
        with _Modulations() as mods:
            out = T.run_step(case, HIP4, dropout=p, seeds=iter(seeds), fused_loss=True)
        assert mods.calls == plan
        ref = T.assert_step_against_mirror(case, out, seeds, "forward_loss, dropout %g" % p, keys=case.names + [T.PER_POS], label="unet_geometry train parity",
                                           p_of_level=p_of_level)
        top2 = ref[T.LOGITS].topk(2, dim=1).values
        near = (top2[:, 0] - top2[:, 1]) < U.NEAR_TIE_EPS
        mism = out["correct"].cpu() != (ref[T.LOGITS].argmax(1) == case.inp[0])
        print("unet_geometry train parity %s forward_loss, dropout %g: `correct` differs at %d positions with a clear margin and %d of %d near-ties"
              % (name, p, int((mism & ~near).sum()), int((mism & near).sum()), int(near.sum())))
        assert out["correct"].dtype == torch.bool and int((mism & ~near).sum()) == 0
    finally:
        mode.__exit__(None, None, None)
        case.m.set_training_modulation("torch")
        case.m.eval()


def test_eval_after_the_train_steps_is_the_engine(train_cases):
    """after train-mode steps on a geometry off the shipped family, eval-mode logits are finite and under the rule: the engine never sees the switches"""
    name = "orders"
    case = train_cases(name)
    T.run_step(case, HIP4, dropout=0.1, seeds=iter(T.injected(case)))
    case.m.set_training_modulation("torch")
    r = U.reference(name)
    x, rr, c, _ = _dev_inputs(r)
    with torch.no_grad(), T.Harness() as h:
        got = case.m(x, rr, **c)
    assert not h.lib_calls, "eval mode reached a training op"
    assert not case.m.training
    fails = _parity(name, "logits after training", got, r["f64"]["logits_c"], r["f32"]["logits_c"])
    assert not fails, "\n".join(fails)
