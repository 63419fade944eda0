"""GPU: the training timestep modulation (paella_amd/csrc/mod_train.hip) against the fp64 model of tests/mod_ln_model.py.

The yardstick of every accuracy check is MEASURED in the same test, as tests/test_gpu_dwconv_train.py does: the torch fp32 chain the network runs by default (the add,
the chunk, x (1 + a) + b, F.layer_norm, backward with the same dx' and dz) runs on the same device and inputs, its max abs error against the fp64 model is taken for
each of x', z, dx and dab, and the fused op must stay within 4x max(that error, one fp32 ulp at the model's largest magnitude) -- train_op_checks.within_yardstick.
The measured pairs are kept in profiles/train_modulation_parity.txt."""
import functools
import itertools

import pytest
import torch
import torch.nn.functional as F

from paella_amd import _lib, training
from tests import mod_ln_model as M
from tests import train_op_checks as T
from tests.test_gpu_training import _train_step

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 1e-6
# (B, H, W, C): one position of one vector; a row image of two samples; small; off every grain but 4 and five strips of positions; more than 256 vectors per row;
# the real level-2 width; three strips exactly (asserted from the documented workspace size in test_the_strip_case_spans_three_strips)
SHAPES = [(1, 1, 1, 4), (2, 1, 5, 8), (2, 3, 2, 24), (3, 5, 13, 136), (1, 8, 8, 1032), (2, 4, 4, 1280), (2, 5, 7, 16)]
STRIP_CASE = (2, 5, 7, 16)
CASES = [s + (res, ln) for s in SHAPES for res in (False, True) for ln in (False, True)]
ids = lambda c: "x".join(map(str, c[:4])) + ("-res" if c[4] else "") + ("-ln" if c[5] else "")


@functools.lru_cache(maxsize=None)
def _inputs(B, H, W, C, res=True):
    """rows [B, P, C] on the device: x, residual (or None), ab [B, 2C], dxp, dz"""
    gen = torch.Generator().manual_seed(1000000 * B + 10000 * H + 100 * W + C)
    r = lambda *s: torch.randn(*s, generator=gen)
    x, rs, ab, dxp, dz = r(B, H * W, C), r(B, H * W, C), r(B, 2 * C) * 0.5, r(B, H * W, C), r(B, H * W, C)
    return x.to(DEV), rs.to(DEV) if res else None, ab.to(DEV), dxp.to(DEV), dz.to(DEV)


def fused(x, res, ab, dxp=None, dz=None, ln=True, want=(True, True), poison=True):
    """the raw op on [B, P, C] rows: forward, and backward when a gradient is given -> dict of outputs.  Outputs and workspace start as NaN: they are WRITTEN, and
    the workspace needs no set-up."""
    lib = _lib.load()
    B, P, C = x.shape
    new = (lambda *sh: torch.full(sh, float("nan"), device=DEV)) if poison else (lambda *sh: torch.empty(sh, device=DEV))
    out = dict(xp=new(B, P, C), z=new(B, P, C) if ln else None, rstd=new(B, P) if ln else None)
    _lib.check(lib.paella_mod_ln_train_forward(_lib.ptr(x), _lib.ptr(res), _lib.ptr(ab), B, P, C, EPS, _lib.ptr(out["xp"]), _lib.ptr(out["z"]), _lib.ptr(out["rstd"]),
                                               None, 0, _lib.stream_ptr(x.device)))
    if dxp is not None or dz is not None:
        assert dz is None or ln
        ws = torch.empty(lib.paella_mod_ln_train_workspace_bytes(B, P, C, int(dz is not None)), dtype=torch.uint8, device=DEV)
        if poison:
            ws.fill_(255)
        out["dx"] = new(B, P, C) if want[0] else None
        out["dab"] = new(B, 2 * C) if want[1] else None
        _lib.check(lib.paella_mod_ln_train_backward(_lib.ptr(x), _lib.ptr(res), _lib.ptr(ab), _lib.ptr(out["z"]), _lib.ptr(out["rstd"]), _lib.ptr(dxp), _lib.ptr(dz),
                                                    B, P, C, _lib.ptr(out["dx"]), _lib.ptr(out["dab"]), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(x.device)))
    return out


def torch_chain(x, res, ab, dxp, dz):
    """the joint as torch runs it in fp32 by default ([B, P, C] rows in and out) -> (x', z, dx, dab); dz None: no LayerNorm"""
    xx, aa = x.clone().requires_grad_(True), ab.clone().requires_grad_(True)
    C = x.size(-1)
    a, b = aa[:, None, :].chunk(2, dim=-1)
    xp = (xx if res is None else xx + res) * (1 + a) + b
    if dz is None:
        xp.backward(dxp)
        return xp.detach(), None, xx.grad, aa.grad
    z = F.layer_norm(xp, (C,), None, None, EPS)
    torch.autograd.backward([xp, z], [dxp, dz])
    return xp.detach(), z.detach(), xx.grad, aa.grad


def _model(x, res, ab, dxp, dz):
    xp, z, _ = M.forward(x, ab, res, EPS)
    return (xp, z if dz is not None else None) + M.backward(x, ab, res, dxp, dz, EPS)


def _check_accuracy(tag, out, ref, model):
    pairs = []
    for name, b, m in zip(("xp", "z", "dx", "dab"), ref, model):
        if m is None:
            continue
        assert torch.isfinite(out[name]).all(), "%s: not finite" % name
        pairs.append((name, T.err(out[name], m), T.err(b, m), T.ulp(m)))
    print("train_modulation parity %s: " % tag + "  ".join("%s fused %.3e torch %.3e ulp %.3e" % q for q in pairs))
    for name, e_fused, e_torch, ulp in pairs:
        assert T.within_yardstick(e_fused, e_torch, ulp), "%s %s: fused error %.3e exceeds %gx max(torch fp32 chain %.3e, ulp %.3e)" % (tag, name, e_fused, T.FACTOR, e_torch, ulp)


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_accuracy_against_the_fp64_model(built_lib, case):
    """Measured pairs (fused / torch, MI355X): all of them in profiles/train_modulation_parity.txt."""
    x, res, ab, dxp, dz = _inputs(*case[:5])
    ln = case[5]
    dz = dz if ln else None
    out = fused(x, res, ab, dxp, dz, ln)
    _check_accuracy(ids(case), out, torch_chain(x, res, ab, dxp, dz), _model(x, res, ab, dxp, dz))
    if ln:  # rstd itself, loosely (z and the gradients above hold it to account)
        torch.testing.assert_close(out["rstd"].double(), M.forward(x, ab, res, EPS)[2], rtol=1e-4, atol=0)


def test_the_strip_case_spans_three_strips(built_lib):
    """include/paella_hip.h: without the LayerNorm the workspace is the partials alone, B x strips x 2C floats rounded up to 256 bytes"""
    B, H, W, C = STRIP_CASE
    per_strip = B * 2 * C * 4
    assert per_strip % 256 == 0
    assert _lib.load().paella_mod_ln_train_workspace_bytes(B, H * W, C, 0) // per_strip >= 3
    assert _lib.load().paella_mod_ln_train_workspace_bytes(B, 16, C, 0) == 256      # and a sample of one strip has none


@pytest.mark.parametrize("res", [False, True], ids=["plain", "res"])
def test_a_equal_to_minus_one(built_lib, res):
    """1 + a = 0 exactly on some channels: dx is exactly 0 there and da still agrees with the model -- a backward that divided by 1 + a would give inf or nan"""
    case = (2, 3, 2, 24, res)
    x, rs, ab, dxp, dz = _inputs(*case)
    ab = ab.clone()
    ab[:, 3:9] = -1.0
    out = fused(x, rs, ab, dxp, dz)
    assert torch.all(out["dx"][..., 3:9] == 0) and torch.all(out["dx"][..., :3] != 0)
    assert torch.all(out["xp"][..., 3:9] == ab[:, None, 24 + 3:24 + 9])
    _check_accuracy("a = -1 " + ids(case + (True,)), out, torch_chain(x, rs, ab, dxp, dz), _model(x, rs, ab, dxp, dz))


@pytest.mark.parametrize("res", [False, True], ids=["plain", "res"])
def test_constant_row(built_lib, res):
    """x = residual = 0 and one b for every channel: variance 0, z = 0 exactly, rstd = 1 / sqrt(eps), and finite gradients equal to the model's under the rule"""
    case = (2, 3, 2, 24, res)
    x, rs, ab, dxp, dz = _inputs(*case)
    x = torch.zeros_like(x)
    rs = None if rs is None else torch.zeros_like(rs)
    ab = ab.clone()
    ab[:, 24:] = 0.5
    out = fused(x, rs, ab, dxp, dz)
    assert torch.all(out["z"] == 0) and torch.all(out["xp"] == 0.5)
    torch.testing.assert_close(out["rstd"], torch.full_like(out["rstd"], 1000.0), rtol=1e-6, atol=0)
    model = _model(x, rs, ab, dxp, dz)
    assert torch.all(model[1] == 0)
    _check_accuracy("constant row " + ids(case + (True,)), out, torch_chain(x, rs, ab, dxp, dz), model)


@pytest.mark.parametrize("res", [False, True], ids=["plain", "res"])
def test_sample_independence(built_lib, res):
    """For a batch of 3, every output of a sample -- its row of dab included -- is the bits of a one-sample call on its slice"""
    x, rs, ab, dxp, dz = _inputs(3, 5, 13, 136, res)
    full = fused(x, rs, ab, dxp, dz)
    plain = fused(x, rs, ab, dxp, None, ln=False)
    for b in range(3):
        s = slice(b, b + 1)
        one = fused(x[s], None if rs is None else rs[s], ab[s], dxp[s], dz[s])
        for k in ("xp", "z", "rstd", "dx", "dab"):
            assert torch.equal(full[k][s], one[k]), (b, k)
        one = fused(x[s], None if rs is None else rs[s], ab[s], dxp[s], None, ln=False)
        for k in ("xp", "dx", "dab"):
            assert torch.equal(plain[k][s], one[k]), (b, k)


@pytest.mark.parametrize("case", [(3, 5, 13, 136, True), (2, 5, 7, 16, False), (1, 8, 8, 1032, True), (2, 4, 4, 1280, False)], ids=lambda c: ids(c + (True,)))
def test_null_arguments_and_determinism(built_lib, case):
    """(3, 5 x 13) and (2, 5 x 7): more than one strip, dab through the partials; the others: one strip, written by the summing kernel itself"""
    x, rs, ab, dxp, dz = _inputs(*case)
    for gin in itertools.product((dxp, None), (dz, None)):
        if gin[0] is None and gin[1] is None:      # refused: no gradient arrived, there is no backward (tests/test_mod_train.py)
            continue
        full = fused(x, rs, ab, *gin)
        again = fused(x, rs, ab, *gin, poison=False)
        for k in ("xp", "z", "rstd", "dx", "dab"):
            assert torch.isfinite(full[k]).all(), k   # the NaN the outputs and the workspace were filled with is gone
            assert torch.equal(full[k], again[k]), k
        for want in itertools.product((True, False), repeat=2):
            if all(want):
                continue
            part = fused(x, rs, ab, *gin, want=want)
            for k, on in zip(("dx", "dab"), want):
                assert (torch.equal(part[k], full[k]) if on else part[k] is None), (want, k)
    # a gradient that did not arrive is a gradient of zeros: the pass without dz (dx written by the summing kernel) gives the bits of the pass through the LayerNorm
    zeros = torch.zeros_like(dz)
    for a, b in (((dxp, None), (dxp, zeros)), ((None, dz), (zeros, dz))):
        fa, fb = fused(x, rs, ab, *a), fused(x, rs, ab, *b)
        assert torch.equal(fa["dx"], fb["dx"]) and torch.equal(fa["dab"], fb["dab"])
    # and the forward without the LayerNorm writes the same x'
    assert torch.equal(fused(x, rs, ab, ln=False)["xp"], fused(x, rs, ab)["xp"])


def test_offsets_past_4_gib(built_lib):
    """B = 1025 samples of 32 x 32 x 1024 fp32: the last sample starts at byte 2^32.  No residual, the LayerNorm on, no dx' -- the arithmetic of a sample depends
    neither on b nor on B: every output of the last sample is the bits of a one-sample call on its slice."""
    B, P, C = 1025, 32 * 32, 1024
    assert (B - 1) * P * C * 4 >= 2 ** 32
    gen = torch.Generator(device=DEV).manual_seed(5)
    big = one = x = dz = None
    try:
        x = torch.randn(B, P, C, device=DEV, generator=gen)
        dz = torch.randn(B, P, C, device=DEV, generator=gen)
        ab = torch.randn(B, 2 * C, device=DEV, generator=gen) * 0.5
        big = fused(x, None, ab, None, dz, poison=False)
        one = fused(x[B - 1:], None, ab[B - 1:], None, dz[B - 1:])
        for k in ("xp", "z", "rstd", "dx", "dab"):
            assert torch.isfinite(one[k]).all(), k
            assert torch.equal(big[k][B - 1:], one[k]), k
        # and the one-sample call is right (fp32 chain, loose: the accuracy tests hold the op to the fp64 model)
        rxp, rz, rdx, rdab = torch_chain(x[B - 1:], None, ab[B - 1:], torch.zeros_like(dz[B - 1:]), dz[B - 1:])
        torch.testing.assert_close(one["z"], rz, rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(one["dx"], rdx, rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(one["dab"], rdab, rtol=1e-3, atol=1e-3)
        # sample 0 and the samples around byte 2^31 are finite and differ from the last one
        assert torch.isfinite(big["z"][0]).all() and torch.isfinite(big["dx"][511:513]).all() and torch.isfinite(big["dab"]).all()
        assert not torch.equal(big["z"][0], one["z"][0])
    finally:
        del big, one, x, dz
        torch.cuda.empty_cache()


@pytest.mark.parametrize("res", [False, True], ids=["plain", "res"])
@pytest.mark.parametrize("ln", [False, True], ids=["noln", "ln"])
def test_autograd_function_and_saved_state(built_lib, res, ln):
    B, H, W, C = 3, 5, 13, 136
    P = H * W
    x, rs, ab, dxp, dz = _inputs(B, H, W, C, res)
    raw = fused(x, rs, ab, dxp, dz if ln else None, ln)
    nchw = lambda t: t.view(B, H, W, C).permute(0, 3, 1, 2)       # logical [B, C, H, W] over NHWC memory
    xx = nchw(x.clone()).requires_grad_(True)
    rr = nchw(rs.clone()).requires_grad_(True) if res else None
    aa = ab.clone().requires_grad_(True)
    packed = []

    def pack(t):
        packed.append((t.data_ptr(), t.numel() * t.element_size()))
        return t

    def run(xx, aa, rr):
        out = training.timestep_modulate(xx, aa, rr, ln)
        return out if ln else (out, None)

    def back(xp, z):
        torch.autograd.backward([xp, z] if ln else [xp], [nchw(dxp), dz] if ln else [nchw(dxp)])

    before = dict(training.MOD_COUNTERS)
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        xp, z = run(xx, aa, rr)
    now = training.MOD_COUNTERS
    assert now["copied"] == before["copied"], "an NHWC-dense input was copied"
    assert (now["calls"], now["residual"], now["layernorm"]) == (before["calls"] + 1, before["residual"] + int(res), before["layernorm"] + int(ln))
    assert xp.shape == (B, C, H, W) and xp.permute(0, 2, 3, 1).is_contiguous() and xp.requires_grad
    assert not ln or (z.shape == (B, P, C) and z.is_contiguous() and z.requires_grad)
    ptrs = [p for p, _ in packed]
    assert xx.data_ptr() in ptrs and aa.data_ptr() in ptrs and (not res or rr.data_ptr() in ptrs)     # used in place: what is saved shares its memory with the inputs
    assert xp.data_ptr() not in ptrs, "x' was saved"
    inputs = (1 + int(res)) * B * P * C * 4 + B * 2 * C * 4
    assert sum(n for _, n in packed) <= inputs + (B * P * C * 4 if ln else 0) + 4 * B * P, packed
    back(xp, z)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(B, P, C)
    assert torch.equal(rows(xp.detach()), raw["xp"]) and (not ln or torch.equal(z.detach(), raw["z"]))
    assert xx.grad.shape == (B, C, H, W) and xx.grad.permute(0, 2, 3, 1).is_contiguous()      # the gradient stays in the layout the block upstream reads
    assert torch.equal(rows(xx.grad), raw["dx"]) and aa.grad.shape == (B, 2 * C) and torch.equal(aa.grad, raw["dab"])
    if res:
        assert torch.equal(rows(rr.grad), raw["dx"])
        # the same tensor serves x and residual: u = 2 x, and its gradient is the two equal halves added
        x2 = nchw(x.clone()).requires_grad_(True)
        back(*run(x2, ab, x2))
        twice = fused(x, x, ab, dxp, dz if ln else None, ln)
        assert torch.equal(rows(x2.grad), twice["dx"] + twice["dx"])
    # an NCHW-dense input is copied once and gives the same bits
    xc = nchw(x).contiguous()
    rc = nchw(rs).contiguous() if res else None
    assert xc.is_contiguous() and not xc.permute(0, 2, 3, 1).is_contiguous()
    copied = training.MOD_COUNTERS["copied"]
    assert torch.equal(rows(run(xc, ab, rc)[0]), raw["xp"])
    assert training.MOD_COUNTERS["copied"] == copied + 1 + int(res)
    # once differentiable: the gradient comes back without a graph of its own, so a second differentiation cannot silently use a wrong one
    x3 = nchw(x.clone()).requires_grad_(True)
    (gx,) = torch.autograd.grad(run(x3, ab, nchw(rs) if res else None)[0].sum(), x3, create_graph=True)
    assert not gx.requires_grad
    # a frozen ab: no gradient for it, the same dx bits ...
    x4 = nchw(x.clone()).requires_grad_(True)
    back(*run(x4, ab, nchw(rs) if res else None))
    assert ab.grad is None and torch.equal(rows(x4.grad), raw["dx"])
    # ... and a frozen trunk: dab alone, the same bits
    a5 = ab.clone().requires_grad_(True)
    back(*run(nchw(x), a5, nchw(rs) if res else None))
    assert torch.equal(a5.grad, raw["dab"])
    if ln:  # an output nobody used arrives as None: z alone gives the bits of the raw call without dx', x' alone those of the raw call without dz
        x6, a6 = nchw(x.clone()).requires_grad_(True), ab.clone().requires_grad_(True)
        training.timestep_modulate(x6, a6, nchw(rs) if res else None, True)[1].backward(dz)
        only_z = fused(x, rs, ab, None, dz)
        assert torch.equal(rows(x6.grad), only_z["dx"]) and torch.equal(a6.grad, only_z["dab"])
        x7, a7 = nchw(x.clone()).requires_grad_(True), ab.clone().requires_grad_(True)
        training.timestep_modulate(x7, a7, nchw(rs) if res else None, True)[0].backward(nchw(dxp))
        only_xp = fused(x, rs, ab, dxp, None)
        assert torch.equal(rows(x7.grad), only_xp["dx"]) and torch.equal(a7.grad, only_xp["dab"])
    with pytest.raises(ValueError, match="multiple of 4"):
        training.timestep_modulate(torch.zeros(1, 6, 2, 2, device=DEV), torch.zeros(1, 12, device=DEV))


def _t_blocks(m):
    """(T blocks, those right behind a C / F block, those right in front of an A / F block) of the network, level by level"""
    n = after = before = 0
    for level in list(m.down_blocks) + list(m.up_blocks):
        kinds = [b.kind for b in level]
        for j, k in enumerate(kinds):
            if k == 'T':
                n += 1
                after += int(j > 0 and kinds[j - 1] in ('C', 'F'))
                before += int(j + 1 < len(kinds) and kinds[j + 1] in ('A', 'F'))
    return n, after, before


@pytest.mark.parametrize("others", ["torch", "hip"])
@pytest.mark.parametrize("which", ["tiny", "variant"])
def test_train_step_with_hip_modulation_reproduces_the_reference(golden, built_lib, which, others):
    """_train_step of tests/test_gpu_training.py under set_training_modulation("hip"), the other three switches all "torch" and all "hip", against the reference's
    recorded step and under that test's tolerances; then the hand-over to the HIP engine, which never sees the switch.  `variant` is ['CFT', 'TAC']: T after F, T
    first in a level, T before A."""
    cfg, m = T.model_for(which, golden, DEV)
    m.set_training_modulation("hip").set_training_activation(others).set_training_depthwise(others).set_training_attention(others)
    calls = []
    real = training.timestep_modulate

    def counting(x, ab, residual=None, layernorm=False, eps=1e-6):
        calls.append((residual is not None, bool(layernorm)))
        return real(x, ab, residual, layernorm, eps)

    training.timestep_modulate = counting
    try:
        pred, loss = _train_step(m, cfg)
    finally:
        training.timestep_modulate = real
    n, after, before = _t_blocks(m)
    assert n > 0 and after > 0 and before > 0 and (which != "variant" or after < n)
    assert len(calls) == n, "the train-mode forward did not route every TimestepBlock through the HIP op"
    assert sum(r for r, _ in calls) == after, "a C / F block in front of a T block did not hand its summands over unadded"
    assert sum(ln for _, ln in calls) == before, "an A / F block behind a T block did not get its LayerNorm rows from the op"
    T.assert_switched_step_and_handover(m, cfg, golden("train_%s_step" % which), pred, loss, lambda: m.set_training_modulation("torch"),
                                        op_calls=lambda: training.MOD_COUNTERS["calls"], calls_per_forward=n)


@pytest.fixture(scope="module")
def dropout_cases(golden, built_lib):
    made = {}

    def get(name):
        if name not in made:
            made[name] = T.Case(name, T.STEP_CASES[name], golden)
        return made[name]

    yield get
    made.clear()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name", ["recorded-tiny", "odd-variant", "head-80"])
def test_step_with_dropout_and_all_four_switches(dropout_cases, name):
    """tests/test_gpu_train_step_dropout.py's step with injected seeds, all four switches on "hip", against the fp64 mirror under that file's rule.  The new op draws
    no seed: the library calls of the other ops are still the mirror's call plan, each backward call with its forward's (p, seed)."""
    case = dropout_cases(name)
    seeds = T.injected(case)
    calls = training.MOD_COUNTERS["calls"]
    case.m.set_training_modulation("hip")
    try:
        out = T.run_step(case, seeds=iter(seeds))
    finally:
        case.m.set_training_modulation("torch")
    assert training.MOD_COUNTERS["calls"] == calls + _t_blocks(case.m)[0]
    ref, e32, plan = case.mirror(seeds)
    T.assert_call_protocol(case, out["harness"], plan)
    T.assert_within_yardstick(case, "all four switches", out["values"], ref, e32)
