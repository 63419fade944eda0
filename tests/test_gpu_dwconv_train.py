"""GPU: the training ResBlock front (paella_amd/csrc/dwconv_train.hip) against the fp64 model of tests/dwconv_ln_model.py.

The yardstick of every accuracy check is MEASURED in the same test, as tests/test_gpu_grn_act.py does: the torch fp32 chain of `training._res_block` (torch.cat ->
F.conv2d(groups=C) -> F.layer_norm, backward with the same dy) runs on the same device and inputs, its max abs error against the fp64 model is taken for each of y,
dx, dskip, dw and dbias, and the fused op must stay within 4x max(that error, one fp32 ulp at the model's largest magnitude) -- the ulp floor is the rounding no
fp32 result can avoid.  The measured pairs are kept in profiles/train_dwconv_parity.txt."""
import functools
import itertools

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from paella_amd import _lib, training
from tests import dwconv_ln_model as M
from tests import train_op_checks as T
from tests.test_gpu_training import _train_step

pytestmark = pytest.mark.gpu
DEV = "cuda"
# every tap but the centre is padding; one-row and one-column images of two samples; small; non-square with C off every grain and more than one strip of positions;
# more than 256 float4 slots per row; the real level-2 width
SHAPES = [(1, 1, 1, 8), (2, 1, 5, 8), (2, 5, 1, 8), (2, 3, 2, 24), (3, 5, 13, 136), (1, 8, 8, 1032), (2, 4, 4, 1280)]
CASES = [s + (k,) for s in SHAPES for k in (False, True)] + [(1, 1, 1, 4, False), (2, 3, 2, 20, False)]
FACTOR = T.FACTOR
_err, _ulp = T.err, T.ulp
EPS = 1e-6
OUTS = ("y", "dx", "dskip", "dw", "dbias")
ids = lambda s: "x".join(map(str, s[:4])) + ("-skip" if s[4] else "")


@functools.lru_cache(maxsize=None)
def _inputs(B, H, W, C, skip):
    gen = torch.Generator().manual_seed(1000000 * B + 10000 * H + 100 * W + C + int(skip))
    J = 2 if skip else 1
    x = torch.randn(B, H, W, C, generator=gen).to(DEV)
    s = torch.randn(B, H, W, C, generator=gen).to(DEV) if skip else None
    w = (torch.randn(C, J, 3, 3, generator=gen) * 0.4).to(DEV)
    bias = (torch.randn(C, generator=gen) * 0.5).to(DEV)
    dy = torch.randn(B, H, W, C, generator=gen).to(DEV)
    return x, s, w, bias, dy


@functools.lru_cache(maxsize=None)
def _model(case):
    x, s, w, bias, dy = _inputs(*case)
    y, rstd = M.forward(x, s, w, bias, EPS)
    return (y,) + M.backward(x, s, w, bias, dy, EPS)


def fused(x, s, w, bias, dy=None, want=(True, True, True, True), poison=True):
    """the raw op on NHWC tensors: forward, and backward when dy is given -> dict of outputs.  Outputs and workspace start as NaN: they are WRITTEN, and the
    workspace needs no set-up."""
    lib = _lib.load()
    B, H, W, C = x.shape
    has = int(s is not None)
    new = (lambda *sh: torch.full(sh, float("nan"), device=DEV)) if poison else (lambda *sh: torch.empty(sh, device=DEV))
    ws = torch.empty(lib.paella_dwconv_ln_train_workspace_bytes(B, H, W, C, has), dtype=torch.uint8, device=DEV)
    if poison:
        ws.fill_(255)
    out = dict(y=new(B, H, W, C), rstd=new(B, H, W))
    nf = lib.paella_dwconv_ln_train_workspace_bytes(1, 1, 1, C, has)   # the forward asks for the repacked weights only
    _lib.check(lib.paella_dwconv_ln_train_forward(_lib.ptr(x), _lib.ptr(s), _lib.ptr(w), _lib.ptr(bias), B, H, W, C, EPS, _lib.ptr(out["y"]), _lib.ptr(out["rstd"]),
                                                  _lib.ptr(ws), nf, _lib.stream_ptr(x.device)))
    if dy is not None:
        if poison:
            ws.fill_(255)
        out["dx"] = new(B, H, W, C) if want[0] else None
        out["dskip"] = new(B, H, W, C) if want[1] and has else None
        out["dw"] = new(*w.shape) if want[2] else None
        out["dbias"] = new(C) if want[3] else None
        _lib.check(lib.paella_dwconv_ln_train_backward(_lib.ptr(x), _lib.ptr(s), _lib.ptr(w), _lib.ptr(out["y"]), _lib.ptr(out["rstd"]), _lib.ptr(dy), B, H, W, C,
                                                       _lib.ptr(out["dx"]), _lib.ptr(out["dskip"]), _lib.ptr(out["dw"]), _lib.ptr(out["dbias"]), _lib.ptr(ws), ws.numel(),
                                                       _lib.stream_ptr(x.device)))
    return out


def torch_chain(x, s, w, bias, dy):
    """the front of training._res_block as torch runs it in fp32 (NHWC tensors in and out) -> (y, dx, dskip, dw, dbias)"""
    leaves = [t.clone().requires_grad_(True) if t is not None else None for t in (x, s, w, bias)]
    xx, ss, ww, bb = leaves
    xc = xx.permute(0, 3, 1, 2)
    if ss is not None:
        xc = torch.cat([xc, ss.permute(0, 3, 1, 2)], dim=1)
    C = w.size(0)
    y = F.layer_norm(F.conv2d(xc, ww, bb, padding=1, groups=C).permute(0, 2, 3, 1), (C,), None, None, EPS)
    y.backward(dy)
    return (y.detach(),) + tuple(None if t is None else t.grad for t in leaves)


def _check_accuracy(tag, out, ref, model):
    pairs = []
    for name, b, m in zip(OUTS, ref, model):
        if m is None:
            continue
        assert torch.isfinite(out[name]).all(), "%s: not finite" % name
        pairs.append((name, _err(out[name], m), _err(b, m), _ulp(m)))
    print("train_dwconv parity %s: " % tag + "  ".join("%s fused %.3e torch %.3e ulp %.3e" % q for q in pairs))
    for name, e_fused, e_torch, ulp in pairs:
        assert T.within_yardstick(e_fused, e_torch, ulp), "%s %s: fused error %.3e exceeds %gx max(torch fp32 chain %.3e, ulp %.3e)" % (tag, name, e_fused, FACTOR, e_torch, ulp)


@pytest.mark.parametrize("case", CASES, ids=ids)
def test_accuracy_against_the_fp64_model(built_lib, case):
    """Measured pairs (fused / torch, MI355X): all of them in profiles/train_dwconv_parity.txt."""
    x, s, w, bias, dy = _inputs(*case)
    out = fused(x, s, w, bias, dy)
    _check_accuracy(ids(case), out, torch_chain(x, s, w, bias, dy), _model(case))
    # rstd itself, loosely (y and the gradients above hold it to account): the variance of O(1) values whose fp32 sums of up to 18 products carry ~1e-6 each
    _, rstd64 = M.forward(x, s, w, bias, EPS)
    torch.testing.assert_close(out["rstd"].double(), rstd64, rtol=1e-4, atol=0)


@pytest.mark.parametrize("skip", [False, True], ids=["plain", "skip"])
def test_sample_independence(built_lib, skip):
    """For a batch of 3, y, dx and dskip of each sample are the bits of a one-sample call on its slice -- a tap that crossed a sample border would show"""
    x, s, w, bias, dy = _inputs(3, 5, 13, 136, skip)
    full = fused(x, s, w, bias, dy)
    for b in range(3):
        one = fused(x[b:b + 1], None if s is None else s[b:b + 1], w, bias, dy[b:b + 1])
        for k in ("y", "rstd", "dx") + (("dskip",) if skip else ()):
            assert torch.equal(full[k][b:b + 1], one[k]), (b, k)


@pytest.mark.parametrize("case", [(3, 5, 13, 136, False), (3, 5, 13, 136, True), (1, 8, 8, 1032, True), (2, 4, 4, 1280, False)], ids=ids)
def test_null_outputs_and_determinism(built_lib, case):
    """(3, 5, 13): more than one strip of positions, dw / dbias through the partials; the others: one strip, written by the summing kernel itself"""
    x, s, w, bias, dy = _inputs(*case)
    names = ("dx", "dskip", "dw", "dbias")
    full = fused(x, s, w, bias, dy)
    again = fused(x, s, w, bias, dy, poison=False)
    for k in ("y", "rstd") + names:
        if full[k] is None:
            assert k == "dskip" and s is None
            continue
        assert torch.isfinite(full[k]).all(), k   # the NaN the outputs and the workspace were filled with is gone
        assert torch.equal(full[k], again[k]), k
    for want in itertools.product((False, True), repeat=4):
        if all(want) or (s is None and want[1]):
            continue
        part = fused(x, s, w, bias, dy, want)
        assert torch.equal(part["y"], full["y"])
        for k, on in zip(names, want):
            if on and full[k] is not None:
                assert torch.equal(part[k], full[k]), (want, k)
            else:
                assert part[k] is None


@pytest.mark.parametrize("skip", [False, True], ids=["plain", "skip"])
def test_constant_row(built_lib, skip):
    """x = 0 and one bias for every channel: variance 0, y = 0 exactly, rstd = 1 / sqrt(eps), and finite gradients equal to the model's under the accuracy rule"""
    case = (2, 3, 2, 24, skip)
    x, s, w, _, dy = _inputs(*case)
    x = torch.zeros_like(x)
    s = None if s is None else torch.zeros_like(s)
    bias = torch.full((24,), 0.5, device=DEV)
    out = fused(x, s, w, bias, dy)
    assert torch.all(out["y"] == 0)
    torch.testing.assert_close(out["rstd"], torch.full_like(out["rstd"], 1000.0), rtol=1e-6, atol=0)
    y64, _ = M.forward(x, s, w, bias, EPS)
    assert torch.all(y64 == 0)
    _check_accuracy("constant row " + ids(case), out, torch_chain(x, s, w, bias, dy), (y64,) + M.backward(x, s, w, bias, dy, EPS))


def test_offsets_past_4_gib(built_lib):
    """B = 1025 samples of 32 x 32 x 1024 fp32: the last sample starts at byte 2^32.  The arithmetic of a sample depends neither on b nor on B: its y and dx are
    the bits of a one-sample call on its slice."""
    B, H, W, C = 1025, 32, 32, 1024
    assert (B - 1) * H * W * C * 4 >= 2 ** 32
    _, _, w, bias, _ = _inputs(1, 1, 1, C, False)
    gen = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(B, H, W, C, device=DEV, generator=gen)
    dy = torch.randn(B, H, W, C, device=DEV, generator=gen)
    big = one = None
    try:
        big = fused(x, None, w, bias, dy, poison=False)
        one = fused(x[B - 1:], None, w, bias, dy[B - 1:])
        assert torch.isfinite(one["y"]).all() and torch.isfinite(one["dx"]).all()
        assert torch.equal(big["y"][B - 1:], one["y"]) and torch.equal(big["dx"][B - 1:], one["dx"]) and torch.equal(big["rstd"][B - 1:], one["rstd"])
        # and the one-sample call is right (fp32 chain, loose: the accuracy tests hold the op to the fp64 model)
        ry, rdx, _, _, _ = torch_chain(x[B - 1:], None, w, bias, dy[B - 1:])
        torch.testing.assert_close(one["y"], ry, rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(one["dx"], rdx, rtol=1e-4, atol=1e-4)
        # sample 0 and the samples around byte 2^31 are finite and differ from the last one; the parameter gradients of 2^20 positions are finite
        assert torch.isfinite(big["y"][0]).all() and torch.isfinite(big["dx"][511:513]).all() and not torch.equal(big["y"][0], one["y"][0])
        assert torch.isfinite(big["dw"]).all() and torch.isfinite(big["dbias"]).all()
    finally:
        del big, one, x, dy
        torch.cuda.empty_cache()


@pytest.mark.parametrize("skip", [False, True], ids=["plain", "skip"])
def test_autograd_function_and_saved_state(built_lib, skip):
    case = (3, 5, 13, 136, skip)
    B, H, W, C = case[:4]
    x, s, w, bias, dy = _inputs(*case)
    raw = fused(x, s, w, bias, dy)
    nchw = lambda t: t.permute(0, 3, 1, 2)                   # logical [B, C, H, W] over NHWC memory
    xx = nchw(x.clone()).requires_grad_(True)
    ss = nchw(s.clone()).requires_grad_(True) if skip else None
    ww = nn.Parameter(w.clone())                              # the module's parameter shapes, as they are
    bb = nn.Parameter(bias.clone())
    packed = []

    def pack(t):
        packed.append((t.data_ptr(), t.numel() * t.element_size()))
        return t

    copied = training.DW_COUNTERS["copied"]
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        y = training.dwconv_layernorm(xx, ww, bb, ss)
    assert training.DW_COUNTERS["copied"] == copied, "an NHWC-dense input was copied"
    assert y.shape == (B, H, W, C) and y.is_contiguous() and y.requires_grad
    ptrs = [p for p, _ in packed]
    assert xx.data_ptr() in ptrs and (not skip or ss.data_ptr() in ptrs)     # used in place: the saved x shares its memory with the input
    inputs_and_y = (1 + int(skip) + 1) * B * H * W * C * 4 + ww.numel() * 4 + C * 4
    assert sum(n for _, n in packed) <= inputs_and_y + 8 * B * H * W, packed
    y.backward(dy)
    assert torch.equal(y.detach(), raw["y"])
    assert xx.grad.shape == (B, C, H, W) and xx.grad.permute(0, 2, 3, 1).is_contiguous()      # the gradient stays in the layout the block upstream reads
    assert torch.equal(xx.grad.permute(0, 2, 3, 1), raw["dx"]) and torch.equal(ww.grad, raw["dw"]) and torch.equal(bb.grad, raw["dbias"])
    assert ww.grad.shape == ww.shape and bb.grad.shape == bb.shape
    if skip:
        assert torch.equal(ss.grad.permute(0, 2, 3, 1), raw["dskip"])
    # an NCHW-dense input is copied once and gives the bits of its NHWC-dense copy
    xc = nchw(x).contiguous()
    sc = nchw(s).contiguous() if skip else None
    assert xc.is_contiguous() and not xc.permute(0, 2, 3, 1).is_contiguous()
    copied = training.DW_COUNTERS["copied"]
    assert torch.equal(training.dwconv_layernorm(xc, w, bias, sc), raw["y"])
    assert training.DW_COUNTERS["copied"] == copied + 1 + int(skip)
    # once differentiable: the gradient comes back without a graph of its own, so a second differentiation cannot silently use a wrong one
    x2 = nchw(x.clone()).requires_grad_(True)
    (gx,) = torch.autograd.grad(training.dwconv_layernorm(x2, w, bias, nchw(s) if skip else None).sum(), x2, create_graph=True)
    assert not gx.requires_grad
    # frozen parameters: no gradient for them, the same dx bits
    x3 = nchw(x.clone()).requires_grad_(True)
    training.dwconv_layernorm(x3, w, bias, nchw(s) if skip else None).backward(dy)
    assert w.grad is None and bias.grad is None and torch.equal(x3.grad.permute(0, 2, 3, 1), raw["dx"])
    # and a frozen trunk: the parameter gradients alone, the same bits
    w4, b4 = nn.Parameter(w.clone()), nn.Parameter(bias.clone())
    training.dwconv_layernorm(nchw(x), w4, b4, nchw(s) if skip else None).backward(dy)
    assert torch.equal(w4.grad, raw["dw"]) and torch.equal(b4.grad, raw["dbias"])
    with pytest.raises(ValueError, match="multiple of 4"):
        training.dwconv_layernorm(torch.zeros(1, 6, 2, 2, device=DEV), torch.zeros(6, 1, 3, 3, device=DEV), torch.zeros(6, device=DEV))


@pytest.mark.parametrize("act", ["torch", "hip"])
@pytest.mark.parametrize("which", ["tiny", "variant"])
def test_train_step_with_hip_depthwise_reproduces_the_reference(golden, built_lib, which, act):
    """_train_step of tests/test_gpu_training.py under set_training_depthwise("hip"), alone and together with set_training_activation("hip"), against the
    reference's recorded step and under that test's tolerances; then the hand-over to the HIP engine, which never sees the switch"""
    cfg, m = T.model_for(which, golden, DEV)
    m.set_training_depthwise("hip").set_training_activation(act)
    calls = []
    real = training.dwconv_layernorm

    def counting(x, weight, bias, skip=None, eps=1e-6):
        calls.append(skip is not None)
        return real(x, weight, bias, skip, eps)

    training.dwconv_layernorm = counting
    try:
        pred, loss = _train_step(m, cfg)
    finally:
        training.dwconv_layernorm = real
    c_blocks = [b for lv in list(m.down_blocks) + list(m.up_blocks) for b in lv if b.kind == "C"]
    assert len(calls) == len(c_blocks), "the train-mode forward did not route every ResBlock through the HIP op"
    assert sum(calls) == sum(1 for b in c_blocks if b.depthwise.weight.size(1) == 2), "the up-path blocks did not hand their skip to the op"
    T.assert_switched_step_and_handover(m, cfg, golden("train_%s_step" % which), pred, loss, lambda: m.set_training_depthwise("torch"),
                                        op_calls=lambda: training.DW_COUNTERS["calls"], calls_per_forward=len(c_blocks))
