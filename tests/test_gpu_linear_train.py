"""GPU: the training linear on bf16 operands (paella_amd/csrc/linear_train.hip; Paella.set_training_gemm("bf16")).

Pack.  `pack_bf16` against CPU torch's `.bfloat16()` of the tensor and of its transpose, bit for bit as int16 (NaN by isnan), on inputs that carry exact ties in
both directions, signed zeros, subnormals, the largest finite float (rounds to inf), infinities and NaN; the column sums under the yardstick rule of
tests/train_op_checks.py on finite inputs.

Op.  The reference is the fp64 product of the bf16-ROUNDED operands (`t.bfloat16().double()`; in the backward dy is rounded too), so what is measured is the GEMM and
not the rounding the mode is made of.  The bound is derived, not measured: a bf16 x bf16 product has 16 significant bits and is exact in fp32; summing R of them in any
order -- the slabs of a split reduction included -- errs by at most (R - 1) 2^-24 sum|a||b| to first order, and the bias add is one more rounding.  Asserted
elementwise: |got - ref| <= 1.01 (R + 2) 2^-24 (|A16| |B16|^T + |bias|), R the reduction length.  db is checked against the fp64 column sums of the UNROUNDED dy under
the yardstick rule.

Network.  A two-level network defined here, dropout 0, synthetic weights.  The reference is the SAME module as a .double() copy on the device, train mode, with the
module global `training.linear_bf16` replaced by a torch-op emulation that rounds the operands and the arriving gradient to bf16 exactly where the op does (and, for
the check with the other four switches on "hip", `training.attention_dropout` replaced by the plain softmax formula, which is what routes the three projections of an
AttnBlock through the linear; the other three ops compute what their torch chains compute and stay on them in the reference).  e_emu is that emulation in fp32 on the
device against the fp64 one, e_hip the HIP route against the fp64 one, per tensor (every parameter gradient, and the logits) as the relative L2 error: one rounding
flip at a bf16 tie moves an element by 2^-9 of its value on either side and would dominate a max-abs figure without saying anything about the op.  The rule is the
project's: e_hip <= FACTOR max(e_emu, 2^-24), FACTOR = 4 from tests/train_op_checks.py, under both settings of the other four switches; the ratios are kept in
profiles/train_linear_parity.txt.  The second case, 1 x 8x8 tokens, leaves the lower level at 16 rows: its sites must run F.linear, counted.

The rule is asserted in two forms (test_network_against_the_fp64_emulation, test_network_against_the_fp64_evaluation_with_the_routes_own_rounding):
  * against the fp64 evaluation that rounds ITS OWN operands, at 2 x 16x16 tokens.  An fp64 operand and the fp32 operand of a route differ by fp32 rounding, so an
    element that sits that close to a bf16 tie takes another bf16 value in the reference than on the route (a "flip", 2^-8 of the element).  Both e_hip and e_emu are
    then mostly flips; with tens of thousands of rounded elements both routes collect hundreds and the ratio is near 1.  At 1 x 8x8 only the linears of the upper
    level (64 rows) are routed and a route collects a few dozen (24 - 35 of 147456 rounded elements), a few of them in the forward: the second form COUNTS them per route (printed), and the statistic is whatever those few make of it
    (recorded: ratios 70.7 and 13.2) -- the figures of this form are printed at that case and not asserted.
  * against the fp64 evaluation that takes every rounding DECISION from the route it is compared with, at BOTH cases: the i-th routed linear of the fp64 evaluation
    uses x + (bf16(x32) - x32), the same for the weight and for the arriving gradient, x32 the route's own fp32 operand of its i-th call.  That is the fp64
    evaluation "in which every routed linear rounds as the op does", without the flips: what is left in e_hip and e_emu is fp32 arithmetic, and a routed site that
    computed something else -- a transposition, a dropped K block, a stale ticket -- fails it at either size.  Same statistic, same FACTOR, same floor."""
import functools

import pytest
import torch
from torch import nn

import paella_amd
from paella_amd import train_ops, training
from tests import train_op_checks as T
from tests import train_step_model as S
from tests.helpers import to_dev, weights_for

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
# (M, N, K): the smallest; all three differ (a mixed-up transposition cannot pass); one output tile with a long wgrad reduction (split-K, the ticket header); several
# column tiles
SHAPES = [(64, 64, 64), (128, 192, 320), (8192, 64, 64), (256, 1280, 320)]
PACK_SHAPES = [(64, 64), (64, 192), (4160, 128)]       # the last: 65 row tiles, more than one strip


# ---------------------------------------------------------------------------------------------------------------------
# pack
# ---------------------------------------------------------------------------------------------------------------------
def _special_values():
    tie_down, tie_up = 1.0 + 2.0 ** -8, 1.0 + 3.0 * 2.0 ** -8         # exactly between two bf16 values: to even is DOWN for the first, UP for the second
    fmax = torch.finfo(torch.float32).max
    v = [tie_down, tie_up, -tie_down, -tie_up, 0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 2.0 ** -133, 3.0 * 2.0 ** -134, 2.0 ** -126, fmax, -fmax,
         float("inf"), float("-inf"), float("nan"), 1.0, -1.0, 2.0 ** -8, 1.0 + 2.0 ** -7, 1.0 + 2.0 ** -9, 1.0 + 2.0 ** -8 + 2.0 ** -20]
    return torch.tensor(v, dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def _pack_input(rows, cols, special=True):
    g = torch.Generator().manual_seed(100 * rows + cols)
    x = torch.randn(rows, cols, generator=g)
    if special:
        sv = _special_values()
        pos = torch.randperm(rows * cols, generator=g)[:8 * sv.numel()]      # each value at eight places: every row quad and column offset sees some
        x.view(-1)[pos] = sv.repeat(8)
        x[0, :sv.numel()] = sv                                               # and at known places of the first tile
        x[rows - 1, cols - sv.numel():] = sv                                 # and of the last
    return x


def _same_bf16_bits(got, want, what):
    got, want = got.cpu(), want
    assert got.dtype == want.dtype == torch.bfloat16 and got.shape == want.shape, what
    nan = want.isnan()
    assert torch.equal(got.isnan(), nan), what + ": NaN in other places"
    g, w = got.view(torch.int16)[~nan], want.view(torch.int16)[~nan]
    bad = (g != w).nonzero()
    assert bad.numel() == 0, "%s: %d elements differ, first at flat index %d (got 0x%04x, torch 0x%04x)" % (
        what, bad.numel(), int(bad[0]), int(g[bad[0]]) & 0xffff, int(w[bad[0]]) & 0xffff)


@pytest.mark.parametrize("shape", PACK_SHAPES, ids=lambda s: "%dx%d" % s)
def test_pack_bits(shape):
    x = _pack_input(*shape)
    sv = _special_values().bfloat16()
    assert sv[13].isinf() and sv[14].isinf() and sv[0] == 1.0 and float(sv[1]) == 1.0 + 2.0 ** -6     # the ties and the overflow do what the docstring says
    row_ref, tr_ref = x.bfloat16(), x.t().contiguous().bfloat16()
    xd = x.to(DEV)
    row, tr = training.pack_bf16(xd, transposed=True)
    _same_bf16_bits(row, row_ref, "row-major")
    _same_bf16_bits(tr, tr_ref, "transposed")
    (row_only,) = training.pack_bf16(xd)
    _same_bf16_bits(row_only, row_ref, "row-major alone")
    # with the column sums in the same pass the bf16 outputs are the same bits (NaN / inf columns sum to NaN / inf: not compared here)
    row3, tr3, _ = training.pack_bf16(xd, transposed=True, colsum=True)
    _same_bf16_bits(row3, row_ref, "row-major beside the sums")
    _same_bf16_bits(tr3, tr_ref, "transposed beside the sums")


@pytest.mark.parametrize("shape", PACK_SHAPES, ids=lambda s: "%dx%d" % s)
def test_pack_column_sums(shape):
    x = _pack_input(*shape, special=False)
    xd = x.to(DEV)
    ref = x.double().sum(0)
    outs = [training.pack_bf16(xd, colsum=True)[-1], training.pack_bf16(xd, transposed=True, colsum=True)[-1]]
    e_torch = T.err(xd.sum(0).cpu(), ref)
    for cs in outs:
        e = T.err(cs.cpu(), ref)
        print("train_linear parity pack %dx%d colsum: e %.3e, torch fp32 sum(0) %.3e, ulp %.3e" % (shape + (e, e_torch, T.ulp(ref))))
        assert T.within_yardstick(e, e_torch, T.ulp(ref))
    assert torch.equal(outs[0], outs[1])
    assert torch.equal(outs[0], training.pack_bf16(xd, colsum=True)[-1])       # the strips fix the order: the same bits again


# ---------------------------------------------------------------------------------------------------------------------
# op
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _op_inputs(M, N, K):
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K)
    return (torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * K ** -0.5, torch.randn(N, generator=g), torch.randn(M, N, generator=g))


@functools.lru_cache(maxsize=None)
def _op_reference(M, N, K):
    """fp64 products of the rounded operands, and the |A| |B|^T sums the bound is made of; computed once per shape"""
    x, w, b, dy = _op_inputs(M, N, K)
    x16, w16, dy16 = x.bfloat16().double(), w.bfloat16().double(), dy.bfloat16().double()
    return dict(y=x16 @ w16.t(), y_abs=x16.abs() @ w16.abs().t(), dx=dy16 @ w16, dx_abs=dy16.abs() @ w16.abs(), dw=dy16.t() @ x16, dw_abs=dy16.abs().t() @ x16.abs(),
                db=dy.double().sum(0))


def _run_op(M, N, K, bias=True, need=(True, True, True), x=None, dy=None):
    """forward + backward through the public function -> dict(y, dx, dw, db) on the device (None where autograd did not want it)"""
    x0, w0, b0, dy0 = (t.to(DEV) for t in _op_inputs(M, N, K))
    x = (x0 if x is None else x).requires_grad_(need[0])
    w = w0.requires_grad_(need[1])
    b = b0.requires_grad_(need[2]) if bias else None
    y = training.linear_bf16(x, w, b)
    if any(need[:2]) or (bias and need[2]):
        y.backward(dy0 if dy is None else dy)
    return dict(y=y.detach(), dx=x.grad, dw=w.grad, db=None if b is None else b.grad)


def _assert_bound(name, got, ref, absprod, R, extra=None):
    bound = 1.01 * (R + 2) * U * (absprod if extra is None else absprod + extra)
    d = (got.double().cpu() - ref).abs()
    ratio = float((d / bound).max())
    print("train_linear parity op %s: largest |got - ref| / bound = %.4f (R = %d)" % (name, ratio, R))
    assert torch.isfinite(got).all() and bool((d <= bound).all()), "%s: |got - ref| exceeds the bound by up to %.3f x" % (name, ratio)


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_op_against_the_rounded_operand_reference(shape, bias):
    M, N, K = shape
    ref = _op_reference(M, N, K)
    b = _op_inputs(M, N, K)[2].double()
    before = dict(training.LINEAR_COUNTERS)
    out = _run_op(M, N, K, bias)
    assert training.LINEAR_COUNTERS == dict(before, calls=before["calls"] + 1, backward=before["backward"] + 1)
    tag = "%dx%dx%d%s" % (M, N, K, "" if bias else " no bias")
    _assert_bound(tag + " y", out["y"], ref["y"] + b if bias else ref["y"], ref["y_abs"], K, b.abs() if bias else None)
    _assert_bound(tag + " dx", out["dx"], ref["dx"], ref["dx_abs"], N)
    _assert_bound(tag + " dw", out["dw"], ref["dw"], ref["dw_abs"], M)
    if bias:
        dy = _op_inputs(M, N, K)[3].to(DEV)
        e, e_torch = T.err(out["db"].cpu(), ref["db"]), T.err(dy.sum(0).cpu(), ref["db"])
        print("train_linear parity op %s db: e %.3e, torch fp32 sum(0) %.3e, ulp %.3e" % (tag, e, e_torch, T.ulp(ref["db"])))
        assert T.within_yardstick(e, e_torch, T.ulp(ref["db"]))
    else:
        assert out["db"] is None
    # two identical calls: identical bits
    again = _run_op(M, N, K, bias)
    for k in ("y", "dx", "dw") + (("db",) if bias else ()):
        assert torch.equal(out[k], again[k]), k


@pytest.mark.parametrize("need", [(True, False, False), (False, True, False), (False, False, True), (False, False, False)], ids=["x", "weight", "bias", "none"])
def test_needs_input_grad_subsets(need):
    M, N, K = 128, 192, 320
    full = _run_op(M, N, K)
    before = dict(training.LINEAR_COUNTERS)
    out = _run_op(M, N, K, need=need)
    # the forward was called; a backward call was made exactly when some gradient is wanted
    assert training.LINEAR_COUNTERS == dict(before, calls=before["calls"] + 1, backward=before["backward"] + int(any(need)))
    assert torch.equal(out["y"], full["y"])
    for k, wanted in zip(("dx", "dw", "db"), need):
        if wanted:
            assert torch.equal(out[k], full[k]), k      # a gradient does not depend on which others are computed
        else:
            assert out[k] is None, k


def test_non_contiguous_x_and_dy_give_the_same_bits():
    M, N, K = 128, 192, 320
    dense = _run_op(M, N, K)
    x0, _, _, dy0 = (t.to(DEV) for t in _op_inputs(M, N, K))
    xb, dyb = torch.zeros(M, 2 * K, device=DEV), torch.zeros(M, 2 * N, device=DEV)
    xb[:, ::2], dyb[:, ::2] = x0, dy0
    x_nc, dy_nc = xb[:, ::2].detach(), dyb[:, ::2]
    assert not x_nc.is_contiguous() and not dy_nc.is_contiguous()
    before = dict(training.LINEAR_COUNTERS)
    out = _run_op(M, N, K, x=x_nc, dy=dy_nc)
    assert training.LINEAR_COUNTERS == dict(before, calls=before["calls"] + 1, backward=before["backward"] + 1, copied=before["copied"] + 2)
    for k in ("y", "dx", "dw", "db"):
        assert torch.equal(out[k], dense[k]), k
    # [..., K]: leading dimensions are flattened to rows and come back
    y3 = training.linear_bf16(x0.view(2, M // 2, K), _op_inputs(M, N, K)[1].to(DEV), _op_inputs(M, N, K)[2].to(DEV))
    assert y3.shape == (2, M // 2, N) and torch.equal(y3.view(M, N), dense["y"])


def test_refusals_launch_nothing(monkeypatch):
    launched = []
    monkeypatch.setattr(train_ops, "_call", lambda *a: launched.append(a))
    before = dict(training.LINEAR_COUNTERS)
    z = lambda *s: torch.zeros(*s, device=DEV)
    with pytest.raises(ValueError, match="M = 96"):
        training.linear_bf16(z(96, 128), z(192, 128), z(192))
    with pytest.raises(ValueError, match="K = 32"):
        training.linear_bf16(z(128, 32), z(192, 32), z(192))
    with pytest.raises(ValueError, match="fp32 x, weight and bias"):
        training.linear_bf16(z(128, 128).half(), z(192, 128), z(192))
    with pytest.raises(ValueError, match="fp32 x, weight and bias"):
        training.linear_bf16(z(128, 128), z(192, 128).half(), z(192))
    with pytest.raises(ValueError, match="x, weight and bias must live on the same cuda device"):
        training.linear_bf16(torch.zeros(128, 128), z(192, 128), z(192))
    with pytest.raises(ValueError, match="x, weight and bias must live on the same cuda device"):
        training.linear_bf16(z(128, 128), z(192, 128), torch.zeros(192))
    assert not launched and training.LINEAR_COUNTERS == before


# ---------------------------------------------------------------------------------------------------------------------
# network
# ---------------------------------------------------------------------------------------------------------------------
# every MLP and every projection of the AttnBlock qualifies at 2 x 16x16 tokens: M = 512 at level 0, 128 at level 1, and 2 x 32 conditioning rows for the kv projection
NET = dict(c_in=32, c_out=32, num_labels=64, c_r=16, patch_size=1, c_cond=64, c_hidden=[64, 128], nhead=[-1, 2], blocks=[1, 1], level_config=['CT', 'CTA'],
           clip_embd=48, byt5_embd=40, clip_seq_len=4, kernel_size=3, dropout=0.0, self_attn=False)
NET_CASES = {"2x16x16": (2, 16, 16), "1x8x8": (1, 8, 8)}       # the second leaves the lower level at M = 16 and the kv projection at 32 rows: they fall back
OTHERS = {"torch": ("torch",) * 4, "hip": ("hip",) * 4}


def _rnd(t):
    return t.float().bfloat16().to(t.dtype)


class _EmuLinear(torch.autograd.Function):
    """what `linear_bf16` computes, as torch ops in the dtype of its inputs: operands and the arriving gradient rounded to bf16, db from the unrounded gradient"""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        y = _rnd(x) @ _rnd(w).t()
        return y if b is None else y + b

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        g = _rnd(dy)
        return g @ _rnd(w), g.t() @ _rnd(x), dy.sum(0)


def _emu_linear(x, weight, bias=None):
    return _EmuLinear.apply(x.reshape(-1, x.size(-1)), weight, bias).view(x.shape[:-1] + (weight.size(0),))


def _emu_attention(q, kv, nhead, p=0.0, seed=None):
    """`attention_dropout` at p = 0 as torch ops in the dtype of its inputs"""
    assert p == 0.0
    B, P, C = q.shape
    heads = lambda t: t.reshape(B, -1, nhead, C // nhead).transpose(1, 2)
    w = torch.softmax(heads(q) @ heads(kv[..., :C]).transpose(-1, -2) / (C // nhead) ** 0.5, dim=-1)
    return (w @ heads(kv[..., C:])).transpose(1, 2).reshape(B, P, C)


class _Record:
    """a linear (the op or its fp32 emulation) that keeps, per call, the bf16 value and the rounding error bf16(t) - t of x, the weight and the arriving gradient"""

    def __init__(self, fn):
        self.fn, self.x, self.w, self.g = fn, [], [], []

    @staticmethod
    def _of(t):
        t = t.detach()
        r = t.bfloat16().double()
        return r, r - t.double()

    def __call__(self, x, weight, bias=None):
        i = len(self.x)
        self.x.append(self._of(x))
        self.w.append(self._of(weight))
        self.g.append(None)
        y = self.fn(x, weight, bias)
        y.register_hook(lambda g, i=i: self.g.__setitem__(i, self._of(g)))
        return y


class _ReplayLinear(torch.autograd.Function):
    """the routed linear in fp64 with the rounding decisions of a recorded route: operand + (the route's rounding error of that operand)"""

    @staticmethod
    def forward(ctx, x, w, b, replay, i):
        rec = replay.rec
        (rx, ex), (rw, ew) = rec.x[i], rec.w[i]
        replay.count(x, rx)
        replay.count(w, rw)
        xr, wr = x + ex.reshape(x.shape), w + ew
        ctx.save_for_backward(xr, wr)
        ctx.replay, ctx.i = replay, i
        y = xr @ wr.t()
        return y if b is None else y + b

    @staticmethod
    def backward(ctx, dy):
        xr, wr = ctx.saved_tensors
        rg, eg = ctx.replay.rec.g[ctx.i]
        ctx.replay.count(dy, rg.reshape(dy.shape))
        g = dy + eg.reshape(dy.shape)
        return g @ wr, g.t() @ xr, dy.sum(0), None, None


class _Replay:
    """`linear_bf16` for the fp64 module: call i replays call i of the record; counts the elements whose own bf16 value (of the fp64 operand, through fp32) is not
    the route's -- the flips the other form of the rule is exposed to"""

    def __init__(self, rec):
        self.rec, self.i, self.flips, self.rounded = rec, 0, 0, 0

    def count(self, t64, r):
        self.flips += int((t64.detach().float().bfloat16().double() != r.reshape(t64.shape)).sum())
        self.rounded += t64.numel()

    def __call__(self, x, weight, bias=None):
        i, self.i = self.i, self.i + 1
        return _ReplayLinear.apply(x.reshape(-1, x.size(-1)), weight, bias, self, i).view(x.shape[:-1] + (weight.size(0),))


def _step(m, inp, dtype=torch.float32, fused_loss=False):
    """one training step of m on inp -> {parameter name: gradient, T.LOGITS: logits}; with fused_loss through `forward_loss` (no logits)"""
    latents, t, mask, random_x, c = inp
    latents, t, mask = latents.to(DEV), t.to(DEV), mask.to(DEV)
    noised = latents * (1 - mask) + random_x.to(DEV) * mask
    c = {k: (v.to(dtype) if torch.is_tensor(v) else [u.to(dtype) for u in v] if v is not None else None) for k, v in to_dev(c, DEV).items()}
    m.train()
    m.dropout = 0.0
    m.zero_grad(set_to_none=True)
    lw = m.get_loss_weight(t, mask).to(dtype)
    pred = None
    if fused_loss:
        per_pos, _ = m.forward_loss(noised, t, latents, **c)
    else:
        pred = m(noised, t, **c)
        per_pos = nn.CrossEntropyLoss(label_smoothing=0.1, reduction='none')(pred, latents)
    ((per_pos * lw).sum(dim=[1, 2]) / lw.sum(dim=[1, 2])).mean().backward()
    out = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
    if pred is not None:
        out[T.LOGITS] = pred.detach()
    return out


def _switch(m, others, gemm):
    return m.set_training_activation(others[0]).set_training_depthwise(others[1]).set_training_attention(others[2]).set_training_modulation(others[3]).set_training_gemm(gemm)


@functools.lru_cache(maxsize=None)
def _net():
    m = paella_amd.Paella(**NET)
    sd = weights_for(m, sum(NET["blocks"]))
    m64 = paella_amd.Paella(**NET)
    m64.load_state_dict(sd)
    return m.to(DEV), m64.double().to(DEV)


@functools.lru_cache(maxsize=None)
def _net_inputs(case):
    B, H, W = NET_CASES[case]
    return S.inputs(NET, B, H, W, S_byt5=24, n_img=1)      # 24 ByT5 rows + 4 CLIP text + 4 CLIP image = 32 conditioning rows per sample


def _expected_counts(m, case, others):
    """(calls, fallbacks) of one forward: two linears per C / F block, three per A block on the route.attn branch, each at its level's row count"""
    B, H, W = NET_CASES[case]
    calls = fallbacks = 0

    def site(M, N, K):
        nonlocal calls, fallbacks
        if training.linear_shapes_ok(M, N, K):
            calls += 1
        else:
            fallbacks += 1

    levels = list(enumerate(m.down_blocks)) + [(len(NET["c_hidden"]) - 1 - u, lv) for u, lv in enumerate(m.up_blocks)]
    for i, level in levels:
        C, M = NET["c_hidden"][i], B * (H >> i) * (W >> i) // NET["patch_size"] ** 2
        for blk in level:
            if blk.kind in ("C", "F"):
                site(M, 4 * C, C)
                site(M, C, 4 * C)
            elif blk.kind == "A" and others[2] == "hip":
                site(M, C, C)
                site(B * 32, 2 * C, C)
                site(M, C, C)
    return calls, fallbacks


def _rel_l2(got, ref):
    return float((got.double() - ref).norm() / ref.norm().clamp_min(1e-300))


@functools.lru_cache(maxsize=None)
def _reference(case, others_name):
    """(the fp64 emulation's step, e_emu per tensor): both with the emulations in place of the module globals"""
    m, m64 = _net()
    others = OTHERS[others_name]
    route = ("torch", "torch", others[2], "torch")      # the fp64 module runs torch ops; the attention branch decides which projections are routed
    real = training.linear_bf16, training.attention_dropout
    training.linear_bf16, training.attention_dropout = _emu_linear, _emu_attention
    try:
        ref = _step(_switch(m64, route, "bf16"), _net_inputs(case), torch.float64)
        emu = _step(_switch(m, route, "bf16"), _net_inputs(case))
    finally:
        training.linear_bf16, training.attention_dropout = real
        _switch(m, ("torch",) * 4, "fp32")
        m.eval()
    assert set(ref) == set(emu)
    return ref, {k: _rel_l2(emu[k], ref[k]) for k in ref}


@pytest.mark.parametrize("others", ["torch", "hip"])
@pytest.mark.parametrize("case", list(NET_CASES))
def test_network_against_the_fp64_emulation(case, others):
    m, _ = _net()
    ref, e_emu = _reference(case, others)
    before = dict(training.LINEAR_COUNTERS)
    with T.deterministic_torch():
        got = _step(_switch(m, OTHERS[others], "bf16"), _net_inputs(case))
    _switch(m, ("torch",) * 4, "fp32")
    m.eval()
    calls, fallbacks = _expected_counts(m, case, OTHERS[others])
    assert calls > 0 and (fallbacks > 0) == (case == "1x8x8")
    assert training.LINEAR_COUNTERS == dict(before, calls=before["calls"] + calls, backward=before["backward"] + calls, fallbacks=before["fallbacks"] + fallbacks)
    assert set(got) == set(ref) and T.LOGITS in got
    worst, fails = (0.0, None, 0.0, 0.0), []
    for k in sorted(ref):
        assert torch.isfinite(got[k]).all(), k
        e_hip = _rel_l2(got[k].to(DEV), ref[k])
        ratio = e_hip / max(e_emu[k], U)
        if ratio > worst[0]:
            worst = (ratio, k, e_hip, e_emu[k])
        if not T.within_yardstick(e_hip, e_emu[k], U):
            fails.append("%s: e_hip %.3e exceeds %gx max(e_emu %.3e, %.3e)" % (k, e_hip, T.FACTOR, e_emu[k], U))
    print("train_linear parity network %s others=%s: largest e_hip / max(e_emu, 2^-24) = %.3f in %s (e_hip %.3e, e_emu %.3e); logits e_hip %.3e e_emu %.3e; "
          "%d calls, %d fallbacks" % ((case, others) + worst + (_rel_l2(got[T.LOGITS], ref[T.LOGITS]), e_emu[T.LOGITS], calls, fallbacks)))
    if case == "2x16x16":       # (the docstring of this file: at 1 x 8x8 a handful of flips decide this form; the form with the route's own rounding is asserted there)
        assert not fails, "%d tensors outside the yardstick:\n%s" % (len(fails), "\n".join(fails))


def _route_and_its_reference(case, others, hip):
    """one step on the HIP route (hip) or on the fp32 emulation, its routed linears recorded; then the fp64 module with those rounding decisions
    -> (the route's values, the fp64 values, the replay with its flip count)"""
    m, m64 = _net()
    ref_route = ("torch", "torch", others[2], "torch")
    real = training.linear_bf16, training.attention_dropout
    try:
        rec = _Record(real[0] if hip else _emu_linear)
        training.linear_bf16 = rec
        if not hip:
            training.attention_dropout = _emu_attention
        with T.deterministic_torch():
            got = _step(_switch(m, others if hip else ref_route, "bf16"), _net_inputs(case))
        assert all(g is not None for g in rec.g) and len(rec.x) == _expected_counts(m, case, others)[0]
        replay = _Replay(rec)
        training.linear_bf16, training.attention_dropout = replay, _emu_attention
        ref = _step(_switch(m64, ref_route, "bf16"), _net_inputs(case), torch.float64)
        assert replay.i == len(rec.x)
    finally:
        training.linear_bf16, training.attention_dropout = real
        _switch(m, ("torch",) * 4, "fp32")
        m.eval()
    return got, ref, replay


@pytest.mark.parametrize("others", ["torch", "hip"])
@pytest.mark.parametrize("case", list(NET_CASES))
def test_network_against_the_fp64_evaluation_with_the_routes_own_rounding(case, others):
    hip, ref_hip, rp_hip = _route_and_its_reference(case, OTHERS[others], True)
    emu, ref_emu, rp_emu = _route_and_its_reference(case, OTHERS[others], False)
    assert set(hip) == set(ref_hip) == set(emu) == set(ref_emu) and T.LOGITS in hip
    worst, fails = (0.0, None, 0.0, 0.0), []
    for k in sorted(hip):
        assert torch.isfinite(hip[k]).all(), k
        e_hip, e_emu = _rel_l2(hip[k], ref_hip[k]), _rel_l2(emu[k], ref_emu[k])
        ratio = e_hip / max(e_emu, U)
        if ratio > worst[0]:
            worst = (ratio, k, e_hip, e_emu)
        if not T.within_yardstick(e_hip, e_emu, U):
            fails.append("%s: e_hip %.3e exceeds %gx max(e_emu %.3e, %.3e)" % (k, e_hip, T.FACTOR, e_emu, U))
    print("train_linear parity network, the route's own rounding, %s others=%s: largest e_hip / max(e_emu, 2^-24) = %.3f in %s (e_hip %.3e, e_emu %.3e); elements whose "
          "fp64 value rounds to another bf16 than the route's fp32 value: HIP route %d of %d, fp32 emulation %d of %d"
          % ((case, others) + worst + (rp_hip.flips, rp_hip.rounded, rp_emu.flips, rp_emu.rounded)))
    assert not fails, "%d tensors outside the yardstick:\n%s" % (len(fails), "\n".join(fails))


def test_the_long_wgrad_reduction_is_split(built_lib):
    """(8192, 64, 64): the wgrad GEMM has one 64 x 64 output and a reduction of 8192 -- the launch rules split it over more workgroups than it has tiles, so its partial
    slabs and the ticket header the entry point zeroed are what test_op_against_the_rounded_operand_reference checks at that shape"""
    import ctypes

    import numpy as np
    lib = built_lib
    assert lib.paella_prof_enable(1) == 0
    try:
        _run_op(8192, 64, 64)
        torch.cuda.synchronize()
        n = lib.paella_prof_grid(None, 0)
        buf = np.zeros(4 * n, dtype=np.int64)
        lib.paella_prof_grid(buf.ctypes.data_as(ctypes.c_void_p), n)
    finally:
        lib.paella_prof_enable(0)
    launches = buf.reshape(n, 4)        # (tile config, workgroups, output tiles, bf16 operands) of forward, dgrad, wgrad
    assert n == 3 and (launches[:, 3] == 1).all(), launches
    cfg, G, tiles, _ = (int(v) for v in launches[2])
    print("train_linear parity op 8192x64x64 wgrad launch: tile config %d, %d workgroups over %d output tiles" % (cfg, G, tiles))
    assert G > tiles, launches


def test_forward_loss_takes_the_same_route_and_the_engine_never_sees_the_switch():
    m, _ = _net()
    case = "2x16x16"
    inp = _net_inputs(case)
    calls, fallbacks = _expected_counts(m, case, OTHERS["hip"])
    n0 = dict(training.LINEAR_COUNTERS)
    _step(_switch(m, OTHERS["hip"], "bf16"), inp)
    n1 = dict(training.LINEAR_COUNTERS)
    got = _step(m, inp, fused_loss=True)                      # `forward_loss`: the same route, the same increments
    n2 = dict(training.LINEAR_COUNTERS)
    assert {k: n1[k] - n0[k] for k in n0} == {k: n2[k] - n1[k] for k in n0} == dict(calls=calls, backward=calls, fallbacks=fallbacks, copied=n1["copied"] - n0["copied"])
    assert all(torch.isfinite(g).all() for g in got.values())
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    try:
        opt = training.ClippedAdamW(m.parameters(), lr=2e-3)
        opt.step()
        assert bool(torch.isfinite(opt.grad_norm))
        m.eval()
        g = torch.Generator().manual_seed(17)
        x = torch.randint(0, NET["num_labels"], (2, 16, 16), generator=g).to(DEV)
        r = torch.tensor([0.8, 0.3]).to(DEV)
        c = to_dev(inp[4], DEV)
        with torch.no_grad():
            n3 = dict(training.LINEAR_COUNTERS)
            with_bf16 = m(x, r, **c).clone()
            m.set_training_gemm("fp32")
            with_fp32 = m(x, r, **c)
            assert training.LINEAR_COUNTERS == n3              # eval mode never reaches the op
        assert torch.isfinite(with_bf16).all() and torch.equal(with_bf16, with_fp32)
        # ... and it serves the weights the optimizer wrote after the bf16 step: the same bits as a module built afresh from them, other bits than before the step
        fresh = paella_amd.Paella(**NET)
        fresh.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()})
        fresh = fresh.to(DEV)
        stale = paella_amd.Paella(**NET)
        stale.load_state_dict({k: v.cpu() for k, v in sd.items()})
        stale = stale.to(DEV)
        with torch.no_grad():
            assert torch.equal(fresh(x, r, **c), with_bf16) and not torch.equal(stale(x, r, **c), with_bf16)
    finally:
        m.load_state_dict(sd)
        m.zero_grad(set_to_none=True)
        _switch(m, ("torch",) * 4, "fp32")
        m.eval()
