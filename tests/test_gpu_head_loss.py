"""GPU: the training loss head (paella_amd/csrc/loss.hip) against the fp64 model of tests/head_loss_model.py.

The yardstick of every accuracy check is MEASURED in the same test, not picked here: the torch fp32 path the training step ran before this op existed
(F.conv2d with out_mapper's weight + nn.CrossEntropyLoss + backward) runs on the same device and inputs, its max abs error against the fp64 model is
taken for each of loss, dh and dw, and the fused op must stay within 4x that error -- both are fp32 sums of up to 8192 terms in different orders.
The measured pairs are kept in profiles/head_loss_parity.txt."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

from oracle import golden_configs as G
from paella_amd import _lib, training
from tests import head_loss_model as M
from tests import train_op_checks as T
from tests.helpers import to_dev

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(1, 64, 32), (63, 64, 32), (65, 128, 32), (130, 1024, 64), (200, 80, 48), (257, 8192, 256)]
FACTOR = T.FACTOR
_err = T.err


@functools.lru_cache(maxsize=None)
def _inputs(rows, N, K, scale=1.0):
    """seeded normal h, w of std 1 / sqrt(K) (unit-scale logits), targets, and g uniform in [0, 2] with a tenth of the rows exactly 0"""
    gen = torch.Generator().manual_seed(1000 * rows + N + K)
    h = (torch.randn(rows, K, generator=gen) * scale).to(DEV)
    w = (torch.randn(N, K, generator=gen) / K ** 0.5).to(DEV)
    t = torch.randint(0, N, (rows,), generator=gen).to(DEV)
    g = torch.rand(rows, generator=gen) * 2
    g[torch.randperm(rows, generator=gen)[: max(rows // 10, 1 if rows >= 10 else 0)]] = 0
    return h, w, t, g.to(DEV)


@functools.lru_cache(maxsize=None)
def _model(rows, N, K, eps, scale=1.0):
    h, w, t, g = _inputs(rows, N, K, scale)
    loss, lse, argmax, l = M.forward(h, w, t, eps)
    dh, dw = M.backward(h, w, t, eps, g)
    return loss, lse, argmax, M.top2_gap(l), dh, dw


def fused(h, w, t, eps, g=None, want_dh=True, want_dw=True, want_argmax=True, ws=None):
    """the raw op: forward, and backward when g is given -> dict of outputs.  The workspace is filled with 0xFF bytes (NaN as floats) before each direction: it
    needs no set-up, and neither direction reads what it did not write."""
    lib = _lib.load()
    rows, K = h.shape
    N = w.size(0)
    if ws is None:
        ws = torch.empty(lib.paella_head_loss_workspace_bytes(rows, N, K), dtype=torch.uint8, device=h.device)
    ws.fill_(255)
    out = dict(loss=torch.empty(rows, device=DEV), lse=torch.empty(rows, device=DEV), argmax=torch.full((rows,), -7, dtype=torch.int32, device=DEV) if want_argmax else None)
    _lib.check(lib.paella_head_loss_forward(_lib.ptr(h), _lib.ptr(w), _lib.ptr(t), rows, N, K, eps, _lib.ptr(out["loss"]), _lib.ptr(out["lse"]), _lib.ptr(out["argmax"]),
                                            _lib.ptr(ws), ws.numel(), _lib.stream_ptr(h.device)))
    if g is not None:
        ws.fill_(255)
        out["dh"] = torch.full_like(h, float("nan")) if want_dh else None   # WRITTEN, not accumulated into: the poison must be gone
        out["dw"] = torch.full_like(w, float("nan")) if want_dw else None
        _lib.check(lib.paella_head_loss_backward(_lib.ptr(h), _lib.ptr(w), _lib.ptr(t), _lib.ptr(out["lse"]), _lib.ptr(g), rows, N, K, eps, _lib.ptr(out["dh"]),
                                                 _lib.ptr(out["dw"]), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(h.device)))
    return out


def torch_path(h, w, t, eps, g):
    """what the training step computed before the fused op: the 1x1 convolution over the NHWC-backed NCHW view + CrossEntropyLoss(reduction='none') + backward"""
    rows, K = h.shape
    hh = h.clone().requires_grad_(True)
    ww = w.clone().view(w.size(0), K, 1, 1).requires_grad_(True)
    pred = F.conv2d(hh.view(1, rows, 1, K).permute(0, 3, 1, 2), ww)
    loss = nn.CrossEntropyLoss(label_smoothing=eps, reduction='none')(pred, t.view(1, rows, 1)).view(rows)
    loss.backward(g)
    return loss.detach(), hh.grad, ww.grad.view(w.size(0), K)


def _check_against_model(tag, got, ref_path, model):
    """got / ref_path = (loss, dh, dw) of the fused op / of the torch fp32 path; model = the fp64 values.  Prints every pair, then asserts."""
    pairs = []
    for name, a, b, m in zip(("loss", "dh", "dw"), got, ref_path, model):
        assert torch.isfinite(a).all(), "%s %s: not finite" % (tag, name)
        pairs.append((name, _err(a, m), _err(b, m)))
    print("head_loss parity %s: " % tag + "  ".join("%s fused %.3e torch %.3e" % p for p in pairs))
    for name, e_fused, e_torch in pairs:
        # measured pairs (fused / torch, MI355X; all of them in profiles/head_loss_parity.txt).  Unit-scale logits: loss 0.4x ... 1.1x, dh 0.02x ... 0.6x, dw 0.4x ... 2.1x
        # of the torch path's error; (257, 8192, 256): loss 1.6e-6 / 3.9e-6, dh 8.9e-8 / 4.9e-7, dw 3.4e-6 / 3.6e-6.  Logits of order 100: 0.02x ... 2.8x; the
        # largest are (63, 64, 32): loss 3.95e-5 / 1.84e-5, dh 1.85e-6 / 7.1e-7, dw 5.96e-4 / 2.16e-4
        assert T.within_yardstick(e_fused, e_torch), "%s %s: fused error %.3e exceeds %gx the torch fp32 path's %.3e" % (tag, name, e_fused, FACTOR, e_torch)


@pytest.mark.parametrize("scale", [1.0, 64.0])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_accuracy_and_argmax_against_the_fp64_model(built_lib, shape, eps, scale):
    """scale 64: logits of order +-60 ... 100 -- everything stays finite and the same error rule holds.  At that size the rounding of the LOGITS decides the
    gradients' error: one fp32 multiply-add chain over K = 32 ends 4.8e-5 (3 ulp) from the fp64 logit and put dh 5x ... 12x above a torch path whose convolution
    accumulates small-K logits more precisely (it picks its algorithm per run: the torch figures of these cases move by 10x between runs).  The kernels therefore cut
    the chain every 16 columns of K and add the chunk sums error-free (loss.hip: Logits); emulating that on the CPU in the kernel's order predicts the measured dh
    and dw to three digits."""
    h, w, t, g = _inputs(*shape, scale)
    loss64, lse64, argmax64, gap, dh64, dw64 = _model(*shape, eps, scale)
    out = fused(h, w, t, eps, g)
    _check_against_model("%s eps=%g scale=%g" % (shape, eps, scale), (out["loss"], out["dh"], out["dw"]), torch_path(h, w, t, eps, g), (loss64, dh64, dw64))
    assert torch.isfinite(out["lse"]).all()
    torch.testing.assert_close(out["lse"].double(), lse64, rtol=1e-5, atol=1e-5)
    clear = gap >= 1e-5   # rows whose fp64 top-two gap is under 1e-5 may go either way; for these inputs none is expected
    assert int((~clear).sum()) * 100 <= shape[0]
    assert torch.equal(out["argmax"].long()[clear], argmax64[clear])


@pytest.mark.parametrize("shape", [(65, 128, 32), (130, 1024, 64), (200, 80, 48)], ids=lambda s: "x".join(map(str, s)))
def test_argmax_tie_returns_the_lowest_label_across_tiles(built_lib, shape):
    rows, N, K = shape
    h, w, t, _ = _inputs(*shape)
    w = w.clone()
    w[70] = w[3]
    w[N - 1] = w[3]
    h = (w[3] * 8)[None, :].repeat(rows, 1).contiguous()   # aligned with the three identical rows: they share the largest logit, bit for bit
    out = fused(h, w, t, 0.0)
    l = M.logits64(h, w)
    assert torch.equal(l.argmax(1).new_full((rows,), 3), M.forward(h, w, t, 0.0)[2])
    assert torch.equal(out["argmax"].long(), torch.full((rows,), 3, device=DEV))


@pytest.mark.parametrize("shape", [(130, 1024, 64), (200, 80, 48), (257, 8192, 256)], ids=lambda s: "x".join(map(str, s)))
def test_ignored_rows(built_lib, shape):
    rows, N, K = shape
    eps = 0.1
    h, w, t, g = _inputs(*shape)
    g = g.clamp_min(0.25)
    ign = torch.arange(rows, device=DEV) % 5 == 2
    bad = torch.tensor([-100, -1, N, 2 ** 40], device=DEV)[torch.arange(rows, device=DEV) % 4]
    t_ign = torch.where(ign, bad, t)
    out = fused(h, w, t_ign, eps, g)
    assert torch.all(out["loss"][ign] == 0) and torch.all(out["dh"][ign] == 0)
    assert torch.isfinite(out["lse"]).all() and int(out["argmax"].min()) >= 0 and int(out["argmax"].max()) < N
    # dw against the fp64 model WITHOUT those rows; the torch path sees them as ignore_index
    keep = ~ign
    loss64, _, _, _ = M.forward(h[keep], w, t[keep], eps)
    dh64, dw64 = M.backward(h[keep], w, t[keep], eps, g[keep])
    tl, tdh, tdw = torch_path(h, w, torch.where(ign, torch.full_like(t, -100), t), eps, g)
    _check_against_model("%s ignored rows" % (shape,), (out["loss"][keep], out["dh"][keep], out["dw"]), (tl[keep], tdh[keep], tdw), (loss64, dh64, dw64))
    # the other rows are unaffected: the bits of the run where those rows carry g = 0 and a valid target
    ref = fused(h, w, t, eps, torch.where(ign, torch.zeros_like(g), g))
    assert torch.equal(out["loss"][keep], ref["loss"][keep]) and torch.equal(out["dh"][keep], ref["dh"][keep])
    assert torch.equal(out["dw"], ref["dw"]) and torch.equal(out["lse"], ref["lse"]) and torch.equal(out["argmax"], ref["argmax"])


@pytest.mark.parametrize("shape", [(130, 1024, 64), (257, 8192, 256)], ids=lambda s: "x".join(map(str, s)))
def test_null_outputs_and_determinism(built_lib, shape):
    h, w, t, g = _inputs(*shape)
    full = fused(h, w, t, 0.1, g)
    again = fused(h, w, t, 0.1, g)
    for k in ("loss", "lse", "argmax", "dh", "dw"):
        assert torch.equal(full[k], again[k]), k
    no_dh = fused(h, w, t, 0.1, g, want_dh=False)
    no_dw = fused(h, w, t, 0.1, g, want_dw=False, want_argmax=False)
    assert no_dh["dh"] is None and torch.equal(no_dh["dw"], full["dw"])
    assert no_dw["dw"] is None and torch.equal(no_dw["dh"], full["dh"])
    assert torch.equal(no_dw["loss"], full["loss"]) and torch.equal(no_dw["lse"], full["lse"])


def test_autograd_function(built_lib):
    shape = (2 * 8 * 8 + 2, 1024, 64)   # 130 rows as [B, H, W] would not factor: use a [2, 5, 13] grid
    B, H, W = 2, 5, 13
    N, K, eps = 1024, 64, 0.1
    h, w, t, g = _inputs(*shape)
    lw = (g.view(B, H, W) + 0.25)
    tgt = t.view(B, H, W)

    def reduce(loss):
        return ((loss * lw).sum(dim=[1, 2]) / lw.sum(dim=[1, 2])).mean()

    # the torch path and the fp64 model of the same weighted, reduced loss
    h64 = h.double().requires_grad_(True)
    w64 = w.double().requires_grad_(True)
    reduce(F.cross_entropy(h64 @ w64.t(), t, label_smoothing=eps, reduction='none').view(B, H, W)).backward()
    h32 = h.clone().requires_grad_(True)
    w32 = w.clone().view(N, K, 1, 1).requires_grad_(True)
    pred = F.conv2d(h32.view(B, H, W, K).permute(0, 3, 1, 2), w32)
    l32 = reduce(nn.CrossEntropyLoss(label_smoothing=eps, reduction='none')(pred, tgt))
    l32.backward()

    hf = h.clone().requires_grad_(True)
    wf = w.clone().view(N, K, 1, 1).requires_grad_(True)
    loss, argmax = training.head_cross_entropy(hf.view(B, H, W, K), wf, tgt, eps)
    assert loss.shape == (B, H, W) and argmax.shape == (B, H, W) and argmax.dtype == torch.int32 and loss.requires_grad and not argmax.requires_grad
    lf = reduce(loss)
    lf.backward()
    assert torch.equal(argmax.view(-1).long(), pred.detach().argmax(1).view(-1))
    np.testing.assert_allclose(float(lf.detach()), float(l32.detach()), rtol=2e-6)
    for name, a, b, m in (("dh", hf.grad, h32.grad, h64.grad), ("dw", wf.grad.view(N, K), w32.grad.view(N, K), w64.grad)):
        e_f, e_t = _err(a, m), _err(b, m)
        print("head_loss parity autograd %s: fused %.3e torch %.3e" % (name, e_f, e_t))
        assert T.within_yardstick(e_f, e_t), name

    # a frozen head: no weight gradient, the same h gradient bits
    hz = h.clone().requires_grad_(True)
    wz = w.clone().requires_grad_(False)
    reduce(training.head_cross_entropy(hz.view(B, H, W, K), wz, tgt, eps)[0]).backward()
    assert wz.grad is None and torch.equal(hz.grad, hf.grad)

    # the permuted view `_ln_nchw` returns (NCHW shape over NHWC memory), permuted back, is taken without a copy and gives the bits of its contiguous copy
    nchw = h.view(B, H, W, K).permute(0, 3, 1, 2)
    assert not nchw.is_contiguous()
    a = training.head_cross_entropy(nchw.permute(0, 2, 3, 1), w, tgt, eps)
    b = training.head_cross_entropy(nchw.permute(0, 2, 3, 1).contiguous().clone(), w, tgt, eps)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[0], loss.detach())
    # and a view whose rows are NOT contiguous is copied, not misread
    wide = torch.randn(B, H, W, 2 * K, device=DEV)
    c = training.head_cross_entropy(wide[..., :K], w, tgt, eps)
    d = training.head_cross_entropy(wide[..., :K].contiguous(), w, tgt, eps)
    assert torch.equal(c[0], d[0])
    with pytest.raises(ValueError, match="256"):
        training.head_cross_entropy(torch.zeros(4, 272, device=DEV), torch.zeros(64, 272, device=DEV), torch.zeros(4, dtype=torch.long, device=DEV))


@pytest.mark.parametrize("which", ["tiny", "variant"])
def test_train_step_with_fused_head_reproduces_the_reference(golden, built_lib, which):
    """_train_step of tests/test_gpu_training.py with forward_loss in place of model(...) + CrossEntropyLoss, against the reference's recorded step"""
    cfg, m = T.model_for(which, golden, DEV)
    g = golden("train_%s_step" % which)
    latents, t, mask, random_x, c = G.train_step_inputs(cfg)
    latents, t, mask, random_x = latents.to(DEV), t.to(DEV), mask.to(DEV), random_x.to(DEV)
    c = to_dev(c, DEV)
    m.train()
    m.dropout = 0.0
    m.zero_grad(set_to_none=True)
    noised = latents * (1 - mask) + random_x * mask
    lw = m.get_loss_weight(t, mask)
    loss, correct = m.forward_loss(noised, t, latents, **c)
    assert loss.shape == latents.shape and correct.shape == latents.shape and correct.dtype == torch.bool
    loss = ((loss * lw).sum(dim=[1, 2]) / lw.sum(dim=[1, 2])).mean()
    loss.backward()
    T.assert_recorded_step(m, g, loss)
    with torch.no_grad():
        pred = m(noised, t, **c)   # the logits path on the same step
    assert float(correct.float().mean()) == float((pred.argmax(1) == latents).float().mean())
    m.eval()
    with pytest.raises(RuntimeError, match=r"model\.train\(\)"):
        m.forward_loss(noised, t, latents, **c)


def test_graph_capture_replays_the_eager_bits(built_lib):
    shape = (130, 1024, 64)
    h, w, t, g = _inputs(*shape)
    eager = fused(h, w, t, 0.1, g)
    ws = torch.empty(_lib.load().paella_head_loss_workspace_bytes(*shape), dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fused(h, w, t, 0.1, g, ws=ws)   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = fused(h, w, t, 0.1, g, ws=ws)
    for _ in range(2):
        for k in ("loss", "lse", "dh", "dw"):
            out[k].fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for k in ("loss", "lse", "argmax", "dh", "dw"):
            assert torch.equal(out[k], eager[k]), k
