"""Training ResBlock front without a GPU: the fp64 model the GPU tests measure against equals fp64 torch autograd of the chain `training._res_block` runs
(torch.cat -> F.conv2d(groups=C) -> F.layer_norm over the channels), one-position images and a constant row included; the C entry points validate their
arguments on the host before anything is enqueued; the Python surface refuses what the op cannot do instead of falling back."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import paella_amd
from oracle import golden_configs as G
from paella_amd import training
from tests import dwconv_ln_model as M
from tests import train_op_checks as T

ERR_ARG, ERR_WORKSPACE = -1, -3


def _inputs(B, H, W, C, skip, seed=7):
    g = torch.Generator().manual_seed(seed)
    J = 2 if skip else 1
    x = torch.randn(B, H, W, C, generator=g, dtype=torch.float64)
    s = torch.randn(B, H, W, C, generator=g, dtype=torch.float64) if skip else None
    w = torch.randn(C, J, 3, 3, generator=g, dtype=torch.float64) * 0.4
    bias = torch.randn(C, generator=g, dtype=torch.float64)
    dy = torch.randn(B, H, W, C, generator=g, dtype=torch.float64)
    return x, s, w, bias, dy


def reference_chain(x, skip, w, bias, dy):
    """fp64 autograd of the torch chain of training._res_block, NHWC in and out -> (y, dx, dskip, dw, dbias)"""
    leaves = [t.clone().requires_grad_(True) if t is not None else None for t in (x, skip, w, bias)]
    xx, ss, ww, bb = leaves
    xc = xx.permute(0, 3, 1, 2)
    if ss is not None:
        xc = torch.cat([xc, ss.permute(0, 3, 1, 2)], dim=1)
    C = w.size(0)
    y = F.layer_norm(F.conv2d(xc, ww, bb, padding=1, groups=C).permute(0, 2, 3, 1), (C,), None, None, M.EPS)
    y.backward(dy)
    return (y.detach(),) + tuple(None if t is None else t.grad for t in leaves)


def _compare(x, s, w, bias, dy):
    ref = reference_chain(x, s, w, bias, dy)
    y, rstd = M.forward(x, s, w, bias)
    got = (y,) + M.backward(x, s, w, bias, dy)
    for name, a, b in zip(("y", "dx", "dskip", "dw", "dbias"), got, ref):
        if b is None:
            assert a is None, name
            continue
        assert torch.isfinite(a).all() and torch.isfinite(b).all(), name
        torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-13, msg=lambda m: "%s: %s" % (name, m))
    return y, rstd


@pytest.mark.parametrize("shape", [(1, 1, 1, 4, False), (2, 1, 5, 8, True), (2, 3, 2, 20, False), (3, 5, 13, 24, True)], ids=lambda s: "x".join(map(str, s)))
def test_model_equals_fp64_autograd_of_the_torch_chain(shape):
    _compare(*_inputs(*shape))


@pytest.mark.parametrize("skip", [False, True])
def test_model_on_a_constant_row(skip):
    """x = 0 and one bias for every channel: the convolution output is constant over C, the variance 0, y = 0 exactly and the gradients finite (rstd = 1000)"""
    x, s, w, bias, dy = _inputs(2, 3, 4, 8, skip)
    x.zero_()
    if s is not None:
        s.zero_()
    bias.fill_(0.5)
    y, rstd = _compare(x, s, w, bias, dy)
    assert torch.all(y == 0) and torch.allclose(rstd, torch.full_like(rstd, 1000.0))


def test_argument_validation_without_gpu(built_lib):
    """every refusal comes from the host checks, before any device work: the pointers below are never dereferenced"""
    lib = built_lib
    p = ctypes.c_void_p(4096)  # stands for any non-NULL, 16-byte aligned device pointer
    B, H, W, C = 4, 8, 8, 256
    size = lib.paella_dwconv_ln_train_workspace_bytes

    def fwd(B=B, H=H, W=W, C=C, skip=None, x=p, ws=p, ws_bytes=None, eps=1e-6):
        if ws_bytes is None:
            ws_bytes = 1 << 40
        return lib.paella_dwconv_ln_train_forward(x, skip, p, p, B, H, W, C, eps, p, p, ws, ws_bytes, None)

    def bwd(B=B, H=H, W=W, C=C, skip=None, x=p, ws=p, ws_bytes=None, dskip=None):
        if ws_bytes is None:
            ws_bytes = 1 << 40
        return lib.paella_dwconv_ln_train_backward(x, skip, p, p, p, p, B, H, W, C, p, dskip, p, p, ws, ws_bytes, None)

    for call in (fwd, bwd):
        for bad in (dict(C=0), dict(C=6), dict(C=8196), dict(C=4100, skip=p), dict(C=12, skip=p), dict(H=0), dict(W=0), dict(B=0), dict(B=-1),
                    dict(B=1 << 11, H=1 << 10, W=1 << 10), dict(x=None), dict(x=ctypes.c_void_p(4100)), dict(skip=ctypes.c_void_p(4100)),
                    dict(ws=ctypes.c_void_p(4100))):
            assert call(**bad) == ERR_ARG, bad
            assert lib.paella_last_error()
    for eps in (0.0, -1.0, float("nan"), float("inf")):
        assert fwd(eps=eps) == ERR_ARG, eps
    assert bwd(dskip=p) == ERR_ARG and b"dskip" in lib.paella_last_error()
    # the workspace: the forward asks for the repacked weights only, the backward for everything
    for has_skip, skip in ((0, None), (1, p)):
        need_f = size(1, 1, 1, C, has_skip)
        need_b = size(B, H, W, C, has_skip)
        assert need_f == 36 * (1 + has_skip) * C and need_b >= B * H * W * C * 4
        assert fwd(skip=skip, ws_bytes=need_f - 1) == ERR_WORKSPACE and b"workspace" in lib.paella_last_error()
        assert bwd(skip=skip, ws_bytes=need_b - 1) == ERR_WORKSPACE and b"workspace" in lib.paella_last_error()
        assert fwd(skip=skip, ws=None) == ERR_WORKSPACE and bwd(skip=skip, ws=None) == ERR_WORKSPACE


def test_workspace_bytes(built_lib):
    size = built_lib.paella_dwconv_ln_train_workspace_bytes
    for B, H, W, C, s in [(1, 1, 1, 0, 0), (1, 1, 1, 6, 0), (1, 1, 1, 8196, 0), (1, 1, 1, 4100, 1), (1, 1, 1, 12, 1), (1, 1, 1, 4, 1), (0, 4, 4, 64, 0), (2, 0, 4, 64, 0),
                          (2, 4, 0, 64, 1), (-1, 4, 4, 64, 0), (1 << 11, 1 << 10, 1 << 10, 64, 0), (1 << 16, 1 << 16, 1 << 16, 64, 0)]:
        assert size(B, H, W, C, s) == 0, (B, H, W, C, s)
    # the documented bound: da (one activation tensor) + partials under a quarter of one + three roundings to 256 bytes for the backward, the repacked weights
    # (36 J C bytes, rounded) for the forward; the call returns the larger
    for B, H, W, C, s in [(16, 16, 16, 640, 0), (16, 16, 16, 640, 1), (16, 8, 8, 1280, 1), (16, 4, 4, 1280, 0), (3, 5, 13, 136, 1), (1, 1, 1, 8192, 0), (1, 1, 1, 4096, 1),
                          (1, 9, 9, 4096, 1), (2, 1, 5, 8, 1), (1025, 32, 32, 1024, 0), (7, 191, 3, 20, 0)]:
        act = B * H * W * C * 4
        fwd = (36 * (1 + s) * C + 255) // 256 * 256
        got = size(B, H, W, C, s)
        assert got >= act and got >= fwd, (B, H, W, C, s, got)
        assert got <= max(fwd, act + act // 4 + 768), (B, H, W, C, s, got)
        assert got <= max(64 * 1024 + 36 * (1 + s) * C, act + act // 4 + 64 * 1024)   # the issue's bound
    # the extremes of the range are sized without overflow
    top = size(1, 1, 2 ** 31 - 1, 8192, 0)
    assert (2 ** 31 - 1) * 8192 * 4 <= top <= (2 ** 31 - 1) * 8192 * 5 + 768
    top = size(2 ** 31 - 1, 1, 1, 4096, 1)
    assert (2 ** 31 - 1) * 4096 * 4 <= top <= (2 ** 31 - 1) * 4096 * 5 + 768


def test_dwconv_layernorm_refuses_what_the_op_cannot_do():
    x, s, w, bias, _ = _inputs(2, 3, 4, 8, True)
    x, s, w, bias = x.float().permute(0, 3, 1, 2), s.float().permute(0, 3, 1, 2), w.float(), bias.float()
    with pytest.raises(ValueError, match="HIP device"):     # cpu tensors: there is no torch fallback
        training.dwconv_layernorm(x, w, bias, s)
    with pytest.raises(ValueError, match="HIP device"):
        training.dwconv_layernorm(x, w[:, :1].contiguous(), bias)
    with pytest.raises(ValueError, match="fp32"):
        training.dwconv_layernorm(x.double(), w, bias, s)
    with pytest.raises(ValueError, match="fp32"):
        training.dwconv_layernorm(x, w.half(), bias, s)
    with pytest.raises(ValueError, match="fp32"):
        training.dwconv_layernorm(x, w, bias, s.double())
    with pytest.raises(ValueError, match="3 x 3"):
        training.dwconv_layernorm(x, torch.zeros(8, 2, 5, 5), bias, s)
    with pytest.raises(ValueError, match="3 x 3"):
        training.dwconv_layernorm(x, torch.zeros(8, 2, 1, 1), bias, s)
    with pytest.raises(ValueError, match="shape of x"):
        training.dwconv_layernorm(x, w, bias, s[:, :4])
    with pytest.raises(ValueError, match="shape of x"):
        training.dwconv_layernorm(x, w, bias, s[:1])
    with pytest.raises(ValueError, match=r"\[C, 1, 3, 3\]"):   # a two-group weight without a skip
        training.dwconv_layernorm(x, w, bias)
    with pytest.raises(ValueError, match=r"\[C, 2, 3, 3\]"):
        training.dwconv_layernorm(x, w[:, :1], bias, s)
    with pytest.raises(ValueError, match="bias"):
        training.dwconv_layernorm(x, w, bias[:4], s)
    with pytest.raises(ValueError, match="multiple of 4"):
        training.dwconv_layernorm(torch.zeros(1, 6, 2, 2), torch.zeros(6, 1, 3, 3), torch.zeros(6))
    with pytest.raises(ValueError, match="multiple of 4"):
        training.dwconv_layernorm(torch.zeros(1, 8196, 1, 1), torch.zeros(8196, 1, 3, 3), torch.zeros(8196))
    with pytest.raises(ValueError, match="multiple of 8"):
        training.dwconv_layernorm(torch.zeros(1, 12, 2, 2), torch.zeros(12, 2, 3, 3), torch.zeros(12), torch.zeros(1, 12, 2, 2))
    with pytest.raises(ValueError, match="multiple of 8"):
        training.dwconv_layernorm(torch.zeros(1, 4104, 1, 1), torch.zeros(4104, 2, 3, 3), torch.zeros(4104), torch.zeros(1, 4104, 1, 1))
    with pytest.raises(ValueError, match="positions"):
        training.dwconv_layernorm(torch.zeros(0, 8, 2, 2), torch.zeros(8, 1, 3, 3), torch.zeros(8))
    with pytest.raises(ValueError, match=r"\[B, C, H, W\]"):
        training.dwconv_layernorm(x[0], w, bias, s[0])
    with pytest.raises(ValueError, match="eps"):
        training.dwconv_layernorm(x, w, bias, s, eps=0.0)
    with pytest.raises(ValueError, match="tensors"):
        training.dwconv_layernorm(x, None, bias)


def test_set_training_depthwise():
    """(what every switch's setter does: tests/test_training.py::test_training_switch)  Its own: the kernel_size rule, through every entry point"""
    names = set(dir(paella_amd))
    k5 = paella_amd.Paella(**dict(G.UNET_TINY, kernel_size=5))
    assert k5.set_training_depthwise("torch") is k5 and k5.set_training_route(depthwise="torch", attention="hip") is k5
    for refused in (lambda: k5.set_training_depthwise("hip"), lambda: k5.set_training_route(depthwise="hip"), lambda: k5.set_training_route(attention="torch", depthwise="hip")):
        with pytest.raises(ValueError, match="kernel_size 3"):
            refused()
        assert k5._train_depthwise == "torch" and k5._train_attention == "hip"
    assert paella_amd.Paella(**G.UNET_TINY).set_training_depthwise("hip")._train_depthwise == "hip"
    assert set(dir(paella_amd)) == names and not hasattr(paella_amd, "dwconv_layernorm")   # nothing new at the package root beyond the method


@pytest.mark.parametrize("act", ["torch", "hip"])
def test_the_switch_leaves_a_cpu_train_step_alone(act):
    T.assert_switch_leaves_a_cpu_train_step_alone(lambda m: m.set_training_depthwise("hip"), before=lambda m: m.set_training_activation(act))
