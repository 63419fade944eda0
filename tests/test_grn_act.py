"""Training MLP activation without a GPU: the fp64 model the GPU tests measure against equals fp64 torch autograd of the expression `training._channelwise` runs
(GELU -> torch.norm over the positions -> channel mean -> divide -> gamma * (h * nx) + beta + h -> a dropout mask), a dead channel included; the C entry points
validate their arguments on the host before anything is enqueued; the Python surface refuses what the op cannot do instead of falling back."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import paella_amd
from oracle import golden_configs as G
from paella_amd import training
from tests import counter_noise as CN
from tests import grn_act_model as M
from tests import train_op_checks as T

ERR_ARG, ERR_WORKSPACE = -1, -3


def _inputs(B=3, P=13, C=20, seed=11, dead=True):
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(B, P, C, generator=g, dtype=torch.float64) * 1.5
    gamma = torch.randn(C, generator=g, dtype=torch.float64)
    beta = torch.randn(C, generator=g, dtype=torch.float64)
    dz = torch.randn(B, P, C, generator=g, dtype=torch.float64)
    if dead:
        u[1, :, 7] = 0.0   # a channel that is identically zero in one sample: Gx = 0 there
    return u, gamma, beta, dz


def reference_expression(u, gamma, beta, keep, scale):
    """the torch chain of training._channelwise between the two Linears, with the dropout as an explicit mask"""
    h = F.gelu(u)
    gx = torch.norm(h, p=2, dim=(1,), keepdim=True)
    nx = gx / (gx.mean(dim=-1, keepdim=True) + 1e-6)
    y = gamma * (h * nx) + beta + h
    return y * keep * scale


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_model_equals_fp64_autograd_of_the_reference_expression(p):
    u, gamma, beta, dz = _inputs()
    keep = M.keep_mask(tuple(u.shape), p, 1234) if p else None
    k64 = torch.ones_like(u) if keep is None else torch.from_numpy(keep).double()
    if p:
        assert 0 < int(keep.sum()) < keep.size
    uu, gg, bb = u.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    ref = reference_expression(uu, gg, bb, k64, M.scale_of(p))
    ref.backward(dz)
    z, Gx = M.forward(u, gamma, beta, keep, p)
    du, dgamma, dbeta = M.backward(u, gamma, dz, keep, p)
    assert float(Gx[1, 7]) == 0.0 and torch.isfinite(du).all() and torch.isfinite(uu.grad).all()
    torch.testing.assert_close(z, ref.detach(), rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(du, uu.grad, rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(dgamma, gg.grad, rtol=1e-12, atol=1e-13)
    torch.testing.assert_close(dbeta, bb.grad, rtol=1e-12, atol=1e-13)


def test_keep_mask_is_the_documented_word_of_the_documented_counter():
    shape, p, seed = (2, 3, 8), 0.3, (1 << 63) + 12345
    keep = M.keep_mask(shape, p, seed).reshape(-1)
    for e in (0, 1, 5, 30, 47):
        w = CN.philox4x32_scalar((seed ^ M.DROPOUT_SALT) & CN.M64, e >> 2, 0)[e & 3]
        assert bool(keep[e]) == ((w >> 8) * 2.0 ** -24 >= float(np.float32(p)))
    assert not np.array_equal(keep, M.keep_mask(shape, p, seed + 1).reshape(-1))
    assert M.scale_of(0.0) == 1.0 and M.scale_of(0.5) == 2.0


def test_argument_validation_without_gpu(built_lib):
    """every refusal comes from the host checks, before any device work: the pointers below are never dereferenced"""
    lib = built_lib
    p = ctypes.c_void_p(4096)  # stands for any non-NULL, 16-byte aligned device pointer
    B, P, C = 4, 64, 256
    need = lib.paella_grn_act_workspace_bytes(B, P, C)
    assert need > 0

    def fwd(B=B, P=P, C=C, p_drop=0.1, u=p, ws=p, ws_bytes=need):
        return lib.paella_grn_act_forward(u, p, p, B, P, C, p_drop, 7, p, p, ws, ws_bytes, None)

    def bwd(B=B, P=P, C=C, p_drop=0.1, u=p, ws=p, ws_bytes=need):
        return lib.paella_grn_act_backward(u, p, p, p, B, P, C, p_drop, 7, p, p, p, ws, ws_bytes, None)

    for call in (fwd, bwd):
        for bad in (dict(C=0), dict(C=6), dict(C=16388), dict(P=0), dict(P=(1 << 20) + 1), dict(B=0), dict(B=65536), dict(p_drop=1.0), dict(p_drop=-0.1),
                    dict(p_drop=float("nan")), dict(u=None), dict(u=ctypes.c_void_p(4100))):
            assert call(**bad) == ERR_ARG, bad
            assert lib.paella_last_error()
        assert call(ws_bytes=need - 1) == ERR_WORKSPACE
        assert b"workspace" in lib.paella_last_error()
        assert call(ws=None) == ERR_WORKSPACE
    for B_, P_, C_ in [(B, P, 6), (B, P, 0), (B, P, 16388), (0, P, C), (65536, P, C), (B, 0, C), (B, (1 << 20) + 1, C)]:
        assert lib.paella_grn_act_workspace_bytes(B_, P_, C_) == 0
    # the bound of the header: two sets of partials of at most an eighth of the activation each (a strip is at least 8 rows), three [B, C] tables, one [B] table
    for B_, P_, C_ in [(16, 256, 2560), (16, 64, 5120), (16, 16, 5120), (1, 1 << 20, 16), (3, 65, 132), (1025, 1024, 1024)]:
        b = lib.paella_grn_act_workspace_bytes(B_, P_, C_)
        assert 0 < b <= 2 * (B_ * ((P_ + 7) // 8) * C_ * 4 + 256) + 3 * (B_ * C_ * 4 + 256) + B_ * 4 + 256, (B_, P_, C_, b)
    # the extremes of the range are sized without overflow
    assert lib.paella_grn_act_workspace_bytes(65535, 1 << 20, 16384) > 0


def test_gelu_grn_dropout_refuses_what_the_op_cannot_do():
    u, gamma, beta, _ = _inputs(B=2, P=5, C=8, dead=False)
    u, gamma, beta = u.float(), gamma.float(), beta.float()
    with pytest.raises(ValueError, match="HIP device"):     # cpu tensors: there is no torch fallback
        training.gelu_grn_dropout(u, gamma, beta, 0.1)
    with pytest.raises(ValueError, match="fp32"):
        training.gelu_grn_dropout(u.double(), gamma, beta)
    with pytest.raises(ValueError, match="fp32"):
        training.gelu_grn_dropout(u, gamma.half(), beta)
    with pytest.raises(ValueError, match="multiple of 4"):
        training.gelu_grn_dropout(u[..., :6], gamma[:6], beta[:6])
    with pytest.raises(ValueError, match="multiple of 4"):
        training.gelu_grn_dropout(torch.zeros(1, 2, 16388), torch.zeros(16388), torch.zeros(16388))
    for p in (1.0, -0.1, float("nan"), 1.5):
        with pytest.raises(ValueError, match=r"\[0, 1\)"):
            training.gelu_grn_dropout(u, gamma, beta, p)
    with pytest.raises(ValueError, match="elements"):
        training.gelu_grn_dropout(u, gamma[:4], beta)
    with pytest.raises(ValueError, match="elements"):
        training.gelu_grn_dropout(u, gamma, torch.zeros(16))
    with pytest.raises(ValueError, match=r"\[B, \.\.\., C\]"):
        training.gelu_grn_dropout(u[0, 0], gamma, beta)
    with pytest.raises(ValueError, match="tensors"):
        training.gelu_grn_dropout(u, None, beta)


def test_set_training_activation():
    """(what every switch's setter does: tests/test_training.py::test_training_switch)"""
    paella_amd.Paella(**G.UNET_TINY).set_training_activation("hip")
    assert not hasattr(paella_amd, "gelu_grn_dropout")   # nothing new at the package root beyond the method


def test_the_switch_leaves_a_cpu_train_step_alone():
    T.assert_switch_leaves_a_cpu_train_step_alone(lambda m: m.set_training_activation("hip"))
