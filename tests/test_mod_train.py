"""Training timestep modulation without a GPU: the fp64 model the GPU tests measure against equals fp64 torch autograd of the chain the network runs by default
(the residual add, `training._timestep_block`'s chunk and x (1 + a) + b, F.layer_norm over the channels), a = -1 and a constant row included; the C entry points
validate their arguments on the host before anything is enqueued; the Python surface refuses what the op cannot do instead of falling back; the switch."""
import ctypes
import itertools

import pytest
import torch
import torch.nn.functional as F

import paella_amd
from oracle import golden_configs as G
from paella_amd import training
from tests import mod_ln_model as M
from tests import train_op_checks as T

ERR_ARG, ERR_WORKSPACE = -1, -3


def _inputs(B, H, W, C, seed=7):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return dict(x=r(B, C, H, W), res=r(B, C, H, W), ab=r(B, 2 * C) * 0.5, dxp=r(B, C, H, W), dz=r(B, H * W, C))


def reference_chain(x, ab, res, dxp, dz):
    """fp64 autograd of the plain formulation, logical [B, C, H, W] in -> (x' [B, P, C], z [B, P, C], dx [B, P, C], dres or None, dab [B, 2C])"""
    leaves = [t.clone().requires_grad_(True) if t is not None else None for t in (x, ab, res)]
    xx, aa, rr = leaves
    B, C = x.shape[:2]
    h = xx if rr is None else xx + rr
    a, b = aa[:, :, None, None].chunk(2, dim=1)
    xp = h * (1 + a) + b
    z = F.layer_norm(xp.permute(0, 2, 3, 1), (C,), None, None, M.EPS).reshape(B, -1, C)
    outs, grads = [], []
    if dxp is not None:
        outs.append(xp)
        grads.append(dxp)
    if dz is not None:
        outs.append(z)
        grads.append(dz)
    torch.autograd.backward(outs, grads)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(B, -1, C)
    return rows(xp.detach()), z.detach(), rows(xx.grad), None if rr is None else rows(rr.grad), aa.grad


def _compare(x, ab, res, dxp, dz):
    B, C = x.shape[:2]
    rows = lambda t: None if t is None else t.permute(0, 2, 3, 1).reshape(B, -1, C)
    ref = reference_chain(x, ab, res, dxp, dz)
    xp, z, rstd = M.forward(rows(x), ab, rows(res))
    dx, dab = M.backward(rows(x), ab, rows(res), rows(dxp), dz)
    for name, a, b in zip(("xp", "z", "dx", "dres", "dab"), (xp, z, dx, dx, dab), ref):
        if b is None:
            continue
        assert torch.isfinite(a).all() and torch.isfinite(b).all(), name
        torch.testing.assert_close(a, b, rtol=1e-12, atol=1e-12, msg=lambda m: "%s: %s" % (name, m))
    return xp, z, rstd, dx, dab


@pytest.mark.parametrize("arriving", [("dxp", "dz"), ("dxp",), ("dz",)], ids="+".join)
@pytest.mark.parametrize("with_res", [True, False], ids=["res", "no-res"])
@pytest.mark.parametrize("shape", [(1, 1, 1, 4), (2, 1, 5, 8), (2, 3, 2, 24), (3, 5, 13, 136)], ids=lambda s: "x".join(map(str, s)))
def test_model_equals_fp64_autograd_of_the_plain_formulation(shape, with_res, arriving):
    d = _inputs(*shape)
    _compare(d["x"], d["ab"], d["res"] if with_res else None, d["dxp"] if "dxp" in arriving else None, d["dz"] if "dz" in arriving else None)


def test_model_with_a_equal_to_minus_one():
    """1 + a = 0 on some channels: dx is 0 there, and da is an ordinary sum -- the model never divides by 1 + a"""
    d = _inputs(2, 3, 2, 24)
    d["ab"][:, 3:9] = -1.0
    _, _, _, dx, dab = _compare(d["x"], d["ab"], d["res"], d["dxp"], d["dz"])
    assert torch.all(dx[..., 3:9] == 0) and torch.all(dab[:, 3:9] != 0)


def test_model_on_a_constant_row():
    """x = residual = 0 and one b for every channel: x' is constant over C, the variance 0, z = 0 exactly and the gradients finite (rstd = 1000)"""
    d = _inputs(2, 3, 4, 8)
    d["x"].zero_()
    d["res"].zero_()
    d["ab"][:, 8:] = 0.5
    _, z, rstd, _, _ = _compare(d["x"], d["ab"], d["res"], d["dxp"], d["dz"])
    assert torch.all(z == 0) and torch.allclose(rstd, torch.full_like(rstd, 1000.0))


def test_argument_validation_without_gpu(built_lib):
    """every refusal comes from the host checks, before any device work: the pointers below are never dereferenced"""
    lib = built_lib
    p = ctypes.c_void_p(4096)  # stands for any non-NULL, 16-byte aligned device pointer
    off = ctypes.c_void_p(4100)
    B, P, C = 4, 64, 256
    big = 1 << 40

    def fwd(B=B, P=P, C=C, x=p, res=None, ab=p, xp=p, z=p, rstd=p, eps=1e-6):
        return lib.paella_mod_ln_train_forward(x, res, ab, B, P, C, eps, xp, z, rstd, None, 0, None)

    def bwd(B=B, P=P, C=C, x=p, res=None, ab=p, z=p, rstd=p, dxp=p, dz=p, dx=p, dab=p, ws=p, ws_bytes=big):
        return lib.paella_mod_ln_train_backward(x, res, ab, z, rstd, dxp, dz, B, P, C, dx, dab, ws, ws_bytes, None)

    for call in (fwd, bwd):
        for bad in (dict(C=0), dict(C=6), dict(C=8196), dict(C=-4), dict(P=0), dict(P=(1 << 20) + 1), dict(B=0), dict(B=-1), dict(B=65536), dict(B=1 << 12, P=1 << 19),
                    dict(x=None), dict(ab=None), dict(x=off), dict(res=off), dict(ab=off), dict(z=off), dict(rstd=off)):
            assert call(**bad) == ERR_ARG, (call.__name__, bad)
            assert lib.paella_last_error()
    assert fwd(xp=None) == ERR_ARG and b"required" in lib.paella_last_error()
    assert fwd(xp=off) == ERR_ARG
    assert fwd(z=None) == ERR_ARG and b"go together" in lib.paella_last_error()
    assert fwd(rstd=None) == ERR_ARG and b"go together" in lib.paella_last_error()
    for eps in (0.0, -1.0, float("nan"), float("inf")):
        assert fwd(eps=eps) == ERR_ARG and b"eps" in lib.paella_last_error(), eps
    assert bwd(dxp=None, dz=None) == ERR_ARG and b"at least one" in lib.paella_last_error()
    assert bwd(z=None) == ERR_ARG and b"dz needs" in lib.paella_last_error()
    assert bwd(rstd=None) == ERR_ARG and b"dz needs" in lib.paella_last_error()
    for bad in (dict(dxp=off), dict(dz=off), dict(dx=off), dict(dab=off), dict(ws=off)):
        assert bwd(**bad) == ERR_ARG, bad
    # the workspace: the backward through the LayerNorm keeps g (one activation tensor), P = 64 is four strips of partials; without dz the partials alone
    size = lib.paella_mod_ln_train_workspace_bytes
    need_ln, need_plain = size(B, P, C, 1), size(B, P, C, 0)
    assert need_ln == B * P * C * 4 + B * 4 * 2 * C * 4 and need_plain == B * 4 * 2 * C * 4
    assert bwd(ws_bytes=need_ln - 1) == ERR_WORKSPACE and b"workspace" in lib.paella_last_error()
    assert bwd(ws=None) == ERR_WORKSPACE
    assert bwd(dz=None, ws_bytes=need_plain - 1) == ERR_WORKSPACE and bwd(dz=None, ws=None) == ERR_WORKSPACE
    # what passes the checks and asks for no output launches nothing
    assert bwd(dx=None, dab=None, ws_bytes=need_ln) == 0
    assert bwd(dz=None, z=None, rstd=None, dx=None, dab=None, ws_bytes=need_plain) == 0
    # a sample of one strip without dz needs no workspace at all
    assert bwd(P=16, dz=None, dx=None, dab=None, ws=None, ws_bytes=0) == 0


def test_workspace_bytes(built_lib):
    size = built_lib.paella_mod_ln_train_workspace_bytes
    for B, P, C in [(1, 1, 0), (1, 1, 6), (1, 1, 8196), (0, 4, 64), (2, 0, 64), (-1, 4, 64), (training.MOD_MAX_B + 1, 1, 4), (1, training.MOD_MAX_P + 1, 4),
                    (1, 1, training.MOD_MAX_C + 4), (1 << 12, 1 << 19, 64)]:
        assert size(B, P, C, 0) == 0 and size(B, P, C, 1) == 0, (B, P, C)
    assert training.MOD_MAX_POSITIONS == 2 ** 31 - 1 and (training.MOD_MAX_B, training.MOD_MAX_P, training.MOD_MAX_C) == (65535, 1 << 20, 8192)
    r256 = lambda n: (n + 255) // 256 * 256
    # the documented layout: g [B, P, C] with the LayerNorm, then B x strips x 2C floats when P exceeds one strip of max(16, ceil(P / 1024)) positions
    for B, P, C in [(16, 1024, 320), (16, 256, 640), (16, 64, 1280), (3, 65, 136), (2, 35, 12), (1, 16, 8), (2, 17, 8), (1, 1, 4), (1, 1 << 20, 8192), (65535, 1, 4),
                    (65535, 32767, 8)]:
        rows = max(16, -(-P // 1024))
        strips = -(-P // rows)
        part = r256(B * strips * 2 * C * 4) if strips > 1 else 0
        assert size(B, P, C, 0) == max(part, 256), (B, P, C)
        assert size(B, P, C, 1) == r256(B * P * C * 4) + part, (B, P, C)
        assert part <= B * P * C * 4 // 4 + 256     # the partials stay under a quarter of one activation tensor


def test_timestep_modulate_refuses_what_the_op_cannot_do():
    d = _inputs(2, 3, 4, 8)
    x, res, ab = d["x"].float(), d["res"].float(), d["ab"].float()
    with pytest.raises(ValueError, match="HIP device"):     # cpu tensors: there is no torch fallback
        training.timestep_modulate(x, ab, res, True)
    with pytest.raises(ValueError, match="HIP device"):
        training.timestep_modulate(x, ab)
    for bad in ((x.double(), ab, res), (x, ab.half(), res), (x, ab, res.double()), (x.long(), ab, None)):
        with pytest.raises(ValueError, match="fp32"):
            training.timestep_modulate(*bad)
    with pytest.raises(ValueError, match="tensors"):
        training.timestep_modulate(x, None)
    with pytest.raises(ValueError, match="tensors"):
        training.timestep_modulate(x, ab, 1.0)
    with pytest.raises(ValueError, match=r"\[B, C, H, W\]"):
        training.timestep_modulate(x[0], ab)
    with pytest.raises(ValueError, match="shape of x"):
        training.timestep_modulate(x, ab, res[:, :4])
    with pytest.raises(ValueError, match="shape of x"):
        training.timestep_modulate(x, ab, res[:1])
    for bad_ab in (ab[:, :8], ab[:1], ab[0], ab[:, :, None, None], torch.zeros(2, 24)):
        with pytest.raises(ValueError, match=r"\[B, 2C\]"):
            training.timestep_modulate(x, bad_ab, res)
    with pytest.raises(ValueError, match="multiple of 4"):
        training.timestep_modulate(torch.zeros(1, 6, 2, 2), torch.zeros(1, 12))
    with pytest.raises(ValueError, match="multiple of 4"):
        training.timestep_modulate(torch.zeros(1, 8196, 1, 1), torch.zeros(1, 16392))
    with pytest.raises(ValueError, match="positions"):
        training.timestep_modulate(torch.zeros(0, 8, 2, 2), torch.zeros(0, 16))
    with pytest.raises(ValueError, match="positions"):
        training.timestep_modulate(torch.zeros(1, 8, 0, 2), torch.zeros(1, 16))
    for eps in (0.0, -1e-6, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="eps"):
            training.timestep_modulate(x, ab, res, True, eps)


def test_set_training_modulation():
    """(what every switch's setter does: tests/test_training.py::test_training_switch)"""
    names = set(dir(paella_amd))
    m = paella_amd.Paella(**G.UNET_TINY)
    # a freshly built model's plan is all-off, in train mode on a cuda device too
    m.train()
    assert not any(training._plan(m, True)[:len(training.TRAIN_SWITCHES)]) and training._plan(m, True).training
    assert training._plan(m.set_training_modulation("hip"), True).mod and not training._plan(m, False).mod
    assert set(training.MOD_COUNTERS) == {"calls", "residual", "layernorm", "copied"}
    # nothing new at the package root beyond the method
    assert set(dir(paella_amd)) == names and not [n for n in dir(paella_amd) if "timestep_modulate" in n or n.startswith("MOD")]


@pytest.mark.parametrize("others", list(itertools.product(("torch", "hip"), repeat=3)), ids="-".join)
def test_the_switch_leaves_a_cpu_train_step_alone(others):
    calls = training.MOD_COUNTERS["calls"]
    T.assert_switch_leaves_a_cpu_train_step_alone(lambda m: m.set_training_modulation("hip"),
                                                  before=lambda m: m.set_training_activation(others[0]).set_training_depthwise(others[1]).set_training_attention(others[2]))
    assert training.MOD_COUNTERS["calls"] == calls
