"""GPU: the training MLP activation (paella_amd/csrc/grn_act.hip) against the fp64 model of tests/grn_act_model.py.

The yardstick of every accuracy check is MEASURED in the same test, as tests/test_gpu_head_loss.py does: the torch fp32 chain of `training._channelwise` (F.gelu ->
torch.norm -> mean -> divide -> gamma * (h * nx) + beta + h -> times the SAME dropout mask) runs on the same device and inputs, its max abs error against the fp64 model
is taken for each of z, du, dgamma and dbeta, and the fused op must stay within 4x max(that error, one fp32 ulp at the largest reference magnitude) -- the ulp floor is
the rounding no fp32 result can avoid.  The measured pairs are kept in profiles/train_activation_parity.txt."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from paella_amd import _lib, training
from tests import grn_act_model as M
from tests import train_op_checks as T
from tests.test_gpu_training import _train_step

pytestmark = pytest.mark.gpu
DEV = "cuda"
# one row; strip tails; C off the 64- and 256-channel grain; more than one channel block; the real level-2 width; one row of a whole channel block (a level of one
# position per sample at B = 1, where du IS the MLP's bias gradient: tests/test_gpu_unet_geometries.py, no_timestep)
SHAPES = [(1, 1, 4), (2, 7, 20), (3, 65, 132), (2, 256, 128), (1, 300, 1028), (4, 16, 5120), (1, 1, 256)]
FACTOR = T.FACTOR
_err, _ulp = T.err, T.ulp
SEED = (0xC0FFEE << 40) + 977   # high key word in use
ids = lambda s: "x".join(map(str, s))


@functools.lru_cache(maxsize=None)
def _inputs(B, P, C):
    gen = torch.Generator().manual_seed(100000 * B + 100 * P + C)
    u = (torch.randn(B, P, C, generator=gen) * 1.5).to(DEV)
    gamma = (torch.randn(C, generator=gen) * 0.5).to(DEV)
    beta = (torch.randn(C, generator=gen) * 0.5).to(DEV)
    dz = torch.randn(B, P, C, generator=gen).to(DEV)
    return u, gamma, beta, dz


@functools.lru_cache(maxsize=None)
def _keep(shape, p, seed=SEED):
    return torch.from_numpy(M.keep_mask(shape, p, seed)).to(DEV) if p else None


@functools.lru_cache(maxsize=None)
def _model(shape, p):
    u, gamma, beta, dz = _inputs(*shape)
    z, gx = M.forward(u, gamma, beta, _keep(shape, p), p)
    return (z, gx) + M.backward(u, gamma, dz, _keep(shape, p), p)


def fused(u, gamma, beta, p=0.0, seed=0, dz=None, want_du=True, want_dgamma=True, want_dbeta=True, poison=True):
    """the raw op: forward, and backward when dz is given -> dict of outputs.  Outputs and workspace start as NaN: they are WRITTEN, and the workspace needs no set-up."""
    lib = _lib.load()
    B, P, C = u.shape
    new = (lambda *s: torch.full(s, float("nan"), device=DEV)) if poison else (lambda *s: torch.empty(s, device=DEV))
    ws = torch.full((lib.paella_grn_act_workspace_bytes(B, P, C),), 255, dtype=torch.uint8, device=DEV) if poison else \
        torch.empty(lib.paella_grn_act_workspace_bytes(B, P, C), dtype=torch.uint8, device=DEV)
    out = dict(z=new(B, P, C), gx=new(B, C))
    _lib.check(lib.paella_grn_act_forward(_lib.ptr(u), _lib.ptr(gamma), _lib.ptr(beta), B, P, C, p, seed, _lib.ptr(out["z"]), _lib.ptr(out["gx"]), _lib.ptr(ws), ws.numel(),
                                          _lib.stream_ptr(u.device)))
    if dz is not None:
        out["du"] = new(B, P, C) if want_du else None
        out["dgamma"] = new(C) if want_dgamma else None
        out["dbeta"] = new(C) if want_dbeta else None
        _lib.check(lib.paella_grn_act_backward(_lib.ptr(u), _lib.ptr(gamma), _lib.ptr(out["gx"]), _lib.ptr(dz), B, P, C, p, seed, _lib.ptr(out["du"]), _lib.ptr(out["dgamma"]),
                                               _lib.ptr(out["dbeta"]), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(u.device)))
    return out


def torch_chain(u, gamma, beta, dz, keep, p):
    """the stretch of training._channelwise between the two Linears as torch runs it in fp32, dropout as a multiplication by the given mask -> (z, du, dgamma, dbeta)"""
    B, P, C = u.shape
    uu = u.clone().view(B, P, 1, C).requires_grad_(True)
    g4 = gamma.clone().view(1, 1, 1, C).requires_grad_(True)
    b4 = beta.clone().view(1, 1, 1, C).requires_grad_(True)
    h = F.gelu(uu)
    gx = torch.norm(h, p=2, dim=(1, 2), keepdim=True)
    nx = gx / (gx.mean(dim=-1, keepdim=True) + 1e-6)
    z = g4 * (h * nx) + b4 + h
    if keep is not None:
        z = z * (keep.view(B, P, 1, C).float() * np.float32(M.scale_of(p)))
    z.backward(dz.view(B, P, 1, C))
    return z.detach().view(B, P, C), uu.grad.view(B, P, C), g4.grad.view(C), b4.grad.view(C)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_accuracy_against_the_fp64_model(built_lib, shape, p):
    """Measured pairs (fused / torch, MI355X; all of them in profiles/train_activation_parity.txt)."""
    u, gamma, beta, dz = _inputs(*shape)
    z64, gx64, du64, dgamma64, dbeta64 = _model(shape, p)
    out = fused(u, gamma, beta, p, SEED, dz)
    ref = torch_chain(u, gamma, beta, dz, _keep(shape, p), p)
    pairs = []
    for name, a, b, m in zip(("z", "du", "dgamma", "dbeta"), (out["z"], out["du"], out["dgamma"], out["dbeta"]), ref, (z64, du64, dgamma64, dbeta64)):
        assert torch.isfinite(a).all(), "%s: not finite" % name
        pairs.append((name, _err(a, m), _err(b, m), _ulp(m)))
    print("train_activation parity %s p=%g: " % (shape, p) + "  ".join("%s fused %.3e torch %.3e ulp %.3e" % q for q in pairs))
    # G sums P squares of a GELU whose documented error is 5.5e-7 per value (gemm_device.h: gelu_erf): |dG| <= sqrt(P) 5.5e-7, plus the fp32 rounding of G itself
    torch.testing.assert_close(out["gx"].double(), gx64, rtol=2e-6, atol=5.5e-7 * shape[1] ** 0.5)
    for name, e_fused, e_torch, ulp in pairs:
        assert T.within_yardstick(e_fused, e_torch, ulp), "%s p=%g %s: fused error %.3e exceeds %gx max(torch fp32 chain %.3e, ulp %.3e)" % (shape, p, name, e_fused, FACTOR, e_torch, ulp)


@pytest.mark.parametrize("shape", [(3, 65, 132), (1, 300, 1028), (4, 16, 5120)], ids=ids)
def test_dropout_mask_is_the_cpu_philox_models(built_lib, shape):
    u, gamma, beta, dz = _inputs(*shape)
    p = 0.1
    keep = _keep(shape, p)
    z64, _, du64, _, _ = _model(shape, p)
    out = fused(u, gamma, beta, p, SEED, dz)
    assert 0.05 < 1.0 - float(keep.float().mean()) < 0.15
    # z == 0 exactly at dropped elements, and the kept set is the model's: a kept element is non-zero wherever the model's value is not itself tiny
    # (du is NOT zero there: a dropped element still feeds the norm, dh = dy (1 + gamma n) + (dG / G) h keeps its second term)
    assert torch.all(out["z"][~keep] == 0)
    torch.testing.assert_close(out["du"][~keep].double(), du64[~keep], rtol=1e-4, atol=1e-5)
    solid = keep & (z64.abs() > 1e-4)
    assert int(solid.sum()) > 0.85 * z64.numel()
    assert torch.all(out["z"][solid] != 0)
    assert torch.equal((out["z"] != 0) & (z64.abs() > 1e-4), solid)
    # two seeds differ, and differ as the model says
    other = fused(u, gamma, beta, p, SEED + 1)
    assert not torch.equal(other["z"] == 0, out["z"] == 0)
    keep2 = _keep(shape, p, SEED + 1)
    assert torch.all(other["z"][~keep2] == 0) and torch.all(other["z"][keep2 & (z64.abs() > 1e-4) & keep] != 0)
    # without dropout the seed is without meaning, and the call that never mentions dropout gives the same bits
    a = fused(u, gamma, beta, 0.0, SEED, dz)
    b = fused(u, gamma, beta, 0.0, 0, dz)
    for k in ("z", "gx", "du", "dgamma", "dbeta"):
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(training.gelu_grn_dropout(u, gamma, beta), a["z"])
    assert torch.equal(training.gelu_grn_dropout(u, gamma, beta, p=0.0, seed=SEED), a["z"])
    assert torch.equal(training.gelu_grn_dropout(u, gamma, beta, p=p, seed=SEED), out["z"])


def test_dead_channel(built_lib):
    shape = (3, 65, 132)
    u, gamma, beta, dz = _inputs(*shape)
    u = u.clone()
    u[1, :, 7] = 0.0
    for p in (0.0, 0.1):
        keep = _keep(shape, p)
        out = fused(u, gamma, beta, p, SEED, dz)
        du64, dgamma64, dbeta64 = M.backward(u, gamma, dz, keep, p)
        z64, gx64 = M.forward(u, gamma, beta, keep, p)
        assert float(out["gx"][1, 7]) == 0.0 and float(gx64[1, 7]) == 0.0
        for k in ("z", "gx", "du", "dgamma", "dbeta"):
            assert torch.isfinite(out[k]).all(), k
        torch.testing.assert_close(out["du"][1, :, 7].double(), du64[1, :, 7], rtol=1e-6, atol=1e-7)
        torch.testing.assert_close(out["z"][1, :, 7].double(), z64[1, :, 7], rtol=1e-6, atol=1e-7)
        torch.testing.assert_close(out["du"].double(), du64, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("shape", [(3, 65, 132), (1, 300, 1028), (4, 16, 5120)], ids=ids)
def test_null_outputs_and_determinism(built_lib, shape, p):
    u, gamma, beta, dz = _inputs(*shape)
    full = fused(u, gamma, beta, p, SEED, dz)
    again = fused(u, gamma, beta, p, SEED, dz, poison=False)
    for k in ("z", "gx", "du", "dgamma", "dbeta"):
        assert torch.isfinite(full[k]).all(), k   # the NaN the outputs and the workspace were filled with is gone
        assert torch.equal(full[k], again[k]), k
    for want in [(True, False, False), (False, True, False), (False, False, True), (True, True, False), (False, True, True), (True, False, True)]:
        part = fused(u, gamma, beta, p, SEED, dz, *want)
        for k, w in zip(("du", "dgamma", "dbeta"), want):
            if w:
                assert torch.equal(part[k], full[k]), (want, k)
            else:
                assert part[k] is None
    none = fused(u, gamma, beta, p, SEED, dz, False, False, False)
    assert torch.equal(none["z"], full["z"]) and torch.equal(none["gx"], full["gx"])


def test_offsets_past_4_gib(built_lib):
    """B = 1025 samples of 1024 x 1024 fp32: the last sample starts at byte 2^32.  The arithmetic of a sample depends neither on b nor on B: its z and du are the
    bits of a one-sample call on its slice."""
    B, P, C = 1025, 1024, 1024
    gen = torch.Generator(device=DEV).manual_seed(5)
    u = torch.randn(B, P, C, device=DEV, generator=gen)
    dz = torch.randn(B, P, C, device=DEV, generator=gen)
    assert (B - 1) * P * C * 4 >= 2 ** 32
    _, gamma, beta, _ = _inputs(1, 1, C)
    big = fused(u, gamma, beta, 0.0, 0, dz, poison=False)
    one = fused(u[B - 1:], gamma, beta, 0.0, 0, dz[B - 1:])
    try:
        assert torch.isfinite(one["z"]).all() and torch.isfinite(one["du"]).all()
        assert torch.equal(big["z"][B - 1:], one["z"]) and torch.equal(big["du"][B - 1:], one["du"]) and torch.equal(big["gx"][B - 1:], one["gx"])
        # and the one-sample call is right (fp32 chain, loose: the accuracy tests hold the op to the fp64 model)
        rz, rdu, _, _ = torch_chain(u[B - 1:], gamma, beta, dz[B - 1:], None, 0.0)
        torch.testing.assert_close(one["z"], rz, rtol=1e-4, atol=1e-4)
        torch.testing.assert_close(one["du"], rdu, rtol=1e-4, atol=1e-4)
        # sample 0 and the samples around byte 2^31 are finite and differ from the last one
        assert torch.isfinite(big["z"][0]).all() and torch.isfinite(big["du"][511:513]).all() and not torch.equal(big["z"][0], one["z"][0])
    finally:
        del big, one, u, dz
        torch.cuda.empty_cache()


def test_autograd_function_and_saved_state(built_lib):
    B, H, W, C = 2, 5, 13, 132
    u3, gamma, beta, dz3 = _inputs(B, H * W, C)
    p = 0.1
    raw = fused(u3, gamma, beta, p, SEED, dz3)
    u = u3.view(B, H, W, C).clone().requires_grad_(True)
    g4 = gamma.view(1, 1, 1, C).clone().requires_grad_(True)   # the module's parameter shapes
    b4 = beta.view(1, 1, 1, C).clone().requires_grad_(True)
    packed = []

    def pack(t):
        packed.append(t.numel() * t.element_size())
        return t

    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        z = training.gelu_grn_dropout(u, g4, b4, p, seed=SEED)
    assert z.shape == (B, H, W, C) and z.requires_grad
    assert sum(packed) <= u.numel() * 4 + C * 4 + 4 * B * C, packed
    z.backward(dz3.view(B, H, W, C))
    assert torch.equal(z.detach().view(B, H * W, C), raw["z"])
    assert torch.equal(u.grad.view(B, H * W, C), raw["du"]) and torch.equal(g4.grad.view(C), raw["dgamma"]) and torch.equal(b4.grad.view(C), raw["dbeta"])
    # once differentiable: the gradient comes back without a graph of its own, so a second differentiation cannot silently use a wrong one
    uu = u3.clone().requires_grad_(True)
    (gz,) = torch.autograd.grad(training.gelu_grn_dropout(uu, gamma, beta).sum(), uu, create_graph=True)
    assert not gz.requires_grad
    # frozen parameters: no gradient for them, the same du bits
    uz = u3.clone().requires_grad_(True)
    training.gelu_grn_dropout(uz, gamma, beta, p, seed=SEED).backward(dz3)
    assert gamma.grad is None and beta.grad is None and torch.equal(uz.grad, raw["du"])
    # a view whose rows are not contiguous is copied, not misread; seed=None draws from torch's default CPU generator
    wide = torch.randn(B, H * W, 2 * C, device=DEV)
    assert torch.equal(training.gelu_grn_dropout(wide[..., :C], gamma, beta), training.gelu_grn_dropout(wide[..., :C].contiguous(), gamma, beta))
    torch.manual_seed(3)
    a = training.gelu_grn_dropout(u3, gamma, beta, p)
    c = training.gelu_grn_dropout(u3, gamma, beta, p)
    torch.manual_seed(3)
    b = training.gelu_grn_dropout(u3, gamma, beta, p)
    assert torch.equal(a, b) and not torch.equal(a == 0, c == 0)
    with pytest.raises(ValueError, match="multiple of 4"):
        training.gelu_grn_dropout(torch.zeros(2, 3, 6, device=DEV), torch.zeros(6, device=DEV), torch.zeros(6, device=DEV))


def test_train_step_with_hip_activation_reproduces_the_reference(golden, built_lib):
    """_train_step of tests/test_gpu_training.py under set_training_activation("hip"), against the reference's recorded step and under that test's tolerances; then
    the hand-over to the HIP engine, which never sees the switch"""
    cfg, m = T.model_for("tiny", golden, DEV)
    m.set_training_activation("hip")
    calls = []
    real = training.gelu_grn_dropout
    training.gelu_grn_dropout = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        pred, loss = _train_step(m, cfg)
    finally:
        training.gelu_grn_dropout = real
    assert len(calls) == sum(1 for lv in list(m.down_blocks) + list(m.up_blocks) for b in lv if b.kind in "CF"), "the train-mode forward did not route through the HIP op"
    T.assert_switched_step_and_handover(m, cfg, golden("train_tiny_step"), pred, loss, lambda: m.set_training_activation("torch"))


def test_train_step_with_dropout_is_reproducible_under_manual_seed(golden, built_lib):
    """Two steps after the same torch.manual_seed: the same loss and the same gradients, bit for bit -- the op's masks come from seeds drawn from torch's default CPU
    generator and everything it computes has a fixed order.  torch's OWN backward kernels do not by default: under EITHER setting, with or without dropout, 135 of
    the 136 gradients of this step move by 1e-9 ... 1e-8 between two runs on MI355X, and under torch.use_deterministic_algorithms they repeat exactly (measured for
    both settings).  So the rest of the step runs under that switch here, and what the comparison then holds to account is the op."""
    cfg, m = T.model_for("tiny", golden, DEV)
    m.set_training_activation("hip")
    runs = []
    was, was_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        for seed in (11, 11, 12):
            torch.manual_seed(seed)
            _, loss = _train_step(m, cfg, p_drop=0.1)
            runs.append((loss.clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}))
    finally:
        torch.use_deterministic_algorithms(was, warn_only=was_warn)
    assert torch.isfinite(runs[0][0]) and torch.equal(runs[0][0], runs[1][0])
    assert runs[0][1].keys() == runs[1][1].keys() and len(runs[0][1]) > 10
    for k, v in runs[0][1].items():
        assert torch.equal(v, runs[1][1][k]), k
    assert not torch.equal(runs[0][0], runs[2][0])   # another seed, other masks
