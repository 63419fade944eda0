"""Training optimizer step without a GPU: the fp64 model the GPU tests measure against equals clip_grad_norm_ + torch.optim.AdamW on the CPU; the chunk plan the
kernels walk; the C entry points validate their arguments on the host before anything is enqueued; the Python surface refuses what the op cannot do instead of
falling back."""
import ctypes
import os

import numpy as np
import pytest
import torch
from torch import nn

from paella_amd import _lib, train_ops, training
from tests import adamw_model as A

ERR_ARG, ERR_WORKSPACE = -1, -3


@pytest.mark.parametrize("max_norm", [1.0, 1e3, None])
def test_model_equals_torch_clip_and_adamw_on_the_cpu(max_norm):
    """3 steps at lr = 1e-2, wd = 0.01 over tensors of 5, 77 and 1000 elements.  This guards the FORMULA: a wrong bias correction or decay moves a weight by the
    order of lr x 0.1 = 1e-3, fp32 rounding of the torch side by ~6e-7 (measured): atol 1e-5.  max_norm 1 clips (the norm is ~33), 1e3 does not."""
    gen = torch.Generator().manual_seed(11)
    hyper = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)
    ps = [nn.Parameter(torch.randn(n, generator=gen)) for n in (5, 77, 1000)]
    opt = torch.optim.AdamW(ps, **hyper)
    p64 = [p.detach().double() for p in ps]
    m64 = [torch.zeros_like(p) for p in p64]
    v64 = [torch.zeros_like(p) for p in p64]
    for step in (1, 2, 3):
        grads = [torch.randn(p.shape, generator=gen) for p in ps]
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        norm = A.model_norm(grads)
        if max_norm is not None:
            got = nn.utils.clip_grad_norm_(ps, max_norm)
            np.testing.assert_allclose(float(got), norm, rtol=1e-6)
        opt.step()
        coef = A.model_coef(norm, max_norm)
        assert (coef < 0.1) if max_norm == 1.0 else (coef == 1.0)
        for i, g in enumerate(grads):
            p64[i], m64[i], v64[i] = A.model_step(p64[i], g.double(), m64[i], v64[i], step, hyper, coef)
            st = opt.state[ps[i]]
            assert float(st["step"]) == step
            for name, got, ref in (("p", ps[i].detach(), p64[i]), ("exp_avg", st["exp_avg"], m64[i]), ("exp_avg_sq", st["exp_avg_sq"], v64[i])):
                e = float((got.double() - ref).abs().max())
                assert e <= 1e-5, "step %d tensor %d %s: max abs error %.3e" % (step, i, name, e)


def test_chunk_plan():
    C = 4096
    begins, total = train_ops.adamw_chunk_plan([0, 1, C - 1, C, C + 1, 2 * C, 0, 2 * C + 3, 0], C)
    assert begins == [0, 0, 1, 2, 3, 5, 7, 7, 10] and total == 10
    assert train_ops.adamw_chunk_plan([], C) == ([], 0)
    assert train_ops.adamw_chunk_plan([0, 0], C) == ([0, 0], 0)
    assert train_ops.adamw_chunk_plan([2 ** 31 + C + 5], C) == ([0], 2 ** 19 + 2)
    with pytest.raises(ValueError):
        train_ops.adamw_chunk_plan([3, -1], C)
    assert training.adamw_chunk_plan is train_ops.adamw_chunk_plan and training.ClippedAdamW is train_ops.ClippedAdamW and training.grad_norm is train_ops.grad_norm


def test_row_layouts_agree(built_lib):
    """the numpy row the optimizer fills is the ctypes row is the header's struct: 88 bytes, the same offsets; the chunk is a multiple of 1024"""
    assert train_ops.ADAMW_ROW.itemsize == ctypes.sizeof(_lib.AdamwTensor) == 88
    for name, _ in _lib.AdamwTensor._fields_:
        assert train_ops.ADAMW_ROW.fields[name][1] == getattr(_lib.AdamwTensor, name).offset, name
    C = built_lib.paella_adamw_chunk_elems()
    assert C > 0 and C % 1024 == 0
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "paella_hip.h")).read()
    assert "#define PAELLA_ADAMW_CHUNK %d " % C in header


def test_entry_points_validate_on_the_host(built_lib):
    lib = built_lib
    assert lib.paella_adamw_workspace_bytes(0, 0) == 256
    assert lib.paella_adamw_workspace_bytes(3, 5) == 3 * 256
    assert lib.paella_adamw_workspace_bytes(17, 33) == 256 + 512 + 512
    assert lib.paella_adamw_workspace_bytes(-1, 0) == 0 and lib.paella_adamw_workspace_bytes(1, -1) == 0
    buf = (ctypes.c_char * 4096)()
    a = ctypes.addressof(buf)
    a += -a % 256
    rows, steps, norm, ws = a, a + 1024, a + 2048, a + 2304      # never dereferenced: every call below fails its checks first
    step, gn = lib.paella_adamw_step, lib.paella_adamw_grad_norm
    assert step(rows, -1, 0, 1.0, steps, norm, ws, 1 << 20, None) == ERR_ARG and b"n_tensors" in lib.paella_last_error()
    assert step(rows, 1, -1, 1.0, steps, norm, ws, 1 << 20, None) == ERR_ARG
    assert step(rows, 0, 1, 1.0, steps, norm, ws, 1 << 20, None) == ERR_ARG          # a chunk without a tensor
    assert step(None, 1, 1, 1.0, steps, norm, ws, 1 << 20, None) == ERR_ARG and b"required" in lib.paella_last_error()
    assert step(rows, 1, 1, 1.0, None, norm, ws, 1 << 20, None) == ERR_ARG
    assert step(rows, 1, 1, 1.0, steps, None, ws, 1 << 20, None) == ERR_ARG
    assert step(rows, 1, 1, float("nan"), steps, norm, ws, 1 << 20, None) == ERR_ARG and b"max_norm" in lib.paella_last_error()
    assert step(rows, 1, 1, 1.0, steps, norm, None, 1 << 20, None) == ERR_WORKSPACE
    assert step(rows, 1, 1, 1.0, steps, norm, ws, 3 * 256 - 1, None) == ERR_WORKSPACE and b"paella_adamw_workspace_bytes" in lib.paella_last_error()
    assert step(rows, 1, 1, 1.0, steps, norm, ws + 4, 1 << 20, None) == ERR_ARG and b"aligned" in lib.paella_last_error()
    assert gn(None, 1, 1, norm, ws, 1 << 20, None) == ERR_ARG
    assert gn(rows, 1, 1, None, ws, 1 << 20, None) == ERR_ARG
    assert gn(rows, 1, 1, norm, ws, 16, None) == ERR_WORKSPACE


def _p(*shape, dtype=torch.float32):
    return nn.Parameter(torch.zeros(*shape, dtype=dtype))


@pytest.mark.parametrize("kwargs", [dict(amsgrad=True), dict(maximize=True), dict(foreach=True), dict(foreach=False), dict(foreach=None), dict(fused=True),
                                    dict(fused=False), dict(capturable=True), dict(differentiable=True)])
def test_refuses_torch_implementation_switches(kwargs):
    with pytest.raises(ValueError, match=next(iter(kwargs))):
        training.ClippedAdamW([_p(3)], **kwargs)


def test_refuses_unknown_keyword():
    with pytest.raises(TypeError, match="nesterov"):
        training.ClippedAdamW([_p(3)], nesterov=True)


@pytest.mark.parametrize("kwargs, name", [(dict(lr=-1e-3), "lr"), (dict(lr=float("nan")), "lr"), (dict(lr=torch.tensor(1e-3)), "lr"), (dict(eps=-1e-8), "eps"),
                                          (dict(betas=(1.0, 0.999)), "betas"), (dict(betas=(-0.1, 0.999)), "betas"), (dict(betas=(0.9, 1.0)), "betas"),
                                          (dict(betas=(0.9,)), "betas"), (dict(weight_decay=-0.01), "weight_decay"), (dict(max_norm=0.0), "max_norm"),
                                          (dict(max_norm=-1.0), "max_norm"), (dict(max_norm=float("inf")), "max_norm"), (dict(max_norm=float("nan")), "max_norm")])
def test_refuses_out_of_range_hyperparameters(kwargs, name):
    with pytest.raises(ValueError, match=name):
        training.ClippedAdamW([_p(3)], **kwargs)


def test_refuses_out_of_range_hyperparameters_of_a_group():
    with pytest.raises(ValueError, match="lr"):
        training.ClippedAdamW([dict(params=[_p(3)], lr=-1.0)])
    with pytest.raises(ValueError, match="amsgrad"):
        training.ClippedAdamW([dict(params=[_p(3)], amsgrad=True)])


def test_refuses_parameters_it_cannot_update():
    with pytest.raises(ValueError, match="fp32 parameters"):
        training.ClippedAdamW([_p(3, dtype=torch.bfloat16)])
    with pytest.raises(ValueError, match="fp32 parameters"):
        training.ClippedAdamW([_p(3), _p(3, dtype=torch.float64)])
    with pytest.raises(ValueError, match="HIP device only"):
        training.ClippedAdamW([_p(3)])                       # a CPU parameter: there is no torch fallback
    with pytest.raises(ValueError, match="takes tensors"):
        training.ClippedAdamW([dict(params=[3.0])])
    with pytest.raises(ValueError):
        training.ClippedAdamW([])                            # torch's own refusal of an empty parameter list


def test_grad_norm_refusals():
    with pytest.raises(ValueError, match="no parameter has a gradient"):
        training.grad_norm([_p(3)])
    p = _p(3)
    p.grad = torch.ones(3)
    with pytest.raises(ValueError, match="HIP device only"):
        training.grad_norm([p])
    with pytest.raises(ValueError, match="takes tensors"):
        training.grad_norm([1.0])
