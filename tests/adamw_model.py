"""The fp64 model of the training optimizer step (paella_amd.train_ops.ClippedAdamW, paella_amd/csrc/optim.hip): clip_grad_norm_'s norm and coefficient and torch's
single-tensor AdamW arithmetic, written out in exact formulas over float64 tensors.  tests/test_adamw_model.py holds it against torch on the CPU; the GPU tests
measure the fused op and the torch pair against it."""
import math

import torch


def model_norm(grads):
    """the 2-norm over every element of every gradient, as a Python float"""
    return math.sqrt(sum(float((g.double() ** 2).sum()) for g in grads))


def model_coef(norm, max_norm):
    """clip_grad_norm_'s factor with its clamp; max_norm None: no clipping"""
    return 1.0 if max_norm is None else min(1.0, max_norm / (norm + 1e-6))


def model_step(p, g, m, v, step, hyper, coef):
    """one AdamW update of one tensor: p, g, m, v float64 tensors, `step` the count INCLUDING this update (1 at the first), hyper = dict(lr, betas, eps,
    weight_decay), coef the clipping factor of the step -> (p, m, v) new"""
    lr, (b1, b2), eps, wd = hyper["lr"], hyper["betas"], hyper["eps"], hyper["weight_decay"]
    g = g * coef
    p = p * (1.0 - lr * wd)
    m = m + (g - m) * (1.0 - b1)
    v = v * b2 + (1.0 - b2) * g * g
    step_size = lr / (1.0 - b1 ** step)
    p = p - step_size * m / (v.sqrt() / math.sqrt(1.0 - b2 ** step) + eps)
    return p, m, v
