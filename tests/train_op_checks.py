"""What the tests of the training ops (paella_amd/train_ops.py) check the same way: the error figures and the yardstick rule of the accuracy tests, and the
model-level block -- the reference's recorded training step under the tolerances of tests/test_gpu_training.py, `forward_loss` on the same route, and the hand-over
to the HIP engine, which never sees a training switch."""
import numpy as np
import torch
from torch import nn

import paella_amd
from oracle import golden_configs as G
from tests.helpers import cond_for, to_dev, weights_for

FACTOR = 4.0


def err(a, ref):
    """max abs error of a against the fp64 values ref"""
    return float((a.double() - ref).abs().max())


def ulp(ref):
    """one fp32 ulp at the largest magnitude of ref: the rounding no fp32 result can avoid"""
    return float(np.spacing(np.float32(float(ref.abs().max()))))


def within_yardstick(e_fused, e_torch, floor=0.0):
    """the accuracy rule: the fused op's error stays within FACTOR x the error MEASURED for the torch fp32 path on the same inputs, or x `floor` where that is larger"""
    return e_fused <= FACTOR * max(e_torch, floor)


def model_for(which, golden, dev):
    """(cfg, the "tiny" or "variant" network with the weights of the recorded step, on dev)"""
    cfg = G.UNET_TINY if which == "tiny" else G.UNET_VARIANT
    m = paella_amd.Paella(**cfg)
    weights_for(m, sum(cfg["blocks"]), golden("unet_%s_forward" % which))
    return cfg, m.to(dev)


def assert_recorded_step(m, g, loss, pred=None):
    """loss (and the logits, where the step has them) and the gradients m holds after one step without dropout, against the reference's record g"""
    np.testing.assert_allclose(float(loss), float(g["nodrop_loss"]), rtol=2e-5)
    if pred is not None:
        np.testing.assert_allclose(pred[:, ::4, ::2, ::2].cpu().numpy(), g["nodrop_pred_sub"], atol=5e-5, rtol=1e-4)
    params = dict(m.named_parameters())
    names = g["names"].tolist()
    norms = np.array([float(params[k].grad.norm()) for k in names])
    np.testing.assert_allclose(norms, g["nodrop_grad_norms"], rtol=5e-4, atol=1e-6)
    for k in [k for k in g.files if k.startswith("nodrop_grad:")]:
        ref = g[k]
        np.testing.assert_allclose(params[k.split(":", 1)[1]].grad.cpu().numpy(), ref, rtol=5e-4, atol=5e-4 * max(float(np.abs(ref).max()), 1e-6), err_msg=k)


def assert_switched_step_and_handover(m, cfg, g, pred, loss, flip_back, op_calls=None, calls_per_forward=0):
    """After `_train_step` of tests/test_gpu_training.py under a training switch gave (pred, loss): the recorded step; `forward_loss` takes the same route; then an
    optimizer step, back to eval, and the engine's logits are the same bits after flip_back() has put the switch back.  op_calls() reads a call counter of the op:
    forward_loss raises it by calls_per_forward, eval mode never reaches the op."""
    dev = pred.device
    assert_recorded_step(m, g, loss, pred)
    latents, t, mask, random_x, c = G.train_step_inputs(cfg)
    latents, t, mask, random_x = latents.to(dev), t.to(dev), mask.to(dev), random_x.to(dev)
    noised = latents * (1 - mask) + random_x * mask
    lw = m.get_loss_weight(t, mask)
    n0 = op_calls() if op_calls else 0
    fl, _ = m.forward_loss(noised, t, latents, **to_dev(c, dev))
    assert not op_calls or op_calls() == n0 + calls_per_forward
    np.testing.assert_allclose(float(((fl.detach() * lw).sum(dim=[1, 2]) / lw.sum(dim=[1, 2])).mean()), float(g["nodrop_loss"]), rtol=2e-5)
    opt = torch.optim.AdamW(m.parameters(), lr=2e-3)
    nn.utils.clip_grad_norm_(m.parameters(), 1.0)
    opt.step()
    m.eval()
    gen = torch.Generator().manual_seed(17)
    x = torch.randint(0, cfg["num_labels"], (2, 16, 16), generator=gen).to(dev)
    r = torch.tensor([0.8, 0.3]).to(dev)
    cc = to_dev(cond_for(cfg, 2, 3, 1, G.COND_SEED + 3), dev)
    with torch.no_grad():
        n0 = op_calls() if op_calls else 0
        with_hip = m(x, r, **cc).clone()
        flip_back()
        with_torch = m(x, r, **cc)
        assert not op_calls or op_calls() == n0
    assert torch.isfinite(with_hip).all() and torch.equal(with_hip, with_torch)


def assert_switch_leaves_a_cpu_train_step_alone(flip, before=None):
    """the switches act on a cuda device only: on the CPU a train-mode forward is the torch chain before and after flip(m), bit for bit"""
    m = paella_amd.Paella(**G.UNET_TINY)
    weights_for(m, sum(G.UNET_TINY["blocks"]))
    latents, t, mask, random_x, c = G.train_step_inputs(G.UNET_TINY)
    noised = latents * (1 - mask) + random_x * mask
    m.train()
    m.dropout = 0.0
    if before:
        before(m)
    a = m(noised, t, **c)
    flip(m)
    b = m(noised, t, **c)
    assert torch.equal(a, b)
