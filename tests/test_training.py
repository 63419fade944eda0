"""CPU: training-mode forward / backward of paella_amd.Paella against ONE TRAINING STEP OF THE REFERENCE
(tests/golden/train_tiny_step.npz, produced by oracle/make_golden.py from /root/reference/src_distributed: add_noise ->
get_loss_weight -> model(...) in train mode -> label-smoothed cross entropy weighted by loss_weight -> backward).
Checked: loss, logits, and the gradient of EVERY parameter (norm and sum to 1e-4, a set of tensors elementwise) -- without dropout
and with the reference's dropout 0.1 under the same torch seed (same mask stream)."""
import numpy as np
import pytest
import torch
from torch import nn

import paella_amd
from oracle import golden_configs as G
from paella_amd import training
from tests.helpers import weights_for


@pytest.fixture(scope="module")
def model(golden):
    m = paella_amd.Paella(**G.UNET_TINY)
    weights_for(m, sum(G.UNET_TINY["blocks"]), golden("unet_tiny_forward"))
    return m


@pytest.fixture(scope="module")
def variant_model(golden):
    """FeedForwardBlock ('F'), cross-attention only (self_attn=False), patch_size 1, two levels (level_config ['CFT', 'TAC'])."""
    m = paella_amd.Paella(**G.UNET_VARIANT)
    weights_for(m, sum(G.UNET_VARIANT["blocks"]), golden("unet_variant_forward"))
    return m


def _step(m, p_drop, seed, cfg=G.UNET_TINY):
    latents, t, mask, random_x, c = G.train_step_inputs(cfg)
    m.train()
    m.dropout = p_drop
    m.zero_grad(set_to_none=True)
    noised = latents * (1 - mask) + random_x * mask          # Paella.add_noise with explicit mask / random_x (src/modules.py:277-283)
    lw = m.get_loss_weight(t, mask)
    if seed is not None:
        torch.manual_seed(seed)
    pred = m(noised, t, **c)
    assert pred.requires_grad and pred.grad_fn is not None
    loss = nn.CrossEntropyLoss(label_smoothing=0.1, reduction='none')(pred, latents)
    loss = ((loss * lw).sum(dim=[1, 2]) / lw.sum(dim=[1, 2])).mean()
    loss.backward()
    return pred.detach(), loss.detach()


@pytest.mark.parametrize("tag,p_drop,seed", [("nodrop", 0.0, None), ("drop", 0.1, 1234)])
@pytest.mark.parametrize("which", ["tiny", "variant"])
def test_training_step_matches_reference(golden, model, variant_model, which, tag, p_drop, seed):
    g = golden("train_%s_step" % which)
    model, cfg = (model, G.UNET_TINY) if which == "tiny" else (variant_model, G.UNET_VARIANT)
    pred, loss = _step(model, p_drop, seed, cfg)
    np.testing.assert_allclose(float(loss), float(g[tag + "_loss"]), rtol=1e-5)
    np.testing.assert_allclose(pred[:, ::4, ::2, ::2].numpy(), g[tag + "_pred_sub"], atol=2e-5, rtol=1e-5)
    params = dict(model.named_parameters())
    names = g["names"].tolist()
    assert names == [k for k, _ in model.named_parameters()], "parameter order / names differ from the reference module"
    norms = np.array([float(params[k].grad.norm()) for k in names])
    sums = np.array([float(params[k].grad.double().sum()) for k in names])
    np.testing.assert_allclose(norms, g[tag + "_grad_norms"], rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(sums, g[tag + "_grad_sums"], rtol=1e-3, atol=1e-4 * float(np.abs(g[tag + "_grad_norms"]).max()))
    full = [k for k in g.files if k.startswith(tag + "_grad:")]
    assert len(full) >= 8
    for k in full:
        ref = g[k]
        got = params[k.split(":", 1)[1]].grad.numpy()
        np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-4 * max(float(np.abs(ref).max()), 1e-6), err_msg=k)
    model.eval()


def test_mode_switch_and_optimizer_step(model):
    """train() / eval() select the path; an optimizer step changes what the next train-mode forward returns; eval mode still
    refuses to run off a HIP device (no CPU fallback for the inference engine)."""
    assert paella_amd.Paella(**G.UNET_TINY).training is False  # constructed in eval mode
    _, l0 = _step(model, 0.0, None)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    nn.utils.clip_grad_norm_(model.parameters(), 1.0)
    opt.step()
    _, l1 = _step(model, 0.0, None)
    assert float(l1) < float(l0)
    model.eval()
    with pytest.raises(RuntimeError, match="HIP device"):
        model(torch.zeros(1, 8, 8, dtype=torch.long), torch.zeros(1), torch.zeros(1, 2, 40))


BAD_MODES = ("HIP", "cuda", "", None, 1, "BF16", "fp16")


@pytest.mark.parametrize("row", training.TRAIN_SWITCHES, ids=lambda s: s.name)
def test_training_switch(row):
    """Every row of `training.TRAIN_SWITCHES` gives one attribute, one `set_training_*` method and one keyword of `set_training_route`: the default, the refusal of
    anything but its two settings (the other rows' settings among them) with the setting left alone, the module returned, the other four switches untouched in
    both directions; then `set_training_route` (all or nothing) and `training_route` (round trip)."""
    others = [s for s in training.TRAIN_SWITCHES if s is not row]
    assert (row.attr, row.setter, row.label) == ("_train_" + row.name, "set_training_" + row.name, "training " + row.name)
    assert row.refusal == "training %s must be '%s' or '%s'" % (row.name, row.off, row.on)
    for start in ("off", "on"):          # the other four all off, then all on
        m = paella_amd.Paella(**G.UNET_TINY)
        assert getattr(m, row.attr) == row.off and m.training_route() == {s.name: s.off for s in training.TRAIN_SWITCHES}
        for s in others:
            getattr(m, s.setter)(getattr(s, start))
        rest = {s.name: getattr(s, start) for s in others}
        for bad in BAD_MODES + tuple(v for s in others for v in (s.off, s.on) if v not in (row.off, row.on)):
            with pytest.raises(ValueError, match=row.refusal):
                getattr(m, row.setter)(bad)
            with pytest.raises(ValueError, match=row.refusal):
                m.set_training_route(**dict({s.name: s.off if start == "on" else s.on for s in others}, **{row.name: bad}))     # a bad value among good ones
            assert m.training_route() == dict(rest, **{row.name: row.off})
        for mode in (row.on, row.off, row.on):
            assert getattr(m, row.setter)(mode) is m and getattr(m, row.attr) == mode
            assert m.training_route() == dict(rest, **{row.name: mode}) and [getattr(m, s.attr) for s in others] == [getattr(s, start) for s in others]
        assert m.set_training_route(**{row.name: row.off}) is m and getattr(m, row.attr) == row.off
        route = m.set_training_route(**{row.name: row.on}).training_route()
        assert list(route) == [s.name for s in training.TRAIN_SWITCHES]
        fresh = paella_amd.Paella(**G.UNET_TINY)
        assert fresh.set_training_route(**route).training_route() == route and fresh.set_training_route().training_route() == route
        del fresh.__dict__[row.attr]        # a module pickled before the switch existed: read as its default
        assert fresh.training_route() == dict(route, **{row.name: row.off}) and training._plan(fresh, True)._asdict()[row.field] is False
    with pytest.raises(TypeError, match="set_training_route takes"):
        m.set_training_route(**{row.name: row.on, "route": "hip"})
