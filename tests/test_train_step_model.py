"""CPU: the mirror of one training step with dropout (tests/train_step_model.py) against the REFERENCE's recorded steps (tests/golden/train_*_step.npz), so that
the place, the order and the scale of its dropout hooks are pinned by the reference itself and not by the HIP route it later judges
(tests/test_gpu_train_step_dropout.py); the order of the hook calls, which is the order in which the HIP route must draw its seeds; and how `model_masks` spends
seeds."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import golden_configs as G
from oracle import paella_oracle as O
from paella_amd import synth
from tests import train_step_model as S

CFGS = {"tiny": G.UNET_TINY, "variant": G.UNET_VARIANT}
# (kind, tensor shape, level) of every dropout the recorded step reaches at B = 2, 16 x 16 tokens, in forward order: "act" [B, H, W, 4c] after the GRN of a ResBlock /
# FeedForwardBlock MLP, "attn" [B, nhead, P, L] on the probabilities of an AttnBlock
_A0, _A1, _A2, _T1, _T2 = ("act", (2, 8, 8, 128), 0), ("act", (2, 4, 4, 256), 1), ("act", (2, 2, 2, 256), 2), ("attn", (2, 4, 16, 29), 1), ("attn", (2, 4, 4, 17), 2)
_V0, _V1, _VT = ("act", (2, 16, 16, 128), 0), ("act", (2, 8, 8, 256), 1), ("attn", (2, 2, 64, 9), 1)
PLAN = {"tiny": [_A0, _A1, _T1, _A1, _T1, _A2, _T2, _A2, _T2, _A1, _T1, _A1, _T1, _A0],
        "variant": [_V0, _V0, _VT, _V1, _VT, _V1, _VT, _V1, _VT, _V1, _V0, _V0]}


def state_dict_for(cfg, golden_npz=None):
    """the seeded synthetic weights of the recorded steps (tests/helpers.weights_for without a module): shapes from the fixture's key list"""
    import paella_amd
    m = paella_amd.Paella(**cfg)
    sd = synth.synth_state_dict(m.state_dict(), seed=G.WEIGHT_SEED, n_blocks=sum(cfg["blocks"]))
    if golden_npz is not None:
        np.testing.assert_allclose(np.array(synth.checksum(sd)), golden_npz["checksum"], rtol=1e-9)
    return sd, [k for k, _ in m.named_parameters()]


@pytest.fixture(scope="module")
def weights(golden):
    return {which: state_dict_for(cfg, golden("unet_%s_forward" % which)) for which, cfg in CFGS.items()}


def test_inputs_reproduce_the_recorded_steps_recipe():
    a, b = S.inputs(G.UNET_TINY), G.train_step_inputs(G.UNET_TINY)
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x, y)
    assert a[4].keys() == b[4].keys() and all(torch.equal(a[4][k], b[4][k]) for k in a[4])
    lat, t, mask, rx, c = S.inputs(G.UNET_VARIANT, 3, 4, 12, seed=5)
    assert lat.shape == mask.shape == rx.shape == (3, 4, 12) and t.shape == (3,) and c["byt5"].shape[:2] == (3, 5)


@pytest.mark.parametrize("tag", ["nodrop", "drop"])
@pytest.mark.parametrize("which", ["tiny", "variant"])
def test_mirror_matches_the_references_recorded_step(golden, weights, which, tag):
    """fp32, the hooks as F.dropout(0.1) under the record's torch seed (or no hooks): the tolerances tests/test_training.py holds paella_amd's own torch route to"""
    g = golden("train_%s_step" % which)
    cfg = CFGS[which]
    sd, names = weights[which]
    drop = None
    if tag == "drop":
        drop = lambda kind, t: F.dropout(t, 0.1, True)
        torch.manual_seed(1234)
    pred, _, loss, grads = S.step(sd, cfg, S.inputs(cfg), drop, torch.float32)
    np.testing.assert_allclose(float(loss), float(g[tag + "_loss"]), rtol=1e-5)
    np.testing.assert_allclose(pred[:, ::4, ::2, ::2].numpy(), g[tag + "_pred_sub"], atol=2e-5, rtol=1e-5)
    assert g["names"].tolist() == names and set(names) == set(grads)
    norms = np.array([float(grads[k].norm()) for k in names])
    sums = np.array([float(grads[k].double().sum()) for k in names])
    np.testing.assert_allclose(norms, g[tag + "_grad_norms"], rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(sums, g[tag + "_grad_sums"], rtol=1e-3, atol=1e-4 * float(np.abs(g[tag + "_grad_norms"]).max()))
    full = [k for k in g.files if k.startswith(tag + "_grad:")]
    assert len(full) >= 8
    for k in full:
        ref = g[k]
        np.testing.assert_allclose(grads[k.split(":", 1)[1]].numpy(), ref, rtol=1e-4, atol=1e-4 * max(float(np.abs(ref).max()), 1e-6), err_msg=k)


@pytest.mark.parametrize("which", ["tiny", "variant"])
def test_hook_call_plan(weights, which):
    """the sequence of dropout calls of the recorded geometry: the order in which the HIP route has to draw its seeds"""
    cfg = CFGS[which]
    drop = S.model_masks(range(100, 200), [0.1] * len(cfg["c_hidden"]), cfg, (16, 16))
    S.step(weights[which][0], cfg, S.inputs(cfg), drop, torch.float32)
    assert [c[:3] for c in drop.calls] == PLAN[which]
    assert [c[4] for c in drop.calls] == list(range(100, 100 + len(PLAN[which])))


def test_model_masks_spend_one_seed_per_call_with_dropout_and_none_without(weights):
    cfg = G.UNET_TINY
    p = [0.0, 0.1, 0.2]
    drop = S.model_masks(range(7, 100), p, cfg, (16, 16))
    kept = {}
    seen = {}

    def watch(kind, t):
        out = drop(kind, torch.ones_like(t))    # a tensor of ones shows the mask: 0 where dropped, the scale where kept
        kind_, shape, level, pc, seed = drop.calls[-1]
        if pc == 0.0:
            assert seed is None and torch.equal(out, torch.ones_like(t))
        else:
            keep = out != 0
            scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(pc)))
            assert torch.all(out[keep] == scale)
            kept.setdefault(pc, []).append(float(keep.double().mean()))
            for other in seen.get(shape, []):
                assert not torch.equal(other, keep), "two calls of one shape under different seeds drew one mask"
            seen.setdefault(shape, []).append(keep)
        return t

    S.step(weights["tiny"][0], cfg, S.inputs(cfg), watch, torch.float32)
    plan = PLAN["tiny"]
    assert [c[:3] for c in drop.calls] == plan and [c[3] for c in drop.calls] == [p[lvl] for _, _, lvl in plan]
    # level 0 consumed nothing: the seeds handed out are consecutive over the calls with p > 0
    assert [c[4] for c in drop.calls if c[3] > 0] == list(range(7, 7 + sum(1 for _, _, lvl in plan if lvl > 0)))
    assert max(len(v) for v in seen.values()) >= 4
    for pc, fracs in kept.items():
        assert all(abs(f - (1 - pc)) < 0.05 for f in fracs), (pc, fracs)


@pytest.mark.parametrize("which", ["tiny", "variant"])
def test_hook_is_neutral_when_absent(weights, which):
    cfg = CFGS[which]
    latents, t, mask, random_x, c = S.inputs(cfg)
    with torch.no_grad():
        a = O.unet_forward(weights[which][0], cfg, latents, t, **c)
        b = O.unet_forward(weights[which][0], cfg, latents, t, drop=None, **c)
        ident = O.unet_forward(weights[which][0], cfg, latents, t, drop=lambda kind, x: x, **c)
    assert torch.equal(a, b) and torch.equal(a, ident)
