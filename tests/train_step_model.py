"""fp64 mirror of one training step WITH dropout: the CPU oracle's network (oracle/paella_oracle.unet_forward with its `drop` hook), the reference's loss
(label smoothing 0.1, weighted by get_loss_weight: src_distributed/train.py:104-112) and autograd's gradients, all in a dtype of the caller's choice.  The dropout
masks are whatever the `drop` callback applies: F.dropout under a torch seed reproduces the reference's recorded step (tests/test_train_step_model.py), and
`model_masks` applies the masks of the HIP ops' CPU Philox models (tests/grn_act_model.keep_mask, tests/attn_train_model.keep_mask) under given seeds, which makes this
the reference of the HIP route with dropout on (tests/test_gpu_train_step_dropout.py).  Nothing here imports paella_amd.training."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import golden_configs as G
from oracle import paella_oracle as O
from paella_amd import synth
from tests import attn_train_model as AM
from tests import grn_act_model as GM


def inputs(cfg, B=2, H=16, W=16, seed=21, S_byt5=5, n_img=1):
    """(latents, t, mask, random_x, conditioning) of one training step on a B x H x W token grid with S_byt5 ByT5 rows, a CLIP text entry and n_img CLIP-image
    entries: the recipe of G.train_step_inputs, which the defaults reproduce"""
    g = torch.Generator().manual_seed(seed)
    latents = torch.randint(0, cfg["num_labels"], (B, H, W), generator=g)
    t = (1 - torch.rand(B, generator=g)).add(0.001).clamp(0.001, 1.0)
    mask = (torch.rand(B, H, W, generator=g) <= t[:, None, None]).long()
    random_x = torch.randint(0, cfg["num_labels"], (B, H, W), generator=g)
    c = synth.synth_conditioning(B, S_byt5, cfg["byt5_embd"], cfg["clip_embd"], seed=G.COND_SEED + 9 + (seed - 21), with_clip=True, n_clip_image=n_img)
    return latents, t, mask, random_x, c


def loss_weight(t, mask, min_val=0.3):
    """get_loss_weight (reference src_distributed/modules.py:283-284)"""
    return 1 - (1 - mask) * ((1 - t) * (1 - min_val))[:, None, None]


def step(sd, cfg, inp, drop, dtype=torch.float64):
    """One training step of the network with the weights sd on inp = inputs(...): -> (pred [B, num_labels, H, W], loss_per_position [B, H, W], loss, grads), all
    detached and of `dtype`; grads maps every floating-point key of sd to the gradient of the loss."""
    latents, t, mask, random_x, c = inp
    leaves = {k: v.detach().to(dtype).clone().requires_grad_(True) if v.is_floating_point() else v for k, v in sd.items()}
    noised = latents * (1 - mask) + random_x * mask           # Paella.add_noise with explicit mask / random_x (reference src/modules.py:277-283)
    lw = loss_weight(t.to(dtype), mask)
    # The angle of the timestep embedding starts as the fp32 product r * max_positions (gen_r_embedding, reference src/modules.py:213, on the fp32 r of the training
    # loop): up to 1e4 with an fp32 spacing of 1e-3, and its sine and cosine feed every TimestepBlock.  That rounded product is part of what the network is GIVEN, as
    # the oracle's fp32 frequency table is: a mirror that redid it in fp64 would evaluate another network (the tiny step's logits move by 1.1e-4, as much as the
    # recorded step's logit tolerance allows in all), and every fp32 route would be charged with it.  The same holds for the second product, with the frequency
    # table: every fp32 route (reference, engine, torch) does fl(fl(r * 1e4) * freq) as the same IEEE multiplications and gets the same bits, and redoing it in fp64
    # moves angles of up to 1e4 by up to 5e-4 (6e-5 ... 1.3e-4 in the logits of small networks, against 2e-6 ... 4e-6 of everything else an fp32 evaluation
    # rounds).  So a wider dtype receives the whole embedding as the oracle's own fp32 evaluation; what the sine and cosine of those angles are is checked on its
    # own (tests/test_gpu_unet_geometries.py: test_timestep_embedding).
    r_embed = None if dtype == torch.float32 else O.r_embedding(t.float(), cfg["c_r"])
    pred = O.unet_forward(leaves, cfg, noised, t, dtype=dtype, drop=drop, r_embed=r_embed, **c)
    per_pos = F.cross_entropy(pred, latents, label_smoothing=0.1, reduction="none")
    loss = ((per_pos * lw).sum(dim=[1, 2]) / lw.sum(dim=[1, 2])).mean()
    loss.backward()
    grads = {k: v.grad for k, v in leaves.items() if v.is_floating_point() and v.grad is not None}
    return pred.detach(), per_pos.detach(), loss.detach(), grads


def levels_of(cfg, grid):
    """grid = (H, W) in tokens -> ({(h, w) of a level's feature map: level}, {its number of positions: level})"""
    hw, pos = {}, {}
    for lvl in range(len(cfg["c_hidden"])):
        f = cfg["patch_size"] << lvl
        assert grid[0] % f == 0 and grid[1] % f == 0, "the grid does not divide down to level %d" % lvl
        h, w = grid[0] // f, grid[1] // f
        hw[(h, w)] = pos[h * w] = lvl
    assert len(hw) == len(pos) == len(cfg["c_hidden"]), "two levels of one geometry: the level cannot be read off a tensor"
    return hw, pos


def model_masks(seeds, p_of_level, cfg, grid):
    """The `drop` callback that does what the HIP route does.  The i-th call works the level out of its tensor's geometry and takes p = p_of_level[level]; at
    p = 0 the tensor comes back as it is and no seed is consumed (gelu_grn_dropout / attention_dropout draw nothing there), otherwise it is multiplied by
    keep_mask(shape, p, next(seeds)) * scale_of(p) of the op's CPU model: "act" masks index the flat [B, P, C] element, "attn" masks [B, nhead, P, L].
    drop.calls records (kind, shape, level, p, seed or None) per call."""
    seeds = iter(seeds)
    hw, pos = levels_of(cfg, grid)
    calls = []

    def drop(kind, t):
        if kind == "act":
            B, H, W, C = t.shape
            level, shape, M = hw[(H, W)], (B, H * W, C), GM
        elif kind == "attn":
            level, shape, M = pos[t.size(2)], tuple(t.shape), AM
        else:
            raise ValueError(kind)
        p = float(p_of_level[level])
        if p == 0.0:
            calls.append((kind, tuple(t.shape), level, p, None))
            return t
        seed = int(next(seeds))
        calls.append((kind, tuple(t.shape), level, p, seed))
        keep = torch.from_numpy(np.ascontiguousarray(M.keep_mask(shape, p, seed))).view(t.shape)
        return t * (keep.to(t.dtype) * M.scale_of(p))

    drop.calls = calls
    return drop
