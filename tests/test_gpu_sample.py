"""GPU: closed-loop sampling parity.  With the torch noise replayed explicitly, paella_amd.sample must reproduce the
token grid the REFERENCE's own sample() produced (tests/golden/sample_tiny*.npz); integer outputs are compared exactly
and any position that differs must trace back to a logit near-tie (reported)."""
import numpy as np
import pytest
import torch

import paella_amd
from oracle import golden_configs as G
from oracle import paella_oracle as O
from paella_amd import _lib, sampling
from tests.helpers import assert_token_parity, cond_for, stepwise_token_parity, to_dev, weights_for

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def tiny_sd(golden, built_lib):
    m = paella_amd.Paella(**G.UNET_TINY)
    sd = weights_for(m, sum(G.UNET_TINY["blocks"]), golden("unet_tiny_forward"))
    return m.to(DEV), sd


@pytest.fixture(scope="module")
def tiny(tiny_sd):
    return tiny_sd[0]


def _oracle_fwd(sd, cfg):
    def fwd(tk, rr, **inp):
        with torch.no_grad():
            return O.unet_forward(sd, cfg, tk, rr, **inp)
    return fwd


def _assert_rows_match_up_to_near_ties(m, part, full_rows, start_rows, cond2, uncond2, cfg_scale, eps=2e-3):
    """Argmax step at sizes the oracle cannot reach: rows sampled as a small shard vs the same rows of the full batch.  Different
    GEMM decompositions (M differs) change the fp32 summation order, so a token may differ ONLY where the mixed logits' top-1 /
    top-2 margin is below eps; such positions are counted and printed."""
    mism = part != full_rows
    n_mis = int(mism.sum())
    if n_mis:
        r = torch.ones(start_rows.size(0), device=DEV)
        l = m(start_rows, r, **cond2) * cfg_scale + m(start_rows, r, **uncond2) * (1.0 - cfg_scale)
        top = l.topk(2, dim=1).values
        margin = (top[:, 0] - top[:, 1])
        clear = int((mism & ~(margin < eps)).sum())
        print("shard vs full batch: %d / %d tokens differ, all at top1-top2 margin < %g: %s (max margin among them %.2e)"
              % (n_mis, mism.numel(), eps, clear == 0, float(margin[mism].max()) if n_mis else 0.0))
        assert clear == 0, "%d token(s) differ where the logits were not a near-tie" % clear
    else:
        print("shard vs full batch: all %d tokens identical" % mism.numel())


def _exact_or_counted(toks, ref_tokens, rep, what):
    """Closed loop: identical integers, unless the teacher-forced run already counted near-tie flips (then the trajectories
    may legitimately separate from that step on and the agreement is reported, not asserted)."""
    same = int((toks.cpu().numpy() == ref_tokens).sum())
    print("%s closed loop: %d / %d tokens identical to the reference" % (what, same, ref_tokens.size))
    if rep["near_tie"] == 0:
        assert same == ref_tokens.size, "%s: closed-loop tokens differ although no step had a near-tie flip" % what


def test_sample_reproduces_reference_tokens(golden, tiny_sd):
    """BASELINE config 1: tiny model, 32x32 grid, 8 steps, batch 1, CFG 8 -- reference src/utils.py:35 signature.
    Bit-exact token parity: per step (teacher-forced on the oracle trajectory) every differing token must sit on a
    reference near-tie; with no such flip the closed-loop grid equals the tokens the REFERENCE's own sample() produced."""
    tiny, sd = tiny_sd
    g = golden("sample_tiny")
    cfg = G.UNET_TINY
    c, u = cond_for(cfg, 1, 4, 0, G.COND_SEED), cond_for(cfg, 1, 4, 0, G.COND_SEED + 5)
    cs, us = to_dev(c, DEV), to_dev(u, DEV)
    noise = O.replay_torch_noise(G.SAMPLER_SEED, (1, 32, 32), cfg["num_labels"], 8, 7)
    rep = stepwise_token_parity(tiny, _oracle_fwd(sd, cfg), cfg["num_labels"], c, u, cs, us, noise, 8, 7, (1.0, 0.2), 8.0)
    assert_token_parity(rep, "tiny categorical, 8 steps")
    toks = paella_amd.sample(tiny, cs, (1, 32, 32), unconditional_inputs=us, steps=8, renoise_steps=7, temperature=(1.0, 0.2), cfg=8.0,
                             device=DEV, noise=noise)
    assert toks.dtype == torch.int64 and toks.shape == (1, 32, 32)
    _exact_or_counted(toks, g["tokens"], rep, "categorical sample vs reference")


def test_sample_argmax_trajectory(golden, tiny_sd):
    """T = 0 extension: argmax substituted for multinomial; final grid equals the oracle's closed-loop argmax trajectory."""
    tiny, sd = tiny_sd
    g = golden("sample_tiny")
    cfg = G.UNET_TINY
    c, u = cond_for(cfg, 1, 4, 0, G.COND_SEED), cond_for(cfg, 1, 4, 0, G.COND_SEED + 5)
    cs, us = to_dev(c, DEV), to_dev(u, DEV)
    noise = O.replay_torch_noise(G.SAMPLER_SEED, (1, 32, 32), cfg["num_labels"], 8, 7)
    rep = stepwise_token_parity(tiny, _oracle_fwd(sd, cfg), cfg["num_labels"], c, u, cs, us, noise, 8, 7, (0.0, 0.0), 8.0, argmax=True, eps=1e-4)
    assert_token_parity(rep, "tiny argmax, 8 steps")
    toks = paella_amd.sample(tiny, cs, (1, 32, 32), unconditional_inputs=us, steps=8, renoise_steps=7, temperature=(0.0, 0.0), cfg=8.0,
                             device=DEV, noise=noise)
    _exact_or_counted(toks, g["tokens_argmax"], rep, "argmax sample vs oracle")


def test_sample_distributed_signature(golden, tiny):
    """src_distributed/utils.py:97 variant: init_x, cfg schedule, conditional-step cutoff, different S for the uncond set.
    Closed loop against the REFERENCE's tokens; a difference is accepted only if a per-step rerun from the reference-side state
    classifies it as a near-tie (same policy as above, printed)."""
    g = golden("sample_tiny_distributed")
    cfg = G.UNET_TINY
    cd, ud = to_dev(cond_for(cfg, 2, 5, 1, G.COND_SEED), DEV), to_dev(cond_for(cfg, 2, 2, 0, G.COND_SEED + 5), DEV)
    noise = O.replay_torch_noise(G.SAMPLER_SEED + 1, (2, 16, 16), cfg["num_labels"], 6, 5)
    toks = paella_amd.sample_distributed(tiny, cd, ud, (2, 16, 16), init_x=torch.from_numpy(g["init_x"]).to(DEV), steps=6,
                                         temperature=(0.7, 0.3), cfg=(8.0, 4.0), t_start=0.8, sampling_conditional_steps=4, noise=noise)
    same = int((toks.cpu().numpy() == g["tokens"]).sum())
    print("sample_distributed vs reference: %d / %d tokens identical" % (same, g["tokens"].size))
    assert same == g["tokens"].size, "closed-loop tokens differ from the reference's (run the stepwise check to classify)"


def test_noise_modes_and_seeding(tiny):
    cfg = G.UNET_TINY
    cs, us = to_dev(cond_for(cfg, 2, 3, 0, 1), DEV), to_dev(cond_for(cfg, 2, 3, 0, 2), DEV)
    kw = dict(unconditional_inputs=us, steps=4, renoise_steps=3, device=DEV)
    torch.manual_seed(7)
    a = paella_amd.sample(tiny, cs, (2, 16, 16), **kw)
    torch.manual_seed(7)
    b = paella_amd.sample(tiny, cs, (2, 16, 16), **kw)
    assert torch.equal(a, b) and int(a.min()) >= 0 and int(a.max()) < cfg["num_labels"]
    torch.manual_seed(7)
    p1 = paella_amd.sample(tiny, cs, (2, 16, 16), noise="philox", seed=5, **kw)
    torch.manual_seed(7)
    p2 = paella_amd.sample(tiny, cs, (2, 16, 16), noise="philox", seed=5, **kw)
    torch.manual_seed(7)
    p3 = paella_amd.sample(tiny, cs, (2, 16, 16), noise="philox", seed=6, **kw)
    assert torch.equal(p1, p2) and not torch.equal(p1, p3)
    # no guidance path
    n = paella_amd.sample(tiny, cs, (2, 16, 16), unconditional_inputs=None, cfg=None, steps=2, renoise_steps=1, device=DEV)
    assert n.shape == (2, 16, 16)


def test_batch_shard_equivalence(tiny):
    """Sharded == unsharded: sampling rows [0:2] and [2:4] separately with sliced noise equals the full batch."""
    cfg = G.UNET_TINY
    B = 4
    cs, us = cond_for(cfg, B, 3, 1, 1), cond_for(cfg, B, 3, 1, 2)
    noise = O.replay_torch_noise(3, (B, 16, 16), cfg["num_labels"], 3, 2)
    run = lambda c, u, n, b: paella_amd.sample(tiny, to_dev(c, DEV), (b, 16, 16), unconditional_inputs=to_dev(u, DEV), steps=3, renoise_steps=2,
                                               device=DEV, noise=n)
    full = run(cs, us, noise, B)
    from paella_amd.dist import shard_bounds, shard_inputs
    parts = []
    for rank in range(2):
        lo, hi = shard_bounds(B, rank, 2)
        rows = 16 * 16
        n = {"init_noise": noise["init_noise"][lo:hi], "q": [q[lo * rows:hi * rows] for q in noise["q"]],
             "u": [u[lo:hi] if u is not None else None for u in noise["u"]]}
        parts.append(run(shard_inputs(cs, lo, hi), shard_inputs(us, lo, hi), n, hi - lo))
    assert torch.equal(full, torch.cat(parts, 0))


def test_add_noise_vs_reference(golden, tiny):
    g = golden("add_noise")
    x, t = torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["t"]).to(DEV)
    xn, mask = tiny.add_noise(x, t, mask=torch.from_numpy(g["user_mask"]).to(DEV), random_x=torch.from_numpy(g["random_x"]).to(DEV))
    assert np.array_equal(xn.cpu().numpy(), g["x_noised_user"]) and np.array_equal(mask.cpu().numpy(), g["mask_user"])
    torch.manual_seed(0)
    xn2, m2 = tiny.add_noise(x, t)
    frac = m2.float().mean(dim=(1, 2)).cpu()
    assert abs(float(frac[0]) - 0.3) < 0.1 and abs(float(frac[1]) - 0.8) < 0.1
    assert torch.equal(xn2[m2 == 0], x[m2 == 0])
    w = tiny.get_loss_weight(t, m2)
    assert w.shape == m2.shape


def test_graph_sampler_matches_eager(tiny, built_lib):
    """HIP-graph replay of sample() (+ decode) returns exactly what the eager philox path returns, and re-seeds per replay."""
    cfg = G.UNET_TINY
    cs, us = to_dev(cond_for(cfg, 2, 3, 0, 1), DEV), to_dev(cond_for(cfg, 2, 3, 0, 2), DEV)
    vq = paella_amd.VQModel(**G.VQ_TINY_F8)
    weights_for(vq, 2)
    vq = vq.to(DEV)
    gs = paella_amd.GraphSampler(tiny, cs, us, (2, 16, 16), steps=4, renoise_steps=3, device=DEV, vqgan=vq)
    torch.manual_seed(5)
    toks, img = gs(cs, us, seed=9)
    toks, img = toks.clone(), img.clone()
    torch.manual_seed(5)
    ref = paella_amd.sample(tiny, cs, (2, 16, 16), unconditional_inputs=us, steps=4, renoise_steps=3, device=DEV, noise="philox", seed=9)
    assert torch.equal(toks, ref)
    assert torch.equal(img, vq.decode_indices(ref))
    # new conditioning + seed through the same graph
    cs2 = to_dev(cond_for(cfg, 2, 3, 0, 11), DEV)
    torch.manual_seed(6)
    t2 = gs(cs2, us, seed=10)[0].clone()
    torch.manual_seed(6)
    ref2 = paella_amd.sample(tiny, cs2, (2, 16, 16), unconditional_inputs=us, steps=4, renoise_steps=3, device=DEV, noise="philox", seed=10)
    assert torch.equal(t2, ref2) and not torch.equal(t2, toks)


def test_inpaint_composition(tiny, built_lib):
    """encode -> masked add_noise -> sample(init_x, t_start<1) -> decode (BASELINE config 5 path, small)."""
    cfg = G.UNET_TINY
    vc = dict(G.VQ_TINY_F8, codebook_size=cfg["num_labels"])
    vq = paella_amd.VQModel(**vc)
    weights_for(vq, 2)
    vq = vq.to(DEV)
    g = torch.Generator().manual_seed(4)
    img = torch.rand(2, 3, 128, 128, generator=g).to(DEV)  # f8 -> 16x16 tokens
    cs, us = to_dev(cond_for(cfg, 2, 3, 0, 1), DEV), to_dev(cond_for(cfg, 2, 3, 0, 2), DEV)
    mask = torch.zeros(2, 16, 16, dtype=torch.int64)
    mask[:, 4:12, 4:12] = 1
    torch.manual_seed(1)
    toks, out = paella_amd.inpaint(tiny, vq, img, mask, cs, us, steps=4, t_start=0.6)
    orig = vq.encode(img)[2]
    assert out.shape == img.shape and toks.shape == orig.shape
    m = mask.to(DEV).bool()
    assert torch.equal(toks[~m], orig[~m])          # known region preserved (keep_known extension)
    assert (toks[m] != orig[m]).float().mean() > 0.2  # the hole was regenerated
    # an all-zero mask is the identity on tokens
    t0, _ = paella_amd.inpaint(tiny, vq, img, torch.zeros_like(mask), cs, us, steps=2, t_start=0.5, decode=False)
    assert torch.equal(t0, orig)


def test_config3_full_size_step_properties(built_lib):
    """BASELINE configs[2] at FULL size (573M-class, 64x64 tokens, batch 64, classifier-free guidance -> 128 rows x 4096
    positions, 8.6 GB of logits per half): one sampling step.  Too big for the CPU oracle, so size-independent properties:
    finite logits, tokens in range, the sampling step is deterministic, and rows sampled as part of the full batch equal
    the same rows sampled as a batch of 2 with the same per-row noise (batch-shard equivalence)."""
    cfg = G.UNET_570M
    m = paella_amd.Paella(**cfg)
    weights_for(m, sum(cfg["blocks"]))
    m = m.to(DEV)
    B, H = 64, 64
    L = cfg["num_labels"]
    cs, us = to_dev(cond_for(cfg, B, 0, 0, 41), DEV), to_dev(cond_for(cfg, B, 0, 0, 42), DEV)
    g = torch.Generator().manual_seed(9)
    init = torch.randint(0, L, (B, H, H), generator=g)
    u = torch.rand(B, H, H, generator=g)
    noise_full = {"init_noise": init, "q": [None], "u": [u]}
    # temperature 0 step: argmax sampling needs no [rows, L] noise tensor (would be another 8.6 GB)
    run = lambda c, un, n, b: paella_amd.sample(m, c, (b, H, H), unconditional_inputs=un, steps=1, renoise_steps=1, temperature=(0.0, 0.0),
                                                cfg=8.0, device=DEV, noise=n)
    full = run(cs, us, noise_full, B)
    assert full.shape == (B, H, H) and int(full.min()) >= 0 and int(full.max()) < L
    assert torch.equal(full, run(cs, us, noise_full, B))
    from paella_amd.dist import shard_inputs
    for lo in (0, 31, 62):
        c2, u2 = shard_inputs(cs, lo, lo + 2), shard_inputs(us, lo, lo + 2)
        # renoise off for the comparison run: the drawn tokens themselves are compared
        nz = lambda sl: {"init_noise": init[sl], "q": [None], "u": [None]}
        run0 = lambda c, un, n, b: paella_amd.sample(m, c, (b, H, H), unconditional_inputs=un, steps=1, renoise_steps=0, temperature=(0.0, 0.0),
                                                     cfg=8.0, device=DEV, noise=n)
        if lo == 0:
            full0 = run0(cs, us, nz(slice(0, B)), B)
        part = run0(c2, u2, nz(slice(lo, lo + 2)), 2)
        _assert_rows_match_up_to_near_ties(m, part, full0[lo:lo + 2], init[lo:lo + 2].to(DEV), c2, u2, 8.0)
    x = full[:2].contiguous()
    r = torch.tensor([0.5, 0.25], device=DEV)
    c2 = shard_inputs(cs, 0, 2)
    logits = m(x, r, **c2)
    assert torch.isfinite(logits).all()
    torch.cuda.empty_cache()


def test_config4_full_size_step_properties(built_lib):
    """BASELINE configs[3] per-GPU share at FULL size: released-size 1B model, ByT5 (768 tokens) + CLIP text + CLIP image
    conditioning, 64x64 tokens, batch 32 per GPU.  The unconditional set has a different (short) ByT5 length, so the two
    guidance passes cannot be batched and run as separate forwards (the other CFG code path).  One argmax step:
    tokens in range, deterministic, and a 2-row shard reproduces the same rows of the full batch up to near-tie flips."""
    cfg = G.UNET_1B
    m = paella_amd.Paella(**cfg)
    weights_for(m, sum(cfg["blocks"]))
    m = m.to(DEV)
    B, H = 32, 64
    L = cfg["num_labels"]
    cs, us = to_dev(cond_for(cfg, B, 768, 1, 51), DEV), to_dev(cond_for(cfg, B, 2, 1, 52), DEV)
    g = torch.Generator().manual_seed(10)
    init = torch.randint(0, L, (B, H, H), generator=g)
    u = torch.rand(B, H, H, generator=g)
    run = lambda c, un, lo, hi: paella_amd.sample(m, c, (hi - lo, H, H), unconditional_inputs=un, steps=1, renoise_steps=1, temperature=(0.0, 0.0),
                                                  cfg=8.0, device=DEV, noise={"init_noise": init[lo:hi], "q": [None], "u": [u[lo:hi]]})
    full = run(cs, us, 0, B)
    assert full.shape == (B, H, H) and int(full.min()) >= 0 and int(full.max()) < L
    assert torch.equal(full, run(cs, us, 0, B))
    from paella_amd.dist import shard_inputs
    run0 = lambda c, un, lo, hi: paella_amd.sample(m, c, (hi - lo, H, H), unconditional_inputs=un, steps=1, renoise_steps=0, temperature=(0.0, 0.0),
                                                   cfg=8.0, device=DEV, noise={"init_noise": init[lo:hi], "q": [None], "u": [None]})
    c2, u2 = shard_inputs(cs, 30, 32), shard_inputs(us, 30, 32)
    _assert_rows_match_up_to_near_ties(m, run0(c2, u2, 30, 32), run0(cs, us, 0, B)[30:32], init[30:32].to(DEV), c2, u2, 8.0)
    torch.cuda.empty_cache()


def test_config5_full_size_inpaint_properties(built_lib):
    """BASELINE configs[4] per-GPU share at FULL size: 1B model, 1024x1024 px = 128x128 tokens (VQGAN f8), batch 16 per GPU:
    VQGAN encode -> masked renoise -> sample(init_x, t_start < 1) -> decode.  Properties: shapes, token range, the known
    region is preserved and the hole is regenerated."""
    cfg = G.UNET_1B
    m = paella_amd.Paella(**cfg)
    weights_for(m, sum(cfg["blocks"]))
    m = m.to(DEV)
    vq = paella_amd.VQModel(levels=3)
    vsd = weights_for(vq, 2)
    vq = vq.to(DEV)
    B, P = 16, 1024
    g = torch.Generator().manual_seed(12)
    img = torch.rand(B, 3, P, P, generator=g).to(DEV)
    cs, us = to_dev(cond_for(cfg, B, 256, 1, 61), DEV), to_dev(cond_for(cfg, B, 256, 1, 62), DEV)
    mask = torch.zeros(B, 128, 128, dtype=torch.int64)
    mask[:, 32:96, 40:100] = 1
    torch.manual_seed(3)
    toks, out = paella_amd.inpaint(m, vq, img, mask, cs, us, steps=2, t_start=0.5, noise="philox", seed=5)
    orig = vq.encode(img)[2]
    assert toks.shape == (B, 128, 128) and out.shape == img.shape and torch.isfinite(out).all()
    assert int(toks.min()) >= 0 and int(toks.max()) < cfg["num_labels"]
    mk = mask.to(DEV).bool()
    assert torch.equal(toks[~mk], orig[~mk])
    assert (toks[mk] != orig[mk]).float().mean() > 0.2
    # orig comes from the same HIP encode the recipe used: image 15 (its activations past the 4 GiB offsets) against the oracle's encode of that image
    vc = G.VQ_F8
    with torch.no_grad():
        _, olat, oidx, _ = O.vq_encode(vsd, vc, img[15:16].cpu())
    rows = (olat * vc["scale_factor"]).permute(0, 2, 3, 1).reshape(-1, vc["c_latent"]).double()
    top = torch.cdist(rows, vsd["vquantizer.codebook.weight"].double()).pow(2).topk(2, dim=1, largest=False).values
    near = ((top[:, 1] - top[:, 0]) < 1e-5).view(oidx.shape)
    mism = orig[15:16].cpu() != oidx
    print("configs[4] inpaint, image 15 encode vs oracle: %d / %d tokens differ, all at nearest-code near-ties: %s" % (int(mism.sum()), mism.numel(), not bool((mism & ~near).any())))
    assert not (mism & ~near).any()
    torch.cuda.empty_cache()


def test_570m_closed_loop_three_steps_vs_oracle(built_lib):
    """BASELINE configs[1] model size: 570M-class stand-in, 32x32 tokens, batch 1, CFG 8, CLIP-text only -- three sampling steps
    with explicit noise against the CPU oracle (src/utils.py:35-55).  Per step every token must equal the oracle's draw unless
    the oracle's own decision was a near-tie (counted); with no such flip the closed-loop result is bit-identical."""
    cfg = G.UNET_570M
    m = paella_amd.Paella(**cfg)
    sd = weights_for(m, sum(cfg["blocks"]))
    m = m.to(DEV)
    c, u = cond_for(cfg, 1, 0, 0, G.COND_SEED), cond_for(cfg, 1, 0, 0, G.COND_SEED + 5)
    cs, us = to_dev(c, DEV), to_dev(u, DEV)
    steps = 3
    noise = O.replay_torch_noise(G.SAMPLER_SEED, (1, 32, 32), cfg["num_labels"], steps, steps - 1)
    fwd = _oracle_fwd(sd, cfg)
    rep = stepwise_token_parity(m, fwd, cfg["num_labels"], c, u, cs, us, noise, steps, steps - 1, (1.0, 0.2), 8.0)
    assert_token_parity(rep, "570M categorical, 3 steps")
    t_list = [float(v) for v in torch.linspace(1.0, 0.0, steps + 1)]
    temps = [float(v) for v in torch.linspace(1.0, 0.2, steps)]
    with torch.no_grad():
        otoks, _ = O.sample(fwd, cfg["num_labels"], c, u, (1, 32, 32), steps=steps, renoise_steps=steps - 1, temperatures=temps,
                            cfgs=[(8.0, -7.0)] * steps, t_list=t_list, noise=noise)
    toks = paella_amd.sample(m, cs, (1, 32, 32), unconditional_inputs=us, steps=steps, renoise_steps=steps - 1, temperature=(1.0, 0.2), cfg=8.0,
                             device=DEV, noise=noise)
    _exact_or_counted(toks, otoks.numpy(), rep, "570M 3-step sample vs oracle")


def test_570m_benchmarked_path_vs_unfused(built_lib):
    """What bench.py times -- shared CFG prefix + guidance mix folded through the linear head + in-kernel Philox noise -- against the
    reference's order of operations (two full evaluations, mix afterwards) on the SAME Philox noise: tokens must be identical
    except where the mixed logits put two labels within eps of each other in score (counted, printed)."""
    cfg = G.UNET_570M
    m = paella_amd.Paella(**cfg)
    weights_for(m, sum(cfg["blocks"]))
    m = m.to(DEV)
    B, H = 1, 32
    L = cfg["num_labels"]
    c, u = to_dev(cond_for(cfg, B, 0, 0, 2), DEV), to_dev(cond_for(cfg, B, 0, 0, 3), DEV)
    g = torch.Generator().manual_seed(1)
    x = torch.randint(0, L, (B, H, H), generator=g).to(DEV)
    r = torch.full((B,), 0.75, device=DEV)
    both = {k: (torch.cat([c[k], u[k]]) if c[k] is not None else None) for k in c}
    cache = m.prepare_cond(**both)
    a, b = 8.0, -7.0
    full = m.forward_prepared(torch.cat([x, x]), torch.cat([r, r]), cache).permute(0, 2, 3, 1).contiguous().clone()  # [2B,H,W,L]
    mixed = m.forward_prepared(x, r, cache, cfg_mix=(a, b)).permute(0, 2, 3, 1).contiguous().clone()                 # [B,H,W,L]
    ref_mix = full[:B] * a + full[B:] * b
    diff = (mixed - ref_mix).abs().max().item()
    rows = B * H * H
    out_f = torch.empty(B, H, H, dtype=torch.int64, device=DEV)
    out_u = torch.empty_like(out_f)
    lib = _lib.load()
    scores = torch.empty(rows, L, dtype=torch.float32, device=DEV)
    for temp in (1.0, 0.2):
        sampling._tail(mixed, None, rows, L, 1.0, 0.0, temp, 0, None, 77, 3, None, None, 0.0, out_f)
        sampling._tail(full[:B].contiguous(), full[B:].contiguous(), rows, L, a, b, temp, 0, None, 77, 3, None, None, 0.0, out_u)
        # decision margin of the REFERENCE-order path: the two best Gumbel-max scores (l/T - log q, the kernels' own arithmetic and
        # Philox counters) of every row.  The folded head moves a logit by <= diff, i.e. a score by <= diff/T: a token may differ only
        # where that margin is below 2*diff/T (+ one rounding of a score) -- every such position is counted, nothing else is tolerated.
        _lib.check(lib.paella_test_tail_scores(_lib.ptr(full[:B].contiguous()), _lib.ptr(full[B:].contiguous()), rows, L, a, b, temp, 77, 3, 0,
                                               _lib.ptr(scores), _lib.stream_ptr(torch.device(DEV))))
        torch.cuda.synchronize()
        top = scores.topk(2, dim=1).values
        assert torch.equal(scores.argmax(1).view(B, H, H), out_u), "score hook and tail kernel disagree"
        margin = (top[:, 0] - top[:, 1]).view(B, H, H)
        assert torch.isfinite(scores).all(), "a Gumbel score is not finite (u01_open must stay strictly inside (0, 1))"
        eps = 2.0 * diff / temp + 4e-6 * float(top[:, 0].abs().max())
        mism = out_f != out_u
        near = margin < eps
        n_mis, n_clear = int(mism.sum()), int((mism & ~near).sum())
        print("benchmarked path vs unfused, T=%.1f: max |logit diff| %.2e, near-tie eps %.2e: %d / %d tokens differ, all at near-ties: %s (%d rows are near-ties)"
              % (temp, diff, eps, n_mis, rows, n_clear == 0, int(near.sum())))
        assert n_clear == 0, "guidance-mix folding changed %d token(s) whose reference decision margin exceeds %.2e" % (n_clear, eps)
    assert diff <= 2e-4 * max(1.0, ref_mix.abs().max().item())
    am = (mixed.argmax(-1) != ref_mix.argmax(-1))
    top = ref_mix.topk(2, dim=-1).values
    near = (top[..., 0] - top[..., 1]) < 1e-3
    print("argmax agreement of the folded head: %d / %d differ, %d of them at margin < 1e-3" % (int(am.sum()), rows, int((am & near).sum())))
    assert not (am & ~near).any()


def test_tail_row_offset_is_exact(built_lib):
    """Philox counters are keyed by the GLOBAL row: rows [lo, hi) drawn with row_offset = lo equal the same rows of the full call."""
    g = torch.Generator().manual_seed(3)
    rows, L = 96, 256
    lc = torch.randn(rows, L, generator=g).to(DEV)
    init = torch.randint(0, L, (rows,), generator=g).to(DEV)
    full = torch.empty(rows, dtype=torch.int64, device=DEV)
    sampling._tail(lc, None, rows, L, 1.0, 0.0, 0.7, 0, None, 1234, 5, init, None, 0.4, full)
    for lo, hi in [(0, 32), (32, 33), (33, 96)]:
        part = torch.empty(hi - lo, dtype=torch.int64, device=DEV)
        sampling._tail(lc[lo:hi].contiguous(), None, hi - lo, L, 1.0, 0.0, 0.7, 0, None, 1234, 5, init[lo:hi].contiguous(), None, 0.4, part,
                       row_offset=lo)
        assert torch.equal(part, full[lo:hi])
    wrong = torch.empty(32, dtype=torch.int64, device=DEV)
    sampling._tail(lc[32:64].contiguous(), None, 32, L, 1.0, 0.0, 0.7, 0, None, 1234, 5, init[32:64].contiguous(), None, 0.4, wrong)
    assert not torch.equal(wrong, full[32:64])  # without the offset a shard would re-use the noise of rows 0..31


def test_philox_shard_equals_unsharded(tiny):
    """sample(noise="philox", shard=(lo, total)) reproduces rows [lo, lo + B) of the unsharded call bit for bit: start tokens,
    categorical draws and renoise masks are all functions of (seed, global row, step) -- SURVEY 8e."""
    cfg = G.UNET_TINY
    B = 4
    cs, us = cond_for(cfg, B, 3, 1, 1), cond_for(cfg, B, 3, 1, 2)
    from paella_amd.dist import shard_bounds, shard_inputs
    kw = dict(steps=3, renoise_steps=2, device=DEV, noise="philox", seed=99)
    full = paella_amd.sample(tiny, to_dev(cs, DEV), (B, 16, 16), unconditional_inputs=to_dev(us, DEV), **kw)
    parts = []
    for world in (2, 4):
        parts = []
        for rank in range(world):
            lo, hi = shard_bounds(B, rank, world)
            parts.append(paella_amd.sample(tiny, to_dev(shard_inputs(cs, lo, hi), DEV), (hi - lo, 16, 16),
                                           unconditional_inputs=to_dev(shard_inputs(us, lo, hi), DEV), shard=(lo, B), **kw))
        assert torch.equal(full, torch.cat(parts, 0)), "world size %d" % world
    # seed=None draws a fresh seed per call
    a = paella_amd.sample(tiny, to_dev(cs, DEV), (B, 16, 16), unconditional_inputs=to_dev(us, DEV), steps=2, renoise_steps=1, device=DEV, noise="philox")
    b = paella_amd.sample(tiny, to_dev(cs, DEV), (B, 16, 16), unconditional_inputs=to_dev(us, DEV), steps=2, renoise_steps=1, device=DEV, noise="philox")
    assert not torch.equal(a, b)


def test_start_tokens_shard_is_a_slice_of_the_global_draw(built_lib):
    """paella_start_tokens: token i of the global grid is a function of (seed, i) -- a shard draws its rows of the unsharded draw;
    seed and row offset may also arrive through device-resident words (what a captured graph uses)."""
    from paella_amd.sampling import start_tokens
    full = start_tokens(8192, (6, 8, 8), 77, DEV)
    assert int(full.min()) >= 0 and int(full.max()) < 8192 and full.float().std() > 1000
    for lo, n in [(0, 2), (2, 3), (5, 1)]:
        assert torch.equal(start_tokens(8192, (n, 8, 8), 77, DEV, shard=(lo, 6)), full[lo:lo + n])
    assert not torch.equal(full, start_tokens(8192, (6, 8, 8), 78, DEV))
    sd = torch.tensor([70], dtype=torch.int64, device=DEV)
    ro = torch.tensor([2 * 64], dtype=torch.int64, device=DEV)
    assert torch.equal(start_tokens(8192, (3, 8, 8), 7, DEV, seed_dev=sd, row_offset_dev=ro), full[2:5])


def test_graph_sampler_shard_equals_unsharded(tiny):
    """ONE captured graph serves every batch shard: GraphSampler(seed=s, shard=(lo, total)) == rows [lo, lo + B) of the unsharded eager
    sample(noise="philox", seed=s) over the global batch, bit for bit (start tokens, categorical draws and renoise masks are keyed by
    the global row through a device-resident offset word) -- the path bench.py --gpus N runs on every rank."""
    cfg = G.UNET_TINY
    total, Bs = 4, 2
    cs, us = cond_for(cfg, total, 3, 1, 1), cond_for(cfg, total, 3, 1, 2)
    from paella_amd.dist import shard_inputs
    kw = dict(steps=3, renoise_steps=2, temperature=(1.0, 0.3), cfg=8.0)
    full = paella_amd.sample(tiny, to_dev(cs, DEV), (total, 16, 16), unconditional_inputs=to_dev(us, DEV), device=DEV, noise="philox", seed=99, **kw)
    gs = paella_amd.GraphSampler(tiny, to_dev(shard_inputs(cs, 0, Bs), DEV), to_dev(shard_inputs(us, 0, Bs), DEV), (Bs, 16, 16), device=DEV, **kw)
    for lo in (0, 2):
        out = gs(to_dev(shard_inputs(cs, lo, lo + Bs), DEV), to_dev(shard_inputs(us, lo, lo + Bs), DEV), seed=99, shard=(lo, total)).clone()
        assert torch.equal(out, full[lo:lo + Bs]), "shard at row %d differs at %d positions" % (lo, int((out != full[lo:lo + Bs]).sum()))
    a = gs(seed=5).clone()
    assert not torch.equal(a, gs(seed=6))
    with pytest.raises(ValueError):
        gs(seed=1, shard=(3, 4))


@pytest.mark.parametrize("tail_tile", [14, 18, 9])
@pytest.mark.parametrize("cfg_name,B,grid", [("UNET_TINY", 3, 16), ("UNET_MID", 2, 16), ("UNET_570M", 1, 32)])
def test_fused_head_tail_is_bit_identical_to_the_two_kernel_path(built_lib, cfg_name, B, grid, tail_tile):
    """out_mapper fused with the sampling tail (no logits tensor; SURVEY section 7 step 3, reference src/utils.py:44-50): same
    tokens, bit for bit, as head GEMM -> logits -> tail kernel on the same Philox seed -- closed loop (every later step would
    amplify a single differing token), with guidance (mix folded through the head), without guidance, and with an argmax step."""
    cfg = dict(getattr(G, cfg_name))
    m = paella_amd.Paella(**cfg)
    weights_for(m, sum(cfg["blocks"]))
    m = m.to(DEV)
    cs, us = to_dev(cond_for(cfg, B, 3, 0, 1), DEV), to_dev(cond_for(cfg, B, 3, 0, 2), DEV)
    kw = dict(steps=3, renoise_steps=2, device=DEV, noise="philox", seed=4242)
    default_tile = 18  # paella_amd/csrc/gemm.hip g_tail_tile (only heads of >= 256 tiles of 128x128 use it: the 570M case here)
    built_lib.paella_test_gemm_tail_tile(tail_tile)
    try:
        _fused_vs_unfused(m, cfg, cfg_name, cs, us, B, grid, kw)
    finally:
        built_lib.paella_test_gemm_tail_tile(default_tile)


def _fused_vs_unfused(m, cfg, cfg_name, cs, us, B, grid, kw):
    for extra in (dict(unconditional_inputs=us, cfg=8.0, temperature=(1.0, 0.3)),
                  dict(unconditional_inputs=None, cfg=None, temperature=(0.9, 0.4)),
                  dict(unconditional_inputs=None, cfg=None, temperature=(0.5, 0.0))):   # last step T = 0 -> argmax mode
        a = paella_amd.sample(m, cs, (B, grid, grid), fused_tail=True, **kw, **extra)
        b = paella_amd.sample(m, cs, (B, grid, grid), fused_tail=False, **kw, **extra)
        assert torch.equal(a, b), "fused and two-kernel tails disagree at %d of %d positions" % (int((a != b).sum()), a.numel())
        assert int(a.min()) >= 0 and int(a.max()) < cfg["num_labels"]
    # sharded rows through the fused path too (row_offset reaches the GEMM epilogue's Philox counters)
    if B >= 2:
        from paella_amd.dist import shard_inputs
        full = paella_amd.sample(m, cs, (B, grid, grid), unconditional_inputs=us, cfg=8.0, **kw)
        part = paella_amd.sample(m, shard_inputs(cs, 1, B), (B - 1, grid, grid), unconditional_inputs=shard_inputs(us, 1, B), cfg=8.0, shard=(1, B), **kw)
        same = int((part == full[1:]).sum())
        print("%s fused shard rows 1..%d vs full batch: %d / %d identical" % (cfg_name, B - 1, same, part.numel()))
        if cfg_name == "UNET_TINY":
            assert same == part.numel()
