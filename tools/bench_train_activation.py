"""The training MLP activation (GELU -> GlobalResponseNorm -> Dropout), two ways, on the same seeded inputs in ONE process:

    torch   what `training._channelwise` runs between its two Linears by default: F.gelu -> torch.norm over the positions -> channel mean -> divide ->
            gamma * (h * nx) + beta + h -> F.dropout, and autograd's backward through that chain
    fused   paella_amd.training.gelu_grn_dropout (paella_amd/csrc/grn_act.hip): the same stretch as one HIP op in both directions; autograd keeps the pre-activation
            and one [B, C] table

    python tools/bench_train_activation.py [--shapes 16x256x2560 16x64x5120] [--p 0.1] [--rounds 7] [--iters 5] [--step-model 570m] [--step-batch 16] [--step-grid 32]
                                           [--no-step] [--out profiles/train_activation_ab.txt]

Op level, per shape [B, P, C]: one warm-up round of each path, then `rounds` rounds in which the two paths take turns; a round is `iters` back-to-back forward +
backward passes between two device synchronisations, timed on the host clock; reported is the median (min, max) per pass.  Memory: torch.cuda.max_memory_allocated
over one pass minus what was allocated before it (the inputs u, gamma, beta and the incoming gradient).  The script also checks that the two paths agree at p = 0
at the shapes it times.
Step level: one full training step (`forward_loss` + backward of the weighted mean loss, parameter gradients freed in between) of the `--step-model` network at
`--step-batch` x `--step-grid`^2 tokens under either `set_training_activation` setting, the settings taking turns: median time per step and peak memory above what is
allocated before the step (weights and inputs).
Nothing is timed without a HIP device."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["16x256x2560", "16x64x5120"])
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--step-model", default="570m")
    ap.add_argument("--step-batch", type=int, default=16)
    ap.add_argument("--step-grid", type=int, default=32)
    ap.add_argument("--step-rounds", type=int, default=5)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F

    import paella_amd
    from paella_amd import synth, training
    if not torch.cuda.is_available():
        sys.exit("bench_train_activation.py needs a HIP device: nothing is timed without one")
    dev = torch.device("cuda", 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def median(v):
        v = sorted(v)
        return v[len(v) // 2], v[0], v[-1]

    def alternate(paths, rounds, iters):
        times = {n: [] for n in paths}
        for _ in range(rounds):
            for name, fn in paths.items():
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(iters):
                    fn()
                torch.cuda.synchronize(dev)
                times[name].append((time.perf_counter() - t0) * 1e3 / iters)
        return times

    def peak_of(fn):
        torch.cuda.empty_cache()
        torch.cuda.synchronize(dev)
        base = torch.cuda.memory_allocated(dev)
        torch.cuda.reset_peak_memory_stats(dev)
        out = fn()
        torch.cuda.synchronize(dev)
        peak = torch.cuda.max_memory_allocated(dev) - base
        del out
        return peak

    say("training MLP activation, forward + backward: dropout p = %g; %d rounds of %d passes per path after one warm-up round, paths alternating" % (a.p, a.rounds, a.iters))
    say("%16s %6s %12s %12s %12s %18s %16s" % ("[B, P, C]", "path", "median ms", "min ms", "max ms", "peak MiB > inputs", "one tensor MiB"))
    for spec in a.shapes:
        B, P, C = (int(v) for v in spec.split("x"))
        gen = torch.Generator().manual_seed(B * P + C)
        u = (torch.randn(B, P, 1, C, generator=gen) * 1.5).to(dev).requires_grad_(True)   # [B, H, W, C] as _channelwise sees it
        gamma = (torch.randn(1, 1, 1, C, generator=gen) * 0.5).to(dev).requires_grad_(True)
        beta = (torch.randn(1, 1, 1, C, generator=gen) * 0.5).to(dev).requires_grad_(True)
        dz = torch.randn(B, P, 1, C, generator=gen).to(dev)

        def torch_pass(p=a.p):
            h = F.gelu(u)
            gx = torch.norm(h, p=2, dim=(1, 2), keepdim=True)
            nx = gx / (gx.mean(dim=-1, keepdim=True) + 1e-6)
            z = F.dropout(gamma * (h * nx) + beta + h, p, True)
            return (z.detach(),) + torch.autograd.grad(z, (u, gamma, beta), dz)

        def fused_pass(p=a.p):
            z = training.gelu_grn_dropout(u, gamma, beta, p)
            return (z.detach(),) + torch.autograd.grad(z, (u, gamma, beta), dz)

        paths = {"torch": torch_pass, "fused": fused_pass}
        res = {name: fn(0.0) for name, fn in paths.items()}   # agreement at p = 0 (with dropout the two paths draw different masks)
        torch.cuda.synchronize(dev)
        for i, what in enumerate(("z", "du", "dgamma", "dbeta")):
            d = float((res["torch"][i].double() - res["fused"][i].double()).abs().max())
            s = float(res["torch"][i].double().abs().max())
            say("#   %s: max |torch - fused| of %s at p = 0: %.3e (max |torch| %.3e)" % (spec, what, d, s))
            assert d <= 1e-4 * max(s, 1.0), "the two paths disagree"
        del res
        for fn in paths.values():   # warm-up at the timed p
            fn()
        peak = {name: peak_of(fn) for name, fn in paths.items()}
        times = alternate(paths, a.rounds, a.iters)
        one = B * P * C * 4 / 2 ** 20
        for name in paths:
            say("%16s %6s %12.3f %12.3f %12.3f %18.1f %16.1f" % ((spec, name) + median(times[name]) + (peak[name] / 2 ** 20, one)))
        say("#   %s: peak above the inputs, in activation tensors: torch %.2f, fused %.2f (z and du are two of them on either path)"
            % (spec, peak["torch"] / (one * 2 ** 20), peak["fused"] / (one * 2 ** 20)))
        del u, gamma, beta, dz
        torch.cuda.empty_cache()

    if not a.no_step:
        import bench
        cfg = bench.MODELS[a.step_model]
        m = paella_amd.Paella(**cfg)
        synth.randomize_(m, seed=0)
        m = m.to(dev)
        m.train()
        Bs, g = a.step_batch, a.step_grid
        gen = torch.Generator().manual_seed(7)
        latents = torch.randint(0, cfg["num_labels"], (Bs, g, g), generator=gen).to(dev)
        t = torch.rand(Bs, generator=gen).to(dev)
        mask = (torch.rand(Bs, g, g, generator=gen) < t.cpu()[:, None, None]).long().to(dev)
        random_x = torch.randint(0, cfg["num_labels"], (Bs, g, g), generator=gen).to(dev)
        cond = synth.synth_conditioning(Bs, 4, cfg["byt5_embd"], cfg["clip_embd"], seed=2, device=dev)
        noised = latents * (1 - mask) + random_x * mask
        lw = m.get_loss_weight(t, mask)

        def step_with(mode):
            def step():
                m.set_training_activation(mode)
                m.zero_grad(set_to_none=True)
                loss, _ = m.forward_loss(noised, t, latents, **cond)
                loss = ((loss * lw).sum(dim=[1, 2]) / lw.sum(dim=[1, 2])).mean()
                loss.backward()
                return loss.detach()
            return step

        paths = {"torch": step_with("torch"), "hip": step_with("hip")}
        say("one training step (forward_loss + backward), model %s (%.1fM parameters), %d x %dx%d tokens, dropout %s; %d rounds of 1 step per setting after one warm-up, "
            "settings alternating" % (a.step_model, sum(p.numel() for p in m.parameters()) / 1e6, Bs, g, g, m.dropout, a.step_rounds))
        losses = {name: float(fn()) for name, fn in paths.items()}   # warm-up
        m.zero_grad(set_to_none=True)
        peak = {name: peak_of(fn) for name, fn in paths.items()}
        m.zero_grad(set_to_none=True)
        times = alternate(paths, a.step_rounds, 1)
        say("%10s %12s %12s %12s %26s %12s" % ("setting", "median ms", "min ms", "max ms", "peak MiB > weights + inputs", "loss"))
        for name in paths:
            say("%10s %12.2f %12.2f %12.2f %26.1f %12.5f" % ((name,) + median(times[name]) + (peak[name] / 2 ** 20, losses[name])))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
