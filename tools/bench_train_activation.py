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

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import train_ab as AB  # noqa: E402


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

    from paella_amd import training
    if not torch.cuda.is_available():
        sys.exit("bench_train_activation.py needs a HIP device: nothing is timed without one")
    dev = torch.device("cuda", 0)
    report = AB.Report(a.out)
    say, median = report.say, AB.median
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
        peak = {name: AB.peak_of(dev, fn) for name, fn in paths.items()}
        times = AB.alternate(dev, paths, a.rounds, a.iters)
        one = B * P * C * 4 / 2 ** 20
        for name in paths:
            say("%16s %6s %12.3f %12.3f %12.3f %18.1f %16.1f" % ((spec, name) + median(times[name]) + (peak[name] / 2 ** 20, one)))
        say("#   %s: peak above the inputs, in activation tensors: torch %.2f, fused %.2f (z and du are two of them on either path)"
            % (spec, peak["torch"] / (one * 2 ** 20), peak["fused"] / (one * 2 ** 20)))
        del u, gamma, beta, dz
        torch.cuda.empty_cache()

    if not a.no_step:
        AB.step_ab(say, AB.TrainStep(a.step_model, a.step_batch, a.step_grid, dev), "activation", a.step_rounds)
    report.finish()


if __name__ == "__main__":
    main()
