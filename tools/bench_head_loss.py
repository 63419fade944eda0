"""Forward + backward of the training loss head, two ways, on the same seeded inputs in ONE process:

    torch   what a training step ran before the fused op: F.conv2d(LayerNorm output, out_mapper.1.weight) -> nn.CrossEntropyLoss(label_smoothing, reduction='none')
            -> backward to the gradients of the features and of the weight (autograd keeps logits, log-softmax and the logit gradient)
    fused   paella_amd.training.head_cross_entropy (paella_amd/csrc/loss.hip): the same loss and the same two gradients, no logits tensor

    python tools/bench_head_loss.py [--rows 16384 65536] [--labels 8192] [--k 256] [--rounds 7] [--iters 5] [--out profiles/head_loss_ab.txt]

Time: per shape one warm-up round of each path, then `rounds` rounds in which the two paths take turns; a round is `iters` back-to-back forward + backward passes
between two device synchronisations, timed on the host clock; reported is the median (min, max) per pass.  Memory: torch.cuda.max_memory_allocated over one pass
minus what was allocated before it (the inputs), and for the fused op also minus its outputs (loss, argmax, both gradients) -- the figure the op's contract bounds
by a quarter of one fp32 logits tensor.  The script also checks that the two paths agree (loss and gradients to fp32 reordering error) at the shapes it times.
Nothing is timed without a HIP device."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import train_ab as AB  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[16 * 32 * 32, 16 * 64 * 64])
    ap.add_argument("--labels", type=int, default=8192)
    ap.add_argument("--k", type=int, default=256)
    ap.add_argument("--eps", type=float, default=0.1)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from torch import nn

    from paella_amd import training
    if not torch.cuda.is_available():
        sys.exit("bench_head_loss.py needs a HIP device: nothing is timed without one")
    dev = torch.device("cuda", 0)
    N, K, eps = a.labels, a.k, a.eps
    report = AB.Report(a.out)
    say = report.say
    say("training loss head, forward + backward: K = %d, N = %d, label_smoothing = %g; %d rounds of %d passes per path after one warm-up round, paths alternating"
        % (K, N, eps, a.rounds, a.iters))
    say("%8s %6s %12s %12s %12s %16s %22s %18s" % ("rows", "path", "median ms", "min ms", "max ms", "peak MiB > inputs", "peak MiB > in + outputs", "one logits MiB"))
    for rows in a.rows:
        gen = torch.Generator().manual_seed(rows)
        h = torch.randn(rows, K, generator=gen).to(dev).requires_grad_(True)
        w = (torch.randn(N, K, 1, 1, generator=gen) / K ** 0.5).to(dev).requires_grad_(True)
        t = torch.randint(0, N, (rows,), generator=gen).to(dev)
        g = (torch.rand(rows, generator=gen) * 2).to(dev)
        crit = nn.CrossEntropyLoss(label_smoothing=eps, reduction='none')

        def torch_pass():
            pred = F.conv2d(h.view(1, rows, 1, K).permute(0, 3, 1, 2), w)
            loss = crit(pred, t.view(1, rows, 1)).view(rows)
            return (loss.detach(),) + torch.autograd.grad(loss, (h, w), g)

        def fused_pass():
            loss, _ = training.head_cross_entropy(h, w, t, eps)
            return (loss.detach(),) + torch.autograd.grad(loss, (h, w), g)

        paths = {"torch": torch_pass, "fused": fused_pass}
        res = {name: fn() for name, fn in paths.items()}   # warm-up, agreement and memory
        torch.cuda.synchronize(dev)
        # outputs: + the int32 argmax of the fused op (the torch path has none: its figure is not used)
        peak = {name: (AB.peak_of(dev, fn), sum(o.numel() * o.element_size() for o in res[name]) + rows * 4) for name, fn in paths.items()}
        for i, what in enumerate(("loss", "dh", "dw")):
            d = float((res["torch"][i].double() - res["fused"][i].double()).abs().max())
            s = float(res["torch"][i].double().abs().max())
            say("#   rows %d: max |torch - fused| of %s = %.3e (max |torch| %.3e)" % (rows, what, d, s))
            assert d <= 1e-4 * max(s, 1.0), "the two paths disagree"
        del res
        times = AB.alternate(dev, paths, a.rounds, a.iters)
        logits_mib = rows * N * 4 / 2 ** 20
        for name in paths:
            p, o = peak[name]
            say("%8d %6s %12.3f %12.3f %12.3f %16.1f %22s %18.1f" % ((rows, name) + AB.median(times[name]) + (p / 2 ** 20,
                                                                  "%.1f" % ((p - o) / 2 ** 20) if name == "fused" else "-", logits_mib)))
        p, o = peak["fused"]
        say("#   rows %d: fused peak above inputs and outputs %.1f MiB, bound (a quarter of one logits tensor) %.1f MiB: %s; torch peak %.2f logits tensors"
            % (rows, (p - o) / 2 ** 20, logits_mib / 4, "under" if p - o < rows * N else "OVER", peak["torch"][0] / (rows * N * 4)))
        del h, w, t, g
        torch.cuda.empty_cache()
    report.finish()


if __name__ == "__main__":
    main()
