"""The attention core of a train-mode AttnBlock (in-projection -> scores -> softmax -> dropout -> @ v -> out-projection), two ways, on the same seeded inputs in ONE
process:

    torch   what `training._attn_block` runs by default: F.multi_head_attention_forward on the LayerNorm rows and the key rows, and autograd's backward through it
    fused   the route of set_training_attention("hip"): one F.linear for the queries, one for keys and values together, paella_amd.training.attention_dropout
            (paella_amd/csrc/attn_train.hip: one HIP op in both directions), the out-projection

Every part is one process and one GPU step; run each under its own time limit:

    timeout 300 python tools/bench_train_attention.py op   [--shapes 16x64x72x16x80 ...] [--rounds 7] [--iters 5] [--p 0.1] [--out FILE]
    timeout 300 python tools/bench_train_attention.py step [--step-model 570m] [--step-batch 16] [--step-grid 32] [--step-rounds 5] [--out FILE]
    timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d DIR_OFF -- python tools/bench_train_attention.py trace-step --setting torch --steps 3
    timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d DIR_ON  -- python tools/bench_train_attention.py trace-step --setting hip --steps 3
    python tools/bench_train_attention.py diff DIR_OFF DIR_ON --steps 4 [--out FILE]     (no device needed: reads the two traces; steps = warm-up + --steps)
    python tools/bench_train_attention.py kernels DIR [--match REGEX] [--out FILE]       (no device needed: dispatches grouped by kernel name and grid)

op: per shape B x P x L x nhead x D (the default shapes are the level-1 and level-2 geometries of the 570M model at 16 x 32x32 tokens and its level-1 geometry at
16 x 64x64 tokens, with 8 conditioning keys; level 2 at 64x64 tokens is level 1 at 32x32): one warm-up round of each path, then `rounds` rounds in which the two
paths take turns; a round is `iters` back-to-back forward + backward passes between two device synchronisations, timed on the host clock; reported is the median
(min, max) per pass.  Memory: torch.cuda.max_memory_allocated over one pass minus what was allocated before it (the rows, the projection weights and the incoming
gradient).  The script also checks, without dropout, that the two paths agree at the shapes it times.
step: one full training step (`forward_loss` + backward of the weighted mean loss, parameter gradients freed in between) with the other two switches on under
either `set_training_attention` setting, the settings taking turns: median time per step, peak memory above what is allocated before the step, what autograd
holds between the forward and the backward, and the op calls of one step.  "torch" is the parent commit's code op for op.
diff: kernel time per step by kernel name in the two traces; the rows that differ are the attention of the AttnBlocks.
Nothing is timed without a HIP device."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import train_ab as AB  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["op", "step", "trace-step", "diff", "kernels"])
    ap.add_argument("dirs", nargs="*")
    ap.add_argument("--shapes", nargs="+", default=["16x64x72x16x80", "16x16x24x16x80", "16x256x264x16x80"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--p", type=float, default=0.1)
    ap.add_argument("--step-model", default="570m")
    ap.add_argument("--step-batch", type=int, default=16)
    ap.add_argument("--step-grid", type=int, default=32)
    ap.add_argument("--step-rounds", type=int, default=5)
    ap.add_argument("--setting", default="torch", choices=["torch", "hip"])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--match", default="attn|attention|softmax|dropout|bmm|Cijk")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    report = AB.Report(a.out)
    say, finish, median = report.say, report.finish, AB.median

    if a.part == "diff":
        AB.trace_diff(say, a.dirs[0], a.dirs[1], a.steps, "attention", share=0.001, calls_too=True)
        return finish()

    if a.part == "kernels":
        AB.trace_kernels(say, a.dirs[0], a.match)
        return finish()

    import torch
    import torch.nn.functional as F

    from paella_amd import training
    if not torch.cuda.is_available():
        sys.exit("bench_train_attention.py needs a HIP device: nothing is timed without one")
    dev = torch.device("cuda", 0)

    if a.part == "op":
        say("training attention core with its projections, forward + backward, dropout %g: %d rounds of %d passes per path after one warm-up round, paths alternating"
            % (a.p, a.rounds, a.iters))
        say("%22s %6s %12s %12s %12s %18s %20s" % ("B x P x L x nhead x D", "path", "median ms", "min ms", "max ms", "peak MiB > inputs", "[B, nhead, P, L] MiB"))
        for spec in a.shapes:
            B, P, L, nhead, D = (int(v) for v in spec.split("x"))
            C = nhead * D
            gen = torch.Generator().manual_seed(B * P + L + C)
            leaf = lambda *s, scale=1.0: (torch.randn(*s, generator=gen) * scale).to(dev).requires_grad_(True)
            x, rows = leaf(B, P, C), leaf(B, L, C)
            w, bias, wo, bo = leaf(3 * C, C, scale=C ** -0.5), leaf(3 * C, scale=0.1), leaf(C, C, scale=C ** -0.5), leaf(C, scale=0.1)
            dy = torch.randn(B, P, C, generator=gen).to(dev)
            leaves = (x, rows, w, bias, wo, bo)

            def torch_pass(p=a.p):
                y, _ = F.multi_head_attention_forward(x.transpose(0, 1), rows.transpose(0, 1), rows.transpose(0, 1), C, nhead, w, bias, None, None, False, p, wo, bo,
                                                      training=True, need_weights=False)
                y = y.transpose(0, 1)
                return (y.detach(),) + torch.autograd.grad(y, leaves, dy)

            def fused_pass(p=a.p):
                y = F.linear(training.attention_dropout(F.linear(x, w[:C], bias[:C]), F.linear(rows, w[C:], bias[C:]), nhead, p), wo, bo)
                return (y.detach(),) + torch.autograd.grad(y, leaves, dy)

            res = {"torch": torch_pass(0.0), "fused": fused_pass(0.0)}   # agreement, without dropout (the two paths draw other masks)
            torch.cuda.synchronize(dev)
            for i, what in enumerate(("y", "dx", "drows", "dw", "dbias", "dwo", "dbo")):
                d = float((res["torch"][i].double() - res["fused"][i].double()).abs().max())
                mx = float(res["torch"][i].double().abs().max())
                say("#   %s: max |torch - fused| of %s: %.3e (max |torch| %.3e)" % (spec, what, d, mx))
                assert d <= 1e-4 * max(mx, 1.0), "the two paths disagree"
            del res
            paths = {"torch": torch_pass, "fused": fused_pass}
            for fn in paths.values():   # warm-up
                fn()
            peak = {name: AB.peak_of(dev, fn) for name, fn in paths.items()}
            times = AB.alternate(dev, paths, a.rounds, a.iters)
            one = B * nhead * P * L * 4 / 2 ** 20
            for name in paths:
                say("%22s %6s %12.3f %12.3f %12.3f %18.1f %20.1f" % ((spec, name) + median(times[name]) + (peak[name] / 2 ** 20, one)))
            del x, rows, w, bias, wo, bo, dy
            torch.cuda.empty_cache()
        return finish()

    S = AB.TrainStep(a.step_model, a.step_batch, a.step_grid, dev)
    first = dict(activation="hip", depthwise="hip")
    if a.part == "trace-step":
        AB.trace_step(say, S, "attention", a.setting, a.steps, first)
        return finish()
    AB.step_ab(say, S, "attention", a.step_rounds, first, training.ATTN_COUNTERS, " %10s" % "op calls", lambda c: " %10d" % c["calls"],
               AB.legend(S, "; the losses differ: the settings draw other dropout masks"))
    finish()


if __name__ == "__main__":
    main()
