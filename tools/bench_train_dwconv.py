"""The training ResBlock front ([cat with the skip ->] depthwise 3x3 -> LayerNorm2d -> NHWC), two ways, on the same seeded inputs in ONE process:

    torch   what `training._res_block` runs in front of its MLP by default: torch.cat -> F.conv2d(groups=C) -> F.layer_norm over a permuted view, and autograd's
            backward through that chain
    fused   paella_amd.training.dwconv_layernorm (paella_amd/csrc/dwconv_train.hip): the same stretch as one HIP op in both directions, x and skip read in place

Every part is one process and one GPU step; run each under its own time limit:

    timeout 300 python tools/bench_train_dwconv.py op   [--shapes 16x16x16x640 16x8x8x1280 16x4x4x1280] [--rounds 7] [--iters 5] [--out FILE]
    timeout 300 python tools/bench_train_dwconv.py step [--step-model 570m] [--step-batch 16] [--step-grid 32] [--step-rounds 5] [--out FILE]
    timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d DIR_OFF -- python tools/bench_train_dwconv.py trace-step --setting torch --steps 3
    timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d DIR_ON  -- python tools/bench_train_dwconv.py trace-step --setting hip --steps 3
    timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d DIR_OP  -- python tools/bench_train_dwconv.py op --rounds 2 --iters 3
    python tools/bench_train_dwconv.py diff DIR_OFF DIR_ON --steps 4 [--out FILE]        (no device needed: reads the two traces; steps = warm-up + --steps)
    python tools/bench_train_dwconv.py kernels DIR_OP [--match REGEX] [--out FILE]       (no device needed: dispatches grouped by kernel name and grid)

op: per shape [B, H, W, C], without and with a skip: one warm-up round of each path, then `rounds` rounds in which the two paths take turns; a round is `iters`
back-to-back forward + backward passes between two device synchronisations, timed on the host clock; reported is the median (min, max) per pass.  Memory:
torch.cuda.max_memory_allocated over one pass minus what was allocated before it (x, skip, weight, bias and the incoming gradient).  The inputs are NHWC-dense, as the
trunk is under the switch.  The script also checks that the two paths agree at the shapes it times.
step: one full training step (`forward_loss` + backward of the weighted mean loss, parameter gradients freed in between) with set_training_activation("hip") under
either `set_training_depthwise` setting, the settings taking turns: median time per step, peak memory above what is allocated before the step (weights and inputs;
no parameter gradients exist then under either setting, so the peak includes the step's own), what autograd holds between the forward and the backward, and how
many of one step's op calls had to copy an input that was not NHWC-dense.  "torch" is the parent commit's code op for op.
diff: kernel time per step by kernel name in the two traces; the rows that differ are the front of the ResBlocks (and whatever else the layout change moved).
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
    ap.add_argument("--shapes", nargs="+", default=["16x16x16x640", "16x8x8x1280", "16x4x4x1280"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--step-model", default="570m")
    ap.add_argument("--step-batch", type=int, default=16)
    ap.add_argument("--step-grid", type=int, default=32)
    ap.add_argument("--step-rounds", type=int, default=5)
    ap.add_argument("--setting", default="torch", choices=["torch", "hip"])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--match", default="dwconv")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    report = AB.Report(a.out)
    say, finish, median = report.say, report.finish, AB.median

    if a.part == "diff":
        AB.trace_diff(say, a.dirs[0], a.dirs[1], a.steps, "depthwise")
        return finish()

    if a.part == "kernels":
        AB.trace_kernels(say, a.dirs[0], a.match)
        return finish()

    import torch
    import torch.nn.functional as F

    from paella_amd import training
    if not torch.cuda.is_available():
        sys.exit("bench_train_dwconv.py needs a HIP device: nothing is timed without one")
    dev = torch.device("cuda", 0)

    if a.part == "op":
        say("training ResBlock front, forward + backward: %d rounds of %d passes per path after one warm-up round, paths alternating" % (a.rounds, a.iters))
        say("%16s %5s %6s %12s %12s %12s %18s %16s" % ("[B, H, W, C]", "skip", "path", "median ms", "min ms", "max ms", "peak MiB > inputs", "one tensor MiB"))
        for spec in a.shapes:
            B, H, W, C = (int(v) for v in spec.split("x"))
            for skip in (False, True):
                J = 2 if skip else 1
                gen = torch.Generator().manual_seed(B * H * W + C + J)
                nchw = lambda t: t.to(dev).permute(0, 3, 1, 2).requires_grad_(True)    # logical NCHW over NHWC memory, as the trunk is under the switch
                x = nchw(torch.randn(B, H, W, C, generator=gen))
                s = nchw(torch.randn(B, H, W, C, generator=gen)) if skip else None
                w = (torch.randn(C, J, 3, 3, generator=gen) * 0.3).to(dev).requires_grad_(True)
                bias = (torch.randn(C, generator=gen) * 0.5).to(dev).requires_grad_(True)
                dy = torch.randn(B, H, W, C, generator=gen).to(dev)
                leaves = (x, s, w, bias) if skip else (x, w, bias)

                def torch_pass():
                    xc = torch.cat([x, s], dim=1) if skip else x
                    y = F.layer_norm(F.conv2d(xc, w, bias, padding=1, groups=C).permute(0, 2, 3, 1), (C,), None, None, 1e-6)
                    return (y.detach(),) + torch.autograd.grad(y, leaves, dy)

                def fused_pass():
                    y = training.dwconv_layernorm(x, w, bias, s)
                    return (y.detach(),) + torch.autograd.grad(y, leaves, dy)

                paths = {"torch": torch_pass, "fused": fused_pass}
                res = {name: fn() for name, fn in paths.items()}   # warm-up, and agreement
                torch.cuda.synchronize(dev)
                for i, what in enumerate(("y", "dx", "dskip", "dw", "dbias") if skip else ("y", "dx", "dw", "dbias")):
                    d = float((res["torch"][i].double() - res["fused"][i].double()).abs().max())
                    m = float(res["torch"][i].double().abs().max())
                    say("#   %s%s: max |torch - fused| of %s: %.3e (max |torch| %.3e)" % (spec, " skip" if skip else "", what, d, m))
                    assert d <= 1e-4 * max(m, 1.0), "the two paths disagree"
                del res
                peak = {name: AB.peak_of(dev, fn) for name, fn in paths.items()}
                times = AB.alternate(dev, paths, a.rounds, a.iters)
                one = B * H * W * C * 4 / 2 ** 20
                for name in paths:
                    say("%16s %5s %6s %12.3f %12.3f %12.3f %18.1f %16.1f" % ((spec, "yes" if skip else "no", name) + median(times[name]) + (peak[name] / 2 ** 20, one)))
                del x, s, w, bias, dy
                torch.cuda.empty_cache()
        return finish()

    S = AB.TrainStep(a.step_model, a.step_batch, a.step_grid, dev)
    first = dict(activation="hip")
    if a.part == "trace-step":
        AB.trace_step(say, S, "depthwise", a.setting, a.steps, first)
        return finish()
    AB.step_ab(say, S, "depthwise", a.step_rounds, first, training.DW_COUNTERS, " %10s %14s" % ("op calls", "inputs copied"),
               lambda c: " %10d %14d" % (c["calls"], c["copied"]), AB.legend(S))
    finish()


if __name__ == "__main__":
    main()
