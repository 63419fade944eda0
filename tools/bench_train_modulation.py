"""The joint around a train-mode TimestepBlock (residual add of the block in front -> x (1 + a) + b -> LayerNorm rows for the block behind), two ways, on the same
seeded inputs in ONE process:

    torch   what `training._forward_features` runs by default: the add that ends `_res_block` / `_ff_block`, `_timestep_block` (chunk of the mapper's output, two
            elementwise ops), `_ln_nchw` at the head of `_attn_block` / `_ff_block`, and autograd's backward through them
    fused   the route of set_training_modulation("hip"): paella_amd.training.timestep_modulate (paella_amd/csrc/mod_train.hip: one HIP op in both directions)

Every part is one process and one GPU step; run each under its own time limit:

    timeout 300 python tools/bench_train_modulation.py op   [--shapes 16x16x16x640 ...] [--rounds 7] [--iters 5] [--out FILE]
    timeout 300 python tools/bench_train_modulation.py step [--step-model 570m] [--step-batch 16] [--step-grid 32] [--step-rounds 5] [--out FILE]
    timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d DIR_OFF -- python tools/bench_train_modulation.py trace-step --setting torch --steps 3
    timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d DIR_ON  -- python tools/bench_train_modulation.py trace-step --setting hip --steps 3
    python tools/bench_train_modulation.py diff DIR_OFF DIR_ON --steps 4 [--out FILE]     (no device needed: reads the two traces; steps = warm-up + --steps)

op: per shape B x H x W x C (the defaults are the three levels of the 570M model at 16 x 32x32 tokens), with a residual and the LayerNorm (the `C T A` joint) and
with a residual alone (the `C T` joint): one warm-up round of each path, then `rounds` rounds in which the two paths take turns; a round is `iters` back-to-back
forward + backward passes between two device synchronisations, timed on the host clock; reported is the median (min, max) per pass and the peak memory of one pass
above its inputs.  The script also checks that the two paths agree at the shapes it times.
step: one full training step (`forward_loss` + backward of the weighted mean loss, parameter gradients freed in between) with the other three switches on under
either `set_training_modulation` setting, the settings taking turns: median time per step, peak memory above what is allocated before the step, what autograd holds
between the forward and the backward, and the op calls of one step.  "torch" is the parent commit's code op for op.
diff: kernel time and calls per step by kernel name in the two traces.
Nothing is timed without a HIP device."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import train_ab as AB  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["op", "step", "trace-step", "diff"])
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
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    report = AB.Report(a.out)
    say, finish, median = report.say, report.finish, AB.median

    if a.part == "diff":
        AB.trace_diff(say, a.dirs[0], a.dirs[1], a.steps, "modulation", share=0.001, calls_too=True)
        return finish()

    import torch

    from paella_amd import training
    if not torch.cuda.is_available():
        sys.exit("bench_train_modulation.py needs a HIP device: nothing is timed without one")
    dev = torch.device("cuda", 0)

    if a.part == "op":
        say("training timestep joint, forward + backward: %d rounds of %d passes per path after one warm-up round, paths alternating" % (a.rounds, a.iters))
        say("%18s %8s %6s %12s %12s %12s %18s %16s" % ("B x H x W x C", "joint", "path", "median ms", "min ms", "max ms", "peak MiB > inputs", "one tensor MiB"))
        for spec in a.shapes:
            B, H, W, C = (int(v) for v in spec.split("x"))
            gen = torch.Generator().manual_seed(B * H + W + C)
            leaf = lambda *s, scale=1.0: (torch.randn(*s, generator=gen) * scale).to(dev).requires_grad_(True)
            # what the blocks hand over: the MLP output and the trunk, logical [B, C, H, W] over NHWC memory; the mapper's output; the incoming gradients
            x, res, ab = leaf(B, H, W, C), leaf(B, H, W, C), leaf(B, 2 * C, scale=0.5)
            dxp, dz = torch.randn(B, H, W, C, generator=gen).to(dev).permute(0, 3, 1, 2), torch.randn(B, H * W, C, generator=gen).to(dev)
            leaves = (x, res, ab)
            for ln in (True, False):

                def torch_pass(ln=ln):
                    h = x.permute(0, 3, 1, 2) + res.permute(0, 3, 1, 2)
                    sa, sb = ab[:, :, None, None].chunk(2, dim=1)
                    xp = h * (1 + sa) + sb
                    outs = [xp] + ([training._ln_nchw(xp).reshape(B, C, H * W).permute(0, 2, 1)] if ln else [])
                    return [o.detach() for o in outs] + list(torch.autograd.grad(outs, leaves, [dxp, dz][:len(outs)]))

                def fused_pass(ln=ln):
                    out = training.timestep_modulate(x.permute(0, 3, 1, 2), ab, res.permute(0, 3, 1, 2), ln)
                    outs = list(out) if ln else [out]
                    return [o.detach() for o in outs] + list(torch.autograd.grad(outs, leaves, [dxp, dz][:len(outs)]))

                res_t, res_f = torch_pass(), fused_pass()   # agreement (and the warm-up)
                torch.cuda.synchronize(dev)
                names = ["xp"] + (["z"] if ln else []) + ["dx", "dres", "dab"]
                for what, t, f in zip(names, res_t, res_f):
                    d = float((t.double() - f.double()).abs().max())
                    mx = float(t.double().abs().max())
                    say("#   %s %s: max |torch - fused| of %s: %.3e (max |torch| %.3e)" % (spec, "C T A" if ln else "C T", what, d, mx))
                    assert d <= 1e-4 * max(mx, 1.0), "the two paths disagree"
                del res_t, res_f
                paths = {"torch": torch_pass, "fused": fused_pass}
                peak = {name: AB.peak_of(dev, fn) for name, fn in paths.items()}
                times = AB.alternate(dev, paths, a.rounds, a.iters)
                for name in paths:
                    say("%18s %8s %6s %12.3f %12.3f %12.3f %18.1f %16.1f" % ((spec, "C T A" if ln else "C T", name) + median(times[name])
                                                                            + (peak[name] / 2 ** 20, B * H * W * C * 4 / 2 ** 20)))
            del x, res, ab, dxp, dz
            torch.cuda.empty_cache()
        return finish()

    S = AB.TrainStep(a.step_model, a.step_batch, a.step_grid, dev)
    first = dict(activation="hip", depthwise="hip", attention="hip")
    if a.part == "trace-step":
        AB.trace_step(say, S, "modulation", a.setting, a.steps, first)
        return finish()
    AB.step_ab(say, S, "modulation", a.step_rounds, first, training.MOD_COUNTERS, "  %s" % "op calls (with residual, with LayerNorm, inputs copied)",
               lambda c: "  %d (%d, %d, %d)" % (c["calls"], c["residual"], c["layernorm"], c["copied"]),
               AB.legend(S, "; the losses differ: each step draws its own dropout masks"))
    finish()


if __name__ == "__main__":
    main()
