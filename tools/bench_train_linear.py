"""The routed linears of a train-mode step (the two of every MLP, the q / kv / out projections around `attention_dropout`), two ways, on the same seeded inputs
in ONE process:

    fp32    what `training._forward_features` runs by default: torch's F.linear, forward and backward (the vendor BLAS in fp32)
    bf16    the route of set_training_gemm("bf16"): paella_amd.training.linear_bf16 (paella_amd/csrc/linear_train.hip: operands packed to bf16 in one pass per tensor,
            forward, dgrad and wgrad on the bf16 matrix cores with fp32 accumulation)

Every part is one process and one GPU step; run each under its own time limit:

    timeout 300 python tools/bench_train_linear.py op    [--shapes 4096x2560x640 ...] [--rounds 7] [--iters 5] [--out FILE]
    timeout 300 python tools/bench_train_linear.py pack  [--shapes ...] [--rounds 7] [--iters 20] [--out FILE]
    timeout 300 python tools/bench_train_linear.py step  [--step-model 570m] [--step-batch 16] [--step-grid 32] [--step-rounds 5] [--out FILE]
    timeout 300 python tools/bench_train_linear.py loss  [--step-model 570m] [--step-batch 16] [--step-grid 32] [--steps 20] [--out FILE]
    timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d DIR_OFF -- python tools/bench_train_linear.py trace-step --setting fp32 --steps 3
    timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d DIR_ON  -- python tools/bench_train_linear.py trace-step --setting bf16 --steps 3
    python tools/bench_train_linear.py diff DIR_OFF DIR_ON --steps 4 [--out FILE]     (no device needed: reads the two traces; steps = warm-up + --steps)

op: per shape M x N x K (rows, output features, input features; the defaults are the MLP and projection shapes of the 570M model at 16 x 32x32 tokens), with a bias
and every gradient wanted: one warm-up round of each path, then `rounds` rounds in which the two paths take turns; a round is `iters` back-to-back forward + backward
passes between two device synchronisations, timed on the host clock; reported is the median (min, max) per pass and the TFLOP/s of its three GEMMs (6 M N K).  The
script also reports how far the two paths are apart at the shapes it times (the rounding of the operands: relative 2^-9 per element).
pack: per shape M x N x K the pack over dy [M, N] with all three outputs (row-major, transposed, column sums) and the row-major pack alone, against a device copy
(float4 loads and stores) of the same fp32 bytes: median time and the bytes each moves.
step: one full training step (`forward_loss` + backward of the weighted mean loss, parameter gradients freed in between) with the other four switches on under
either `set_training_gemm` setting, the settings taking turns: median time per step, peak memory, what autograd holds, and the op calls / fallbacks of one step.
"fp32" is the parent commit's code op for op.
loss: the loss of the first `steps` optimizer steps (ClippedAdamW, lr 1e-4, dropout 0, one fixed batch) under either setting, from the same initial weights.
diff: kernel time and calls per step by kernel name in the two traces.
Nothing is timed without a HIP device."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import train_ab as AB  # noqa: E402

# 570M at 16 x 32x32 tokens: levels of 4096 / 1024 / 256 rows and 640 / 1280 / 1280 channels -- MLP in, MLP out, and the square projections
SHAPES_570M = ["4096x2560x640", "4096x640x2560", "1024x5120x1280", "1024x1280x5120", "256x5120x1280", "256x1280x5120", "1024x1280x1280", "1024x2560x1280", "256x1280x1280"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["op", "pack", "step", "loss", "trace-step", "diff"])
    ap.add_argument("dirs", nargs="*")
    ap.add_argument("--shapes", nargs="+", default=SHAPES_570M)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--step-model", default="570m")
    ap.add_argument("--step-batch", type=int, default=16)
    ap.add_argument("--step-grid", type=int, default=32)
    ap.add_argument("--step-rounds", type=int, default=5)
    ap.add_argument("--setting", default="fp32", choices=["fp32", "bf16"])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    report = AB.Report(a.out)
    say, finish, median = report.say, report.finish, AB.median

    if a.part == "diff":
        AB.trace_diff(say, a.dirs[0], a.dirs[1], a.steps, "training gemm", share=0.001, calls_too=True)
        return finish()

    import torch
    import torch.nn.functional as F

    from paella_amd import training
    if not torch.cuda.is_available():
        sys.exit("bench_train_linear.py needs a HIP device: nothing is timed without one")
    dev = torch.device("cuda", 0)

    if a.part == "op":
        say("training linear, forward + backward (dx, dW, db): %d rounds of %d passes per path after one warm-up round, paths alternating" % (a.rounds, a.iters))
        say("%18s %6s %12s %12s %12s %10s" % ("M x N x K", "path", "median ms", "min ms", "max ms", "TFLOP/s"))
        for spec in a.shapes:
            M, N, K = (int(v) for v in spec.split("x"))
            gen = torch.Generator().manual_seed(M + N + K)
            leaf = lambda *s, scale=1.0: (torch.randn(*s, generator=gen) * scale).to(dev).requires_grad_(True)
            x, w, b = leaf(M, K), leaf(N, K, scale=K ** -0.5), leaf(N)
            dy = torch.randn(M, N, generator=gen).to(dev)

            def run(fn):
                y = fn(x, w, b)
                return [y.detach()] + list(torch.autograd.grad(y, (x, w, b), dy))

            paths = {"fp32": lambda: run(F.linear), "bf16": lambda: run(training.linear_bf16)}
            res_t, res_f = paths["fp32"](), paths["bf16"]()
            torch.cuda.synchronize(dev)
            for what, t, f in zip(("y", "dx", "dW", "db"), res_t, res_f):
                say("#   %s: relative L2 distance of %s between the paths: %.3e" % (spec, what, float((t.double() - f.double()).norm() / t.double().norm())))
            del res_t, res_f
            times = AB.alternate(dev, paths, a.rounds, a.iters)
            for name in paths:
                med = median(times[name])
                say("%18s %6s %12.3f %12.3f %12.3f %10.1f" % ((spec, name) + med + (6.0 * M * N * K / (med[0] * 1e-3) / 1e12,)))
            del x, w, b, dy
            torch.cuda.empty_cache()
        return finish()

    if a.part == "pack":
        say("the pack over dy [M, N] against a device copy of the same fp32 bytes: %d rounds of %d calls per path after one warm-up round, paths alternating" % (a.rounds, a.iters))
        say("%18s %22s %12s %12s %12s %10s %10s" % ("M x N x K", "path", "median us", "min us", "max us", "MB moved", "GB/s"))
        for spec in a.shapes:
            M, N, _ = (int(v) for v in spec.split("x"))
            gen = torch.Generator().manual_seed(M + N)
            dy = torch.randn(M, N, generator=gen).to(dev)
            dst = torch.empty_like(dy)
            paths = {"copy fp32 -> fp32": lambda: dst.copy_(dy), "pack row-major": lambda: training.pack_bf16(dy),
                     "pack row + transposed + sums": lambda: training.pack_bf16(dy, transposed=True, colsum=True)}
            moved = {"copy fp32 -> fp32": 8.0 * M * N, "pack row-major": 6.0 * M * N, "pack row + transposed + sums": 8.0 * M * N}
            for fn in paths.values():
                fn()
            times = AB.alternate(dev, paths, a.rounds, a.iters)
            for name in paths:
                med = median(times[name])
                say("%18s %22s %12.1f %12.1f %12.1f %10.1f %10.0f" % ((spec, name) + tuple(v * 1e3 for v in med) + (moved[name] / 1e6, moved[name] / (med[0] * 1e-3) / 1e9)))
            del dy, dst
            torch.cuda.empty_cache()
        return finish()

    S = AB.TrainStep(a.step_model, a.step_batch, a.step_grid, dev)
    m = S.m
    first = dict(activation="hip", depthwise="hip", attention="hip", modulation="hip")
    others = ", the other four training switches on \"hip\""
    what = S.what + others
    if a.part == "trace-step":
        AB.trace_step(say, S, "gemm", a.setting, a.steps, first, others)
        return finish()

    if a.part == "loss":
        m.set_training_route(**first)
        m.dropout = 0.0
        sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
        say("loss of the first %d optimizer steps on one fixed batch (ClippedAdamW lr 1e-4, dropout 0), same initial weights: %s" % (a.steps, what))
        curves = {}
        for mode in ("fp32", "bf16"):
            m.load_state_dict(sd)
            m.train()
            opt = training.ClippedAdamW(m.parameters(), lr=1e-4)
            step = S.under(m.set_training_gemm, mode)
            curves[mode] = []
            for _ in range(a.steps):
                curves[mode].append(float(step()))
                opt.step()
        say("%6s %12s %12s %12s" % ("step", "fp32", "bf16", "bf16 - fp32"))
        for i in range(a.steps):
            say("%6d %12.6f %12.6f %+12.2e" % (i, curves["fp32"][i], curves["bf16"][i], curves["bf16"][i] - curves["fp32"][i]))
        return finish()

    AB.step_ab(say, S, "gemm", a.step_rounds, first, training.LINEAR_COUNTERS, "  %s" % "linear_bf16 calls (backward calls, fallbacks to F.linear, copies)",
               lambda c: "  %d (%d, %d, %d)" % (c["calls"], c["backward"], c["fallbacks"], c["copied"]),
               "peak = max allocated during the step above weights and inputs (the op's workspaces included); held = allocated between the forward and the backward above "
               "weights and inputs (what autograd keeps); the losses differ: each step draws its own dropout masks, and the bf16 setting rounds the GEMM operands", others)
    finish()


if __name__ == "__main__":
    main()
