"""The other half of a training iteration -- `clip_grad_norm_(params, 1.0); optimizer.step()` with AdamW (reference src/train.py:66-69) -- three ways, on the same
seeded tensors in ONE process:

    foreach   nn.utils.clip_grad_norm_ + torch.optim.AdamW as constructed by default (torch's multi-tensor implementation)
    fused     the same with torch.optim.AdamW(fused=True)
    hip       paella_amd.training.ClippedAdamW (paella_amd/csrc/optim.hip: three launches, the gradients read twice, p / m / v read and written once)

Every part is one process and one GPU step; run each under its own time limit:

    timeout 300 python tools/bench_train_optimizer.py update [--model 570m] [--rounds 7] [--iters 3] [--out FILE]
    timeout 300 python tools/bench_train_optimizer.py step   [--model 570m] [--step-batch 16] [--step-grid 32] [--step-rounds 5] [--out FILE]
    timeout 300 rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_train_optimizer.py trace-update --path hip --steps 3
    python tools/bench_train_optimizer.py count DIR [DIR ...] --steps 3 [--out FILE]      (no device needed: reads the traces; steps = the traces' --steps)

update: tensors with the shapes of the model's parameters (the model itself is freed), one set of seeded gradients that the three paths share, each path with its
own parameters and state; one warm-up update of each path (it creates the state; the torch paths clip the shared gradients in place, after which every path sees a
norm of about 1), then `rounds` rounds in which the paths take turns; a round is `iters` back-to-back updates between two device synchronisations on the host clock.
Reported: median (min, max) per update, the peak memory of one update above parameters, gradients and state, and for `hip` the effective bandwidth 8 passes x
bytes / time next to the 6.29 TB/s a float4 copy reaches on the chip.
step: the whole iteration, `forward_loss` + backward + update, with all four training switches on "hip", for foreach against hip (two optimizers with their own
state over the same module, taking turns).
trace-update: what `count` reads -- kernel dispatches and kernel time per update of one path.
Nothing is timed without a HIP device."""
import argparse
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import train_ab as AB  # noqa: E402

COPY_TBS = 6.29   # MI355X, float4 copy, measured (the microarchitecture guide's figure)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["update", "step", "trace-update", "count"])
    ap.add_argument("dirs", nargs="*")
    ap.add_argument("--model", default="570m")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--step-batch", type=int, default=16)
    ap.add_argument("--step-grid", type=int, default=32)
    ap.add_argument("--step-rounds", type=int, default=5)
    ap.add_argument("--path", default="hip", choices=["foreach", "fused", "hip"])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    report = AB.Report(a.out)
    say, finish, median = report.say, report.finish, AB.median

    if a.part == "count":
        say("kernel dispatches and kernel time per update: the %d updates behind the trace's sentinel (a cumsum launched after set-up and warm-up)" % a.steps)
        say("%-40s %12s %14s  %s" % ("trace", "dispatches", "kernel ms", "kernels by time"))
        for d in a.dirs:
            rows = list(AB._rows(d, "kernel_trace.csv"))
            marks = [int(r["End_Timestamp"]) for r in rows if re.search("scan|cumsum", r["Kernel_Name"], re.I)]
            if not marks:
                sys.exit("no sentinel kernel in %s" % d)
            names = {}
            for r in rows:
                if int(r["Start_Timestamp"]) > max(marks):
                    c, t = names.get(r["Kernel_Name"], (0, 0.0))
                    names[r["Kernel_Name"]] = (c + 1, t + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
            top = sorted(names.items(), key=lambda kv: -kv[1][1])[:4]
            say("%-40s %12.1f %14.3f  %s" % (os.path.basename(os.path.normpath(d)), sum(c for c, _ in names.values()) / a.steps,
                                             sum(t for _, t in names.values()) / a.steps / 1e3,
                                             "; ".join("%s x%.0f %.2f ms" % (AB._short(k, 48), c / a.steps, t / a.steps / 1e3) for k, (c, t) in top)))
        return finish()

    import torch
    from torch import nn

    import bench
    import paella_amd
    from paella_amd import training
    if not torch.cuda.is_available():
        sys.exit("bench_train_optimizer.py needs a HIP device: nothing is timed without one")
    dev = torch.device("cuda", 0)

    def torch_update(params, opt):
        def fn():
            nn.utils.clip_grad_norm_(params, 1.0)
            opt.step()
        return fn

    if a.part in ("update", "trace-update"):
        shapes = [tuple(p.shape) for p in paella_amd.Paella(**bench.MODELS[a.model]).parameters()]
        n = sum(int(torch.Size(s).numel()) for s in shapes)
        gen = torch.Generator(device=dev).manual_seed(3)
        grads = [torch.randn(s, generator=gen, device=dev) * 0.01 for s in shapes]
        wanted = ("foreach", "fused", "hip") if a.part == "update" else (a.path,)
        paths = {}
        for name in wanted:
            params = [nn.Parameter(torch.randn(s, generator=gen, device=dev) * 0.02) for s in shapes]
            for p, g in zip(params, grads):
                p.grad = g
            if name == "hip":
                paths[name] = training.ClippedAdamW(params, lr=1e-4).step
            else:
                paths[name] = torch_update(params, torch.optim.AdamW(params, lr=1e-4, **({"fused": True} if name == "fused" else {})))
        what = "model %s: %d tensors, %.1fM fp32 parameters (%.2f GB per pass)" % (a.model, len(shapes), n / 1e6, n * 4 / 1e9)
        for fn in paths.values():   # warm-up: creates the state
            fn()
        torch.cuda.synchronize(dev)
        if a.part == "trace-update":
            torch.cumsum(torch.ones(64, device=dev), 0)   # the sentinel `count` looks for: what follows it in the trace is the timed updates alone
            torch.cuda.synchronize(dev)
            for _ in range(a.steps):
                paths[a.path]()
            torch.cuda.synchronize(dev)
            say("traced %d + 1 updates of path %s: %s" % (a.steps, a.path, what))
            return finish()
        say("clip_grad_norm_(1.0) + AdamW update, %s; %d rounds of %d updates per path after one warm-up update, paths alternating" % (what, a.rounds, a.iters))
        peak = {name: AB.peak_of(dev, fn) for name, fn in paths.items()}
        times = AB.alternate(dev, paths, a.rounds, a.iters)
        say("peak = max allocated during one update above parameters, gradients and optimizer state")
        say("%10s %12s %12s %12s %12s" % ("path", "median ms", "min ms", "max ms", "peak MiB"))
        for name in paths:
            say("%10s %12.3f %12.3f %12.3f %12.1f" % ((name,) + median(times[name]) + (peak[name] / 2 ** 20,)))
        med, lo, hi = median(times["hip"])
        tb = lambda ms: 8 * n * 4 / (ms * 1e-3) / 1e12
        say("hip: 8 passes x %.2f GB / time = %.2f TB/s at the median (%.2f ... %.2f over the rounds), %.0f %% of the %.2f TB/s of a float4 copy; the time includes the "
            "finalize launch and the host's table upload" % (n * 4 / 1e9, tb(med), tb(hi), tb(lo), 100 * tb(med) / COPY_TBS, COPY_TBS))
        say("waits for a staging buffer: %d in %d updates" % (training.ADAMW_COUNTERS["staging_waits"], training.ADAMW_COUNTERS["steps"]))
        return finish()

    S = AB.TrainStep(a.model, a.step_batch, a.step_grid, dev)
    m = S.m
    m.set_training_route(activation="hip", depthwise="hip", attention="hip", modulation="hip")
    params = list(m.parameters())
    fwd_bwd = S.under(lambda mode: None, None)
    updates = {"foreach": torch_update(params, torch.optim.AdamW(params, lr=1e-6)), "hip": training.ClippedAdamW(params, lr=1e-6).step}

    def iteration(update):
        def fn():
            loss = fwd_bwd()
            update()
            return loss
        return fn

    paths = {name: iteration(u) for name, u in updates.items()}
    paths["no update"] = fwd_bwd
    say("one training iteration (forward_loss + backward + clip_grad_norm_(1.0) + AdamW), %s, all four training switches on \"hip\"; %d rounds of 1 iteration per path "
        "after one warm-up, paths alternating" % (S.what, a.step_rounds))
    for fn in paths.values():
        fn()
    times = AB.alternate(dev, paths, a.step_rounds, 1)
    say("%10s %12s %12s %12s" % ("update", "median ms", "min ms", "max ms"))
    for name in paths:
        say("%10s %12.2f %12.2f %12.2f" % ((name,) + median(times[name])))
    finish()


if __name__ == "__main__":
    main()
