"""One whole training iteration -- `forward_loss` + backward + clip_grad_norm_ + AdamW -- submitted two ways, on the same module in ONE process:

    eager   forward_loss + backward + ClippedAdamW.step() + zero_grad(set_to_none=True): some two thousand launches from the host
    graph   one paella_amd.training.GraphTrainStep call: the input copies, the optimizer-table upload, one graph replay

Both with all five training switches on (activation, depthwise, attention, modulation "hip", gemm "bf16"), which is the fastest eager path there is.  Every part
is one process and one GPU step; run each under its own time limit:

    timeout 600 python tools/bench_train_graph.py step [--model 570m] [--step-batch 16] [--step-grid 32] [--step-rounds 7] [--step-iters 3] [--out FILE]
    timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_train_graph.py trace --path eager|graph --steps 3
    python tools/bench_train_graph.py count DIR_EAGER DIR_GRAPH --steps 3 [--out FILE]     (no device needed: reads the traces; steps = the traces' --steps)

step: one warm-up of the eager path, its memory figures, then the capture (timed: warm-up iteration + capture), the graph's memory figures, one replay, and `rounds`
rounds in which the two paths take turns; a round is `iters` back-to-back iterations between two device synchronisations on the host clock (ms per iteration).  Reported: median (min ... max), whether
the two ranges overlap, peak memory during an iteration and memory held between iterations, both above weights, inputs and optimizer state.
trace: what `count` reads -- the kernel dispatches of `steps` iterations of one path behind a sentinel kernel (a cumsum launched after set-up and warm-up).
count: dispatches and kernel time per iteration of both traces, and every kernel name whose count per iteration differs between them.
Nothing is timed without a HIP device."""
import argparse
import os
import re
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import train_ab as AB  # noqa: E402


def behind_sentinel(directory):
    """kernel name -> (dispatches, us) of what a trace holds behind its last sentinel kernel"""
    rows = list(AB._rows(directory, "kernel_trace.csv"))
    # the cumsum's own kernel: the iteration itself holds other scans (the lookback scans of torch's sorting embedding backward)
    marks = [int(r["End_Timestamp"]) for r in rows if re.search("single_scan_kernel|tensor_kernel_scan|cumsum", r["Kernel_Name"], re.I)]
    if not marks:
        sys.exit("no sentinel kernel in %s" % directory)
    names = {}
    for r in rows:
        if int(r["Start_Timestamp"]) > max(marks):
            c, t = names.get(r["Kernel_Name"], (0, 0.0))
            names[r["Kernel_Name"]] = (c + 1, t + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return names


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["step", "trace", "count"])
    ap.add_argument("dirs", nargs="*")
    ap.add_argument("--model", default="570m")
    ap.add_argument("--step-batch", type=int, default=16)
    ap.add_argument("--step-grid", type=int, default=32)
    ap.add_argument("--step-rounds", type=int, default=7)
    ap.add_argument("--step-iters", type=int, default=3)
    ap.add_argument("--path", default="graph", choices=["eager", "graph"])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    report = AB.Report(a.out)
    say, finish, median = report.say, report.finish, AB.median

    if a.part == "count":
        if len(a.dirs) != 2:
            sys.exit("count takes the eager trace and the graph trace")
        eager, graph = (behind_sentinel(d) for d in a.dirs)
        n = float(a.steps)
        say("kernel dispatches and kernel time per iteration: the %d iterations behind each trace's sentinel" % a.steps)
        say("%-10s %12s %14s" % ("path", "dispatches", "kernel ms"))
        for name, t in (("eager", eager), ("graph", graph)):
            say("%-10s %12.1f %14.3f" % (name, sum(c for c, _ in t.values()) / n, sum(us for _, us in t.values()) / n / 1e3))
        say("kernel names whose dispatches per iteration differ (eager -> graph):")
        same = 0
        for k in sorted(set(eager) | set(graph)):
            ce, cg = eager.get(k, (0, 0.0))[0] / n, graph.get(k, (0, 0.0))[0] / n
            if ce != cg:
                say("%10.1f -> %-10.1f %s" % (ce, cg, AB._short(k, 140)))
            else:
                same += 1
        say("%d kernel names with the same count on both sides" % same)
        return finish()

    import torch

    from paella_amd import training
    if not torch.cuda.is_available():
        sys.exit("bench_train_graph.py needs a HIP device: nothing is timed without one")
    dev = torch.device("cuda", 0)
    S = AB.TrainStep(a.model, a.step_batch, a.step_grid, dev)
    m = S.m
    m.set_training_route(activation="hip", depthwise="hip", attention="hip", modulation="hip", gemm="bf16")
    opt = training.ClippedAdamW(m.parameters(), lr=1e-6)
    opt.materialize_state()
    fwd_bwd = S.under(lambda mode: None, None)      # zero_grad(set_to_none=True) first, then forward_loss + backward of the weighted mean

    def eager():
        loss = fwd_bwd()
        opt.step()
        return loss

    inputs = dict(noised=S.noised, t=S.t, latents=S.latents, loss_weight=S.lw, **S.cond)
    call = dict(noised=S.noised, t=S.t, latents=S.latents, loss_weight=S.lw)

    if a.part == "trace":
        if a.path == "eager":
            run = eager
            run()
        else:
            step = training.GraphTrainStep(m, opt, inputs, seed=1)
            run = lambda: step(**call)
            run()
        torch.cuda.synchronize(dev)
        torch.cumsum(torch.ones(64, device=dev), 0)   # the sentinel `count` looks for: what follows it in the trace is the traced iterations alone
        torch.cuda.synchronize(dev)
        for _ in range(a.steps):
            run()
        torch.cuda.synchronize(dev)
        say("traced %d iterations of path %s behind the sentinel: %s" % (a.steps, a.path, S.what))
        return finish()

    mib = lambda b: b / 2 ** 20
    eager()                                           # warm-up: allocator pools, library selections, the timestep-frequency table
    m.zero_grad(set_to_none=True)
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated(dev)           # weights, inputs, optimizer state and its table
    torch.cuda.reset_peak_memory_stats(dev)
    eager()
    torch.cuda.synchronize(dev)
    eager_peak = torch.cuda.max_memory_allocated(dev) - base
    m.zero_grad(set_to_none=True)
    eager_held = torch.cuda.memory_allocated(dev) - base
    torch.cuda.synchronize(dev)
    torch.cuda.empty_cache()
    eager_reserved = torch.cuda.memory_reserved(dev)
    t0 = time.perf_counter()
    step = training.GraphTrainStep(m, opt, inputs, seed=1)
    torch.cuda.synchronize(dev)
    capture_s = time.perf_counter() - t0
    torch.cuda.empty_cache()
    graph_held = torch.cuda.memory_allocated(dev) - base
    graph_reserved = torch.cuda.memory_reserved(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    step(**call)
    torch.cuda.synchronize(dev)
    graph_peak = torch.cuda.max_memory_allocated(dev) - base
    paths = {"eager": eager, "graph": lambda: step(**call)}
    times = AB.alternate(dev, paths, a.step_rounds, a.step_iters)
    say("one training iteration (forward_loss + backward + clip_grad_norm_(1.0) + AdamW), %s, all five training switches on (gemm \"bf16\"); %d rounds of %d back-to-back "
        "iterations per path after warm-up, paths alternating, host clock between device synchronisations, ms per iteration" % (S.what, a.step_rounds, a.step_iters))
    say("eager = forward_loss + backward + ClippedAdamW.step() + zero_grad(set_to_none=True); graph = one GraphTrainStep call (%d drawing sites, captures %d)"
        % (training.dropout_sites(m), step.captures))
    say("peak / held = allocated by torch during one iteration / between two iterations, above weights, inputs and optimizer state (%.1f MiB); reserved = what the "
        "caching allocator holds from the device in all, after empty_cache() -- the graph keeps its pool, the eager side returns its blocks" % mib(base))
    say("%8s %12s %12s %12s %12s %12s %14s" % ("path", "median ms", "min ms", "max ms", "peak MiB", "held MiB", "reserved MiB"))
    say("%8s %12.2f %12.2f %12.2f %12.1f %12.1f %14.1f" % (("eager",) + median(times["eager"]) + (mib(eager_peak), mib(eager_held), mib(eager_reserved))))
    say("%8s %12.2f %12.2f %12.2f %12.1f %12.1f %14.1f" % (("graph",) + median(times["graph"]) + (mib(graph_peak), mib(graph_held), mib(graph_reserved))))
    (me, lo_e, hi_e), (mg, lo_g, hi_g) = median(times["eager"]), median(times["graph"])
    say("graph - eager at the median: %+.2f ms (%+.1f %%); the ranges %s" % (mg - me, 100.0 * (mg - me) / me, "do not overlap" if hi_g < lo_e or hi_e < lo_g else "OVERLAP"))
    say("construction of the GraphTrainStep (materialize_state, one warm-up iteration, the capture): %.2f s" % capture_s)
    finish()


if __name__ == "__main__":
    main()
