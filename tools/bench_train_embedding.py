"""The training token stem (paella_amd/csrc/embed_train.hip, Paella.set_training_embedding) measured three ways, every part one process and one GPU step; run each
under its own time limit:

    timeout 600 python tools/bench_train_embedding.py step [--model 570m] [--step-batch 16] [--step-grid 32] [--step-rounds 7] [--step-iters 3] [--out FILE]
    timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_train_embedding.py trace --path eager|graph --embedding torch|hip --steps 3
    python tools/bench_train_embedding.py count DIR_OFF DIR_ON --steps 3 [--out FILE]      (no device needed: reads two traces of ONE path, switch off and on)
    timeout 600 python tools/bench_train_embedding.py op [--step-batch 16] [--step-grid 32] [--out FILE]

step: one whole training iteration (forward_loss + backward + clip_grad_norm_ + AdamW) on ONE module with the other five training switches on, four paths taking
turns: eager and one `GraphTrainStep` call, each with the embedding switch off ("torch") and on ("hip").  The two captured steps live side by side; the switch is
set to what a step was captured under before it is called, so neither goes stale.  A round is `iters` back-to-back iterations between two device synchronisations
on the host clock; reported: median (min ... max) per path and whether the ranges of a pair overlap.
trace: the kernel dispatches of `steps` iterations of one path under one setting behind a sentinel kernel (tools/bench_train_graph.py's).
count: dispatches and kernel time per iteration of both traces, the kernel names whose count differs, and the time of the rows that belong to the embedding.
op: the backward alone at c_in 256 and 8192 labels -- `token_embed_layernorm`'s against torch's F.embedding backward on the same tokens, uniform tokens and
all-equal tokens (the op's known worst case: one workgroup does every addition).
Nothing is timed without a HIP device."""
import argparse
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import train_ab as AB  # noqa: E402
from bench_train_graph import behind_sentinel  # noqa: E402

# the rows of a trace that are the token embedding's: the new op, torch's lookups and both forms of its backward with what the sorting form launches
EMBEDDING_ROWS = ("embed_ln_train|embed_ln_unshuffle|embedding_backward|vectorized_gather_kernel|compute_grad_weight|compute_num_of_partial_segments|"
                  "krn_partial|sum_and_scatter|rocprim|arange_cuda")
OTHER_FIVE = dict(activation="hip", depthwise="hip", attention="hip", modulation="hip", gemm="bf16")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("part", choices=["step", "trace", "count", "op"])
    ap.add_argument("dirs", nargs="*")
    ap.add_argument("--model", default="570m")
    ap.add_argument("--step-batch", type=int, default=16)
    ap.add_argument("--step-grid", type=int, default=32)
    ap.add_argument("--step-rounds", type=int, default=7)
    ap.add_argument("--step-iters", type=int, default=3)
    ap.add_argument("--path", default="graph", choices=["eager", "graph"])
    ap.add_argument("--embedding", default="hip", choices=["torch", "hip"])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    report = AB.Report(a.out)
    say, finish, median = report.say, report.finish, AB.median

    if a.part == "count":
        if len(a.dirs) != 2:
            sys.exit("count takes the trace with the switch off and the trace with it on")
        off, on = (behind_sentinel(d) for d in a.dirs)
        n = float(a.steps)
        say("kernel dispatches and kernel time per iteration, embedding switch off -> on: the %d iterations behind each trace's sentinel" % a.steps)
        say("%-10s %12s %14s %22s" % ("embedding", "dispatches", "kernel ms", "embedding rows ms"))
        for name, t in (("torch", off), ("hip", on)):
            mine = sum(us for k, (_, us) in t.items() if re.search(EMBEDDING_ROWS, k))
            say("%-10s %12.1f %14.3f %22.3f" % (name, sum(c for c, _ in t.values()) / n, sum(us for _, us in t.values()) / n / 1e3, mine / n / 1e3))
        say("kernel names whose dispatches per iteration differ, or that belong to the embedding (off -> on; us per iteration):")
        for k in sorted(set(off) | set(on)):
            (c0, t0), (c1, t1) = off.get(k, (0, 0.0)), on.get(k, (0, 0.0))
            if c0 != c1 or re.search(EMBEDDING_ROWS, k):
                say("%8.1f -> %-8.1f %10.1f -> %-10.1f %s" % (c0 / n, c1 / n, t0 / n, t1 / n, AB._short(k, 120)))
        return finish()

    import torch
    import torch.nn.functional as F

    from paella_amd import training
    if not torch.cuda.is_available():
        sys.exit("bench_train_embedding.py needs a HIP device: nothing is timed without one")
    dev = torch.device("cuda", 0)

    if a.part == "op":
        B, G, C, L, p = a.step_batch, a.step_grid, 256, 8192, 2
        gen = torch.Generator().manual_seed(11)
        w = torch.randn(L, C, generator=gen).to(dev).requires_grad_()
        d_rows = torch.randn(B, G // p, G // p, C * p * p, generator=gen).to(dev)
        g = torch.randn(B, G, G, C, generator=gen).to(dev)
        say("the backward of the token embedding alone, %d x %dx%d tokens, c_in %d, %d labels, patch %d; %d rounds of %d back-to-back calls per path, paths alternating, "
            "host clock between device synchronisations, ms per call.  hip = the backward of token_embed_layernorm (LayerNorm backward included); torch = the backward of "
            "F.embedding alone on the same tokens (%s form)" % (B, G, G, C, L, p, a.step_rounds, a.step_iters, "one-kernel" if B * G * G <= 3072 else "sorting"))
        say("%10s %8s %12s %12s %12s" % ("tokens", "path", "median ms", "min ms", "max ms"))
        for kind in ("uniform", "all-equal"):
            x = (torch.randint(0, L, (B, G, G), generator=gen) if kind == "uniform" else torch.full((B, G, G), 4097, dtype=torch.int64)).to(dev)
            rows, looked = training.token_embed_layernorm(x, w, p), F.embedding(x, w)

            def hip():
                w.grad = None
                rows.backward(d_rows, retain_graph=True)

            def tor():
                w.grad = None
                looked.backward(g, retain_graph=True)

            paths = {"hip": hip, "torch": tor}
            for fn in paths.values():
                fn()
            times = AB.alternate(dev, paths, a.step_rounds, a.step_iters)
            for name in paths:
                say("%10s %8s %12.3f %12.3f %12.3f" % ((kind, name) + median(times[name])))
        return finish()

    S = AB.TrainStep(a.model, a.step_batch, a.step_grid, dev)
    m = S.m
    m.set_training_route(**OTHER_FIVE)
    opt = training.ClippedAdamW(m.parameters(), lr=1e-6)
    opt.materialize_state()
    inputs = dict(noised=S.noised, t=S.t, latents=S.latents, loss_weight=S.lw, **S.cond)
    call = dict(noised=S.noised, t=S.t, latents=S.latents, loss_weight=S.lw)

    def eager_under(mode):
        step = S.under(lambda md: m.set_training_embedding(md), mode)

        def run():
            loss = step()
            opt.step()
            return loss
        return run

    def graph_under(mode):
        m.set_training_embedding(mode)
        step = steps[mode] = training.GraphTrainStep(m, opt, inputs, seed=1)

        def run():
            m.set_training_embedding(mode)      # what this step was captured under: it is never stale
            return step(**call)
        return run

    steps = {}
    if a.part == "trace":
        run = eager_under(a.embedding) if a.path == "eager" else graph_under(a.embedding)
        run()
        torch.cuda.synchronize(dev)
        torch.cumsum(torch.ones(64, device=dev), 0)   # the sentinel `count` looks for: what follows it in the trace is the traced iterations alone
        torch.cuda.synchronize(dev)
        for _ in range(a.steps):
            run()
        torch.cuda.synchronize(dev)
        say("traced %d iterations of path %s with set_training_embedding(\"%s\") behind the sentinel: %s" % (a.steps, a.path, a.embedding, S.what))
        return finish()

    paths = {"eager torch": eager_under("torch"), "eager hip": eager_under("hip")}
    for fn in paths.values():                          # warm-up: allocator pools, library selections, the timestep-frequency table
        fn()
    m.zero_grad(set_to_none=True)
    torch.cuda.synchronize(dev)
    paths["graph torch"] = graph_under("torch")
    paths["graph hip"] = graph_under("hip")
    for name in ("graph torch", "graph hip"):
        paths[name]()
    times = AB.alternate(dev, paths, a.step_rounds, a.step_iters)
    say("one training iteration (forward_loss + backward + clip_grad_norm_(1.0) + AdamW), %s, the other five training switches on (gemm \"bf16\"); %d rounds of %d "
        "back-to-back iterations per path after warm-up, the four paths alternating, host clock between device synchronisations, ms per iteration"
        % (S.what, a.step_rounds, a.step_iters))
    say("eager = forward_loss + backward + ClippedAdamW.step() + zero_grad(set_to_none=True); graph = one GraphTrainStep call; torch / hip = set_training_embedding; "
        "captures of the two steps over the whole run: %d, %d" % (steps["torch"].captures, steps["hip"].captures))
    say("%14s %12s %12s %12s" % ("path", "median ms", "min ms", "max ms"))
    stats = {name: median(v) for name, v in times.items()}
    for name in paths:
        say("%14s %12.2f %12.2f %12.2f" % ((name,) + stats[name]))

    def versus(x, y):
        (mx, lo_x, hi_x), (my, lo_y, hi_y) = stats[x], stats[y]
        say("%s - %s at the median: %+.2f ms (%+.1f %%); the ranges %s" % (x, y, mx - my, 100.0 * (mx - my) / my, "do not overlap" if hi_x < lo_y or hi_y < lo_x else "OVERLAP"))

    versus("graph hip", "graph torch")
    versus("eager hip", "eager torch")
    versus("graph hip", "eager hip")
    versus("graph hip", "eager torch")
    finish()


if __name__ == "__main__":
    main()
