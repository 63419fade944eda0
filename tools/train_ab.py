"""What the A/B tools of the training ops (bench_head_loss.py, bench_train_activation.py, bench_train_dwconv.py, bench_train_attention.py, bench_train_modulation.py, bench_train_linear.py) do the same way: the report
that is printed and kept for --out, the timing of paths that take turns, peak memory of one pass, the set-up of one training step of a bench.py model, the `step` and `trace-step` parts
of a training switch's tool (the switch named as in paella_amd.training.TRAIN_SWITCHES), and the two tables read from rocprofv3 kernel traces.  torch is imported on use: the parts of the tools that only read traces need no device."""
import csv
import glob
import os
import re
import sys
import time


class Report:
    """say(line) prints and keeps; finish() writes what was said to `out`, if one was given"""

    def __init__(self, out=None):
        self.out, self.lines = out, []

    def say(self, s):
        print(s, flush=True)
        self.lines.append(s)

    def finish(self):
        if self.out:
            with open(self.out, "w") as f:
                f.write("\n".join(self.lines) + "\n")


def median(v):
    """(median, min, max)"""
    v = sorted(v)
    return v[len(v) // 2], v[0], v[-1]


def alternate(dev, paths, rounds, iters):
    """`rounds` rounds in which the paths {name: fn} take turns; a round is `iters` back-to-back calls between two device synchronisations, timed on the host
    clock -> {name: [ms per call, one figure per round]}"""
    import torch
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


def peak_of(dev, fn):
    """torch.cuda.max_memory_allocated over one call of fn, its result still alive, minus what was allocated before it"""
    import torch
    torch.cuda.empty_cache()
    torch.cuda.synchronize(dev)
    base = torch.cuda.memory_allocated(dev)
    torch.cuda.reset_peak_memory_stats(dev)
    out = fn()
    torch.cuda.synchronize(dev)
    peak = torch.cuda.max_memory_allocated(dev) - base
    del out
    return peak


class TrainStep:
    """One training step of bench.MODELS[model] in train mode on dev, at `batch` x `grid`^2 seeded tokens: `forward_loss` + backward of the weighted mean loss."""

    def __init__(self, model, batch, grid, dev):
        import torch

        import bench
        import paella_amd
        from paella_amd import synth
        cfg = bench.MODELS[model]
        m = paella_amd.Paella(**cfg)
        synth.randomize_(m, seed=0)
        self.m = m = m.to(dev)
        m.train()
        gen = torch.Generator().manual_seed(7)
        self.latents = torch.randint(0, cfg["num_labels"], (batch, grid, grid), generator=gen).to(dev)
        self.t = torch.rand(batch, generator=gen).to(dev)
        mask = (torch.rand(batch, grid, grid, generator=gen) < self.t.cpu()[:, None, None]).long().to(dev)
        random_x = torch.randint(0, cfg["num_labels"], (batch, grid, grid), generator=gen).to(dev)
        self.cond = synth.synth_conditioning(batch, 4, cfg["byt5_embd"], cfg["clip_embd"], seed=2, device=dev)
        self.noised = self.latents * (1 - mask) + random_x * mask
        self.lw = m.get_loss_weight(self.t, mask)
        self.dev = dev
        self.what = "model %s (%.1fM parameters), %d x %dx%d tokens, dropout %s" % (model, self.parameters() / 1e6, batch, grid, grid, m.dropout)

    def parameters(self):
        return sum(p.numel() for p in self.m.parameters())

    def under(self, switch, mode, held=None):
        """the step after switch(mode), parameter gradients freed first -> the loss; held[mode] = what autograd holds between the forward and the backward"""
        import torch

        def step():
            switch(mode)
            self.m.zero_grad(set_to_none=True)
            base = torch.cuda.memory_allocated(self.dev)
            loss, _ = self.m.forward_loss(self.noised, self.t, self.latents, **self.cond)
            loss = ((loss * self.lw).sum(dim=[1, 2]) / self.lw.sum(dim=[1, 2])).mean()
            if held is not None:
                held[mode] = torch.cuda.memory_allocated(self.dev) - base
            loss.backward()
            return loss.detach()
        return step


def _switch_of(m, name):
    from paella_amd import training
    row = next(s for s in training.TRAIN_SWITCHES if s.name == name)
    return row, lambda mode: m.set_training_route(**{name: mode})


def _first_text(first):
    return "".join(", set_training_%s(\"%s\")" % kv for kv in first.items())


def legend(S, tail=""):
    return ("peak = max allocated during the step above weights and inputs, the step's parameter gradients (%.1f MiB once all exist) included under either setting; "
            "held = allocated between the forward and the backward above weights and inputs (what autograd keeps)" % (S.parameters() * 4 / 2 ** 20)) + tail


def trace_step(say, S, name, setting, steps, first=None, first_text=None):
    """the `trace-step` part of a switch's tool: one warm-up and `steps` training steps under set_training_<name>(setting), the settings `first` turned on before"""
    import torch
    _, switch = _switch_of(S.m, name)
    S.m.set_training_route(**(first or {}))
    fn = S.under(switch, setting)
    fn()   # warm-up (traced as well: divide the totals by 1 + --steps)
    for _ in range(steps):
        fn()
    torch.cuda.synchronize(S.dev)
    say("traced %d + 1 training steps with set_training_%s(\"%s\"): %s" % (steps, name, setting, S.what + (first_text or _first_text(first or {}))))


def step_ab(say, S, name, rounds, first=None, counters=None, calls_head="", calls=None, note=None, first_text=None):
    """the `step` part of a switch's tool: one full training step under either set_training_<name> setting, the settings taking turns, the settings `first` turned on
    before.  counters: the op's counters dict -- calls(what one step added to it) formats the table's last column(s) under calls_head; note: the legend line above
    the table (`legend`).  Without counters the table is the short one of bench_train_activation.py."""
    row, switch = _switch_of(S.m, name)
    m = S.m
    m.set_training_route(**(first or {}))
    held = {}
    what = S.what + (first_text or _first_text(first or {}))
    paths = {mode: S.under(switch, mode, held) for mode in (row.off, row.on)}
    say("one training step (forward_loss + backward), %s; %d rounds of 1 step per %ssetting after one warm-up, settings alternating"
        % (what, rounds, "set_training_%s " % name if counters is not None else ""))
    losses, counts = {}, {}
    for mode, fn in paths.items():   # warm-up
        c0 = dict(counters or {})
        losses[mode] = float(fn())
        counts[mode] = {k: counters[k] - c0[k] for k in c0}
    peak = {}
    for mode, fn in paths.items():
        m.zero_grad(set_to_none=True)   # the base of EITHER setting holds no parameter gradients: the peak includes the step's own
        peak[mode] = peak_of(S.dev, fn)
    m.zero_grad(set_to_none=True)
    times = alternate(S.dev, paths, rounds, 1)
    if counters is None:
        say("%10s %12s %12s %12s %26s %12s" % ("setting", "median ms", "min ms", "max ms", "peak MiB > weights + inputs", "loss"))
        for mode in paths:
            say("%10s %12.2f %12.2f %12.2f %26.1f %12.5f" % ((mode,) + median(times[mode]) + (peak[mode] / 2 ** 20, losses[mode])))
        return
    say(note)
    say("%10s %12s %12s %12s %10s %10s %12s" % ("setting", "median ms", "min ms", "max ms", "peak MiB", "held MiB", "loss") + calls_head)
    for mode in paths:
        say("%10s %12.2f %12.2f %12.2f %10.1f %10.1f %12.5f" % ((mode,) + median(times[mode]) + (peak[mode] / 2 ** 20, held[mode] / 2 ** 20, losses[mode])) + calls(counts[mode]))


def _rows(directory, suffix):
    files = sorted(glob.glob(os.path.join(directory, "**", "*" + suffix), recursive=True))
    if not files:
        sys.exit("no *%s under %s" % (suffix, directory))
    for f in files:
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                yield r


def _short(name, n=96):
    name = re.sub(r"\s+", " ", name)
    return name if len(name) <= n else name[:n - 3] + "..."


def by_name(directory):
    """kernel name -> (calls, total us) from a rocprofv3 --kernel-trace csv"""
    out = {}
    for r in _rows(directory, "kernel_trace.csv"):
        c, t = out.get(r["Kernel_Name"], (0, 0.0))
        out[r["Kernel_Name"]] = (c + 1, t + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return out


def trace_diff(say, dir_off, dir_on, steps, switch, share=0.002, calls_too=False):
    """kernel time per step by kernel name in two traces of `steps` steps each, `switch` off -> on: the rows that move by at least `share` of the off step's kernel
    time (calls_too: or whose call count differs), then the sums"""
    off, on = by_name(dir_off), by_name(dir_on)
    n = float(steps)
    tot_off, tot_on = sum(t for _, t in off.values()) / n, sum(t for _, t in on.values()) / n
    say("kernel time per training step by kernel name, %s switch off -> on (%d steps per trace; us per step; calls per step)" % (switch, steps))
    say("%10s %8s %10s %8s %10s  %s" % ("off us", "calls", "on us", "calls", "on - off", "kernel"))
    rows = []
    for k in set(off) | set(on):
        c0, t0 = off.get(k, (0, 0.0))
        c1, t1 = on.get(k, (0, 0.0))
        rows.append((t1 / n - t0 / n, t0 / n, c0 / n, t1 / n, c1 / n, k))
    rows.sort()
    gone = sum(-r[0] for r in rows if r[0] < 0)
    came = sum(r[0] for r in rows if r[0] > 0)
    for d, t0, c0, t1, c1, k in rows:
        if abs(d) >= share * tot_off or (calls_too and c0 != c1):
            say("%10.1f %8.1f %10.1f %8.1f %+10.1f  %s" % (t0, c0, t1, c1, d, _short(k)))
    say("sum of all kernels: off %.1f us, on %.1f us per step; rows that shrank: -%.1f us (%.1f %% of the off step's kernel time), rows that grew: +%.1f us"
        % (tot_off, tot_on, gone, 100.0 * gone / tot_off, came))


def trace_kernels(say, directory, match):
    """the dispatches of a trace whose kernel name matches, grouped by kernel name and grid"""
    groups = {}
    for r in _rows(directory, "kernel_trace.csv"):
        if not re.search(match, r["Kernel_Name"]):
            continue
        wg = int(r["Workgroup_Size_X"]) * int(r["Workgroup_Size_Y"]) * int(r["Workgroup_Size_Z"])
        key = (r["Kernel_Name"], "%dx%dx%d/%d" % (int(r["Grid_Size_X"]), int(r["Grid_Size_Y"]), int(r["Grid_Size_Z"]), wg))
        groups.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    say("%-18s %6s %9s %9s %9s  %s" % ("grid (threads)/wg", "calls", "avg us", "min us", "max us", "kernel"))
    for (k, g), v in sorted(groups.items(), key=lambda kv: (kv[0][0], kv[0][1])):
        say("%-18s %6d %9.1f %9.1f %9.1f  %s" % (g, len(v), sum(v) / len(v), min(v), max(v), _short(k)))
