"""What the A/B tools of the training ops (bench_head_loss.py, bench_train_activation.py, bench_train_dwconv.py) do the same way: the report that is printed and
kept for --out, the timing of paths that take turns, peak memory of one pass, and the set-up of one training step of a bench.py model.  torch is imported on use:
the parts of the tools that only read traces need no device."""
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
