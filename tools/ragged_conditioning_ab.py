"""Same-process measurements around ragged conditioning (per-sample conditioning-key counts in attention; CFG on unequal layouts as one forward): the bench.py
570M-class model, 32x32 tokens, 8 steps, CFG, counter-based noise, captured graphs, no decode.

    python tools/ragged_conditioning_ab.py --part a [--tree DIR]   EQUAL layouts (CLIP text only, S = 4 on both sides: the non-ragged cache, cond_len == NULL in every
                                                                  kernel): GraphSampler images/s at batch 1 / 32 / 128.  --tree DIR imports paella_amd and bench from
                                                                  another checkout (the parent commit, built there): run both trees in one session, alternating,
                                                                  the parent three times -- its spread is the margin the null path must stay inside.
    python tools/ragged_conditioning_ab.py --part b [--tree DIR]   UNEQUAL layouts as conditioning.embed_prompts produces them: 64 ByT5 + 4 + 4 rows against 1 + 4 rows, at
                                                                  batch 1 and 32.  On the parent commit this captures the two-forward path (materialised logits, unfused
                                                                  tail), on this tree the ragged 2B-slot cache (shared prefix, guidance through the head, fused tail).
    python tools/ragged_conditioning_ab.py --part c               the same request with the unconditional side PADDED to the conditional side's 72 rows (equal layouts:
                                                                  the non-ragged batched path, every sample attends 72 conditioning keys) against the ragged cache
                                                                  (72 and 5 keys): what the per-sample loop bound saves.
Recorded: profiles/ragged_conditioning_ab.txt.
"""
import argparse
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", required=True, choices=["a", "b", "c"])
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--batches", type=int, nargs="+", default=None)
    ap.add_argument("--replays", type=int, default=3)
    ap.add_argument("--model", default="570m", choices=["570m", "tiny"])
    ap.add_argument("--grid", type=int, default=32)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch

    import bench
    import paella_amd
    from paella_amd import synth
    if not torch.cuda.is_available():
        sys.exit("ragged_conditioning_ab.py needs a HIP device: nothing is timed without one")
    dev = torch.device("cuda", 0)
    cfg = bench.MODELS[a.model]
    m = paella_amd.Paella(**cfg)
    synth.randomize_(m, seed=0)
    m = m.to(dev)
    mk = lambda n, s_byt5, n_img, seed: synth.synth_conditioning(n, s_byt5, cfg["byt5_embd"], cfg["clip_embd"], seed=seed, with_clip=True, n_clip_image=n_img, device=dev)
    H = a.grid
    print("part %s, tree %s, model %s, %dx%d tokens, 8 steps, CFG 8, philox; kernel sources %s" % (a.part, os.path.abspath(a.tree), a.model, H, H, bench.source_stamp()), flush=True)

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, out

    def measure(B, c, u):
        """(images/s over the replays, best replay in ms, forward_sample calls and forward_prepared calls of one eager pass)"""
        calls = {"sample": 0, "prepared": 0}
        fs, fp = m.forward_sample, m.forward_prepared

        def cs(*x, **k):
            calls["sample"] += 1
            return fs(*x, **k)

        def cp(*x, **k):
            calls["prepared"] += 1
            return fp(*x, **k)
        m.forward_sample, m.forward_prepared = cs, cp
        try:
            paella_amd.sample(m, c, (B, H, H), unconditional_inputs=u, steps=8, renoise_steps=7, cfg=8.0, device=dev, noise="philox", seed=1)
        finally:
            del m.forward_sample, m.forward_prepared
        gs = paella_amd.GraphSampler(m, c, u, (B, H, H), steps=8, renoise_steps=7, temperature=(1.0, 0.2), cfg=8.0, device=dev)
        for i in range(2):
            gs(seed=1000 + i)
        ts = [timed(lambda: gs(seed=10 + i))[0] for i in range(max(a.replays, 3))]
        del gs
        torch.cuda.empty_cache()
        return B * len(ts) / sum(ts), min(ts) * 1e3, calls["sample"], calls["prepared"]

    row = "%6s %28s %12s %12s %16s %18s"
    print(row % ("batch", "conditioning rows (c / u)", "images/s", "best ms", "fused forwards", "unfused forwards"), flush=True)
    show = lambda B, what, r: print(row % (B, what, "%.2f" % r[0], "%.2f" % r[1], r[2], r[3]), flush=True)
    if a.part == "a":
        for B in a.batches or [1, 32, 128]:
            show(B, "4 / 4 (equal)", measure(B, mk(B, 0, 0, 2), mk(B, 0, 0, 3)))
    elif a.part == "b":
        for B in a.batches or [1, 32]:
            show(B, "72 / 5", measure(B, mk(B, 64, 1, 2), mk(B, 1, 0, 3)))
    else:
        for B in a.batches or [1, 32]:
            c, u = mk(B, 64, 1, 2), mk(B, 1, 0, 3)
            pad = mk(B, 64, 1, 5)   # an unconditional side of the conditional side's layout: its own 5 rows are what a caller would pad with 67 more
            show(B, "72 / 72 (padded, equal)", measure(B, c, pad))
            show(B, "72 / 5 (ragged)", measure(B, c, u))


if __name__ == "__main__":
    main()
