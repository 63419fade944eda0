"""What `RequestStream(editing=True)` costs per tick when every slot holds a plain (text-to-image) request, by the method of tools/request_stream_ab.py part b:
the bench.py 570M-class model, 32x32 tokens, CFG, a FULL stream (all B slots busy, 8 steps each, ticks back to back, no decode).

    python tools/request_edit_ab.py [--tree DIR] [--editing 0|1] [--batches 1 32 128] [--rounds 6]

--tree DIR imports paella_amd and bench from another checkout (the parent commit, built there; it has no `editing` argument, so only --editing 0 runs on it).
One process measures one (tree, editing) pair; run the pairs alternately in one session and the parent twice: its run-to-run spread is the margin.
Recorded: profiles/request_stream_editing_ab.txt.
"""
import argparse
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--editing", type=int, default=0, choices=[0, 1])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 32, 128])
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--model", default="570m", choices=["570m", "tiny"])
    ap.add_argument("--grid", type=int, default=32)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch

    import bench
    import paella_amd
    from paella_amd import synth
    if not torch.cuda.is_available():
        sys.exit("request_edit_ab.py needs a HIP device: nothing is timed without one")
    dev = torch.device("cuda", 0)
    cfg = bench.MODELS[a.model]
    m = paella_amd.Paella(**cfg)
    synth.randomize_(m, seed=0)
    m = m.to(dev)
    mk = lambda n, seed: synth.synth_conditioning(n, 0, cfg["byt5_embd"], cfg["clip_embd"], seed=seed, device=dev)
    H, steps = a.grid, 8
    print("tree %s (paella_amd from %s), editing=%d, model %s, %dx%d tokens, CFG, %d-step requests, every slot busy; kernel sources %s"
          % (os.path.abspath(a.tree), os.path.dirname(paella_amd.__file__), a.editing, a.model, H, H, steps, bench.source_stamp()), flush=True)
    print("%6s %14s %14s %14s   (ms per tick: a round = %d back-to-back graph replays between two synchronisations; %d rounds after one warm-up round)"
          % ("batch", "median", "min", "max", steps, a.rounds))
    for B in a.batches:
        st = paella_amd.RequestStream(m, mk(1, 2), mk(1, 3), (B, H, H), max_steps=steps, device=dev, **({"editing": True} if a.editing else {}))
        reqs = [dict(model_inputs=mk(1, 100 + 2 * b), unconditional_inputs=mk(1, 101 + 2 * b)) for b in range(min(B, 16))]
        per_tick = []
        for i in range(a.rounds + 1):
            for b in range(B):
                st.admit(seed=1000 * (b + 1) + i, steps=steps, **reqs[b % len(reqs)])
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            done = []
            for _ in range(steps):
                done += st.tick()
            torch.cuda.synchronize(dev)
            t = time.perf_counter() - t0
            assert sorted(done) == list(range(B))
            for b in done:
                st.result(b)
            if i:
                per_tick.append(t * 1e3 / steps)
        assert st.captures == 1
        per_tick.sort()
        print("%6d %14.4f %14.4f %14.4f" % (B, per_tick[len(per_tick) // 2], per_tick[0], per_tick[-1]), flush=True)
        del st
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
