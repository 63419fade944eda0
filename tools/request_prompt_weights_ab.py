"""What prompt weights cost a `RequestStream` per tick, by the method of tools/request_stream_ab.py part b: the bench.py 570M-class model, 32x32 tokens, CFG, a
FULL stream (all B slots busy, 8 steps each, ticks back to back, no decode), in three configurations measured in ONE process, round-robin (a round of
configuration 0, one of 1, one of 2, again from 0), so that drift of the card lands on all of them alike:

    none    no weights anywhere (key_weights == NULL in every attention launch)
    wide    RequestStream(attn_weights=w): one vector for the life of the stream, the shared-vector path
    table   RequestStream(max_attn_weights=N) with every request admitted with attn_weights=w: the per-request table, every slot weighted

    python tools/request_prompt_weights_ab.py [--tree DIR] [--configs none wide table] [--batches 1 32] [--rounds 6] [--weights 4]

--tree DIR imports paella_amd and bench from another checkout (the parent commit, built there; it has no max_attn_weights, so --configs none wide only): its
`none` against this tree's `none` shows what the extra AttnArgs fields cost when they are unused.  Run the two trees alternately in one session and one of
them twice: the run-to-run spread is the margin.  Recorded: profiles/request_prompt_weights_ab.txt.
"""
import argparse
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--configs", nargs="+", default=["none", "wide", "table"], choices=["none", "wide", "table"])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--weights", type=int, default=4, help="weights per vector: the last CLIP rows of a request")
    ap.add_argument("--model", default="570m", choices=["570m", "tiny"])
    ap.add_argument("--grid", type=int, default=32)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch

    import bench
    import paella_amd
    from paella_amd import synth
    if not torch.cuda.is_available():
        sys.exit("request_prompt_weights_ab.py needs a HIP device: nothing is timed without one")
    dev = torch.device("cuda", 0)
    cfg = bench.MODELS[a.model]
    m = paella_amd.Paella(**cfg)
    synth.randomize_(m, seed=0)
    m = m.to(dev)
    mk = lambda n, seed: synth.synth_conditioning(n, 0, cfg["byt5_embd"], cfg["clip_embd"], seed=seed, device=dev)
    H, steps = a.grid, 8
    w = (torch.rand(a.weights, generator=torch.Generator().manual_seed(5)) + 0.5).to(dev)
    print("tree %s (paella_amd from %s), configurations %s, %d weights, model %s, %dx%d tokens, CFG, %d-step requests, every slot busy; kernel sources %s"
          % (os.path.abspath(a.tree), os.path.dirname(paella_amd.__file__), a.configs, a.weights, a.model, H, H, steps, bench.source_stamp()), flush=True)
    print("%6s %8s %14s %14s %14s   (ms per tick: a round = %d back-to-back graph replays between two synchronisations; %d rounds per configuration after one "
          "warm-up round, the configurations taking turns)" % ("batch", "config", "median", "min", "max", steps, a.rounds))
    for B in a.batches:
        build = {"none": {}, "wide": {"attn_weights": w}, "table": {"max_attn_weights": max(a.weights, 1)}}
        streams = {c: paella_amd.RequestStream(m, mk(1, 2), mk(1, 3), (B, H, H), max_steps=steps, device=dev, **build[c]) for c in a.configs}
        reqs = [dict(model_inputs=mk(1, 100 + 2 * b), unconditional_inputs=mk(1, 101 + 2 * b)) for b in range(min(B, 16))]
        per_tick = {c: [] for c in a.configs}
        for i in range(a.rounds + 1):
            for c in a.configs:
                st = streams[c]
                for b in range(B):
                    st.admit(seed=1000 * (b + 1) + i, steps=steps, **reqs[b % len(reqs)], **({"attn_weights": w} if c == "table" else {}))
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
                    per_tick[c].append(t * 1e3 / steps)
        for c in a.configs:
            assert streams[c].captures == 1
            v = sorted(per_tick[c])
            print("%6d %8s %14.4f %14.4f %14.4f" % (B, c, v[len(v) // 2], v[0], v[-1]), flush=True)
        del streams
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
