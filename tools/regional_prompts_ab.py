"""What regional prompts cost a `RequestStream` per tick, by the method of tools/request_prompt_weights_ab.py: the bench.py 570M-class model, 32x32 tokens, CFG, a
FULL stream (all B slots busy, 8 steps each, ticks back to back, no decode) with ragged slots of 64 rows and base prompts of 16 ByT5 + clip rows, in three
configurations measured in ONE process, round-robin (a round of configuration 0, one of 1, one of 2, again from 0), so that drift of the card lands on all alike:

    plain       RequestStream(max_cond_rows=64): the unmasked attention kernels, exactly what the stream ran before regional prompts existed
    unregional  RequestStream(max_cond_rows=64, max_regions=2), every request admitted with regions=None: the masked kernels with everything visible
    regional    the same stream, every request with two half-image regions (left / right) of 16 ByT5 + clip rows each: 60 conditioning rows, 40 of them masked

    python tools/regional_prompts_ab.py [--tree DIR] [--configs plain unregional regional] [--batches 1 32] [--rounds 6]

--tree DIR imports paella_amd and bench from another checkout (the parent commit, built there; it has no max_regions, so --configs plain only): its `plain`
against this tree's `plain` shows whether anything that existed got slower.  Run every process twice, the parent's once first and once second in its pair: the
run-to-run spread is the margin.  Recorded: profiles/regional_prompts_ab.txt.
"""
import argparse
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--configs", nargs="+", default=["plain", "unregional", "regional"], choices=["plain", "unregional", "regional"])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 32])
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
        sys.exit("regional_prompts_ab.py needs a HIP device: nothing is timed without one")
    dev = torch.device("cuda", 0)
    cfg = bench.MODELS[a.model]
    m = paella_amd.Paella(**cfg)
    synth.randomize_(m, seed=0)
    m = m.to(dev)
    mk = lambda seed: synth.synth_conditioning(1, 16, cfg["byt5_embd"], cfg["clip_embd"], seed=seed, device=dev)   # 16 ByT5 + clip rows
    H, steps, rows = a.grid, 8, 64
    left = torch.zeros(H, H, dtype=torch.bool)
    left[:, : H // 2] = True
    print("tree %s (paella_amd from %s), configurations %s, model %s, %dx%d tokens, CFG, slots of %d rows, %d-step requests, every slot busy; kernel sources %s"
          % (os.path.abspath(a.tree), os.path.dirname(paella_amd.__file__), a.configs, a.model, H, H, rows, steps, bench.source_stamp()), flush=True)
    print("%6s %11s %14s %14s %14s   (ms per tick: a round = %d back-to-back graph replays between two synchronisations; %d rounds per configuration after one "
          "warm-up round, the configurations taking turns)" % ("batch", "config", "median", "min", "max", steps, a.rounds))
    for B in a.batches:
        build = {"plain": {}, "unregional": {"max_regions": 2}, "regional": {"max_regions": 2}}
        streams = {c: paella_amd.RequestStream(m, mk(2), mk(3), (B, H, H), max_steps=steps, device=dev, max_cond_rows=rows, **build[c]) for c in a.configs}
        reqs = [dict(model_inputs=mk(100 + 4 * b), unconditional_inputs=mk(101 + 4 * b)) for b in range(min(B, 16))]
        regions = [[(mk(102 + 4 * b), left), (mk(103 + 4 * b), ~left)] for b in range(min(B, 16))]
        per_tick = {c: [] for c in a.configs}
        for i in range(a.rounds + 1):
            for c in a.configs:
                st = streams[c]
                for b in range(B):
                    st.admit(seed=1000 * (b + 1) + i, steps=steps, **reqs[b % len(reqs)], **({"regions": regions[b % len(regions)]} if c == "regional" else {}))
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
            print("%6d %11s %14.4f %14.4f %14.4f" % (B, c, v[len(v) // 2], v[0], v[-1]), flush=True)
        del streams
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
