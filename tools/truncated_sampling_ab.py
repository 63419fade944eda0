"""What truncated sampling costs a `RequestStream` per tick, by the method of tools/request_prompt_weights_ab.py: the bench.py 570M-class model, 32x32 tokens, CFG, a
FULL stream (all B slots busy, 8 steps each, ticks back to back, no decode), the configurations measured in ONE process, round-robin (a round of each in turn),
so that drift of the card lands on all of them alike:

    plain    RequestStream(filtering=False): the fused head + tail, no logits tensor                                 (b; with --tree PARENT: a)
    off      RequestStream(filtering=True), every request admitted with every filter off: logits forward + filtered stream tail, whose rows skip the selection (c)
    typical  every request admitted with typical_mass=0.2                                                                                     (d)
    topkp    every request admitted with top_k=64, top_p=0.9                                                                                   (e)

    python tools/truncated_sampling_ab.py [--tree DIR] [--configs plain off typical topkp] [--batches 1 32] [--rounds 6]

--tree DIR imports paella_amd and bench from another checkout (the parent commit, built there; it has no filtering, so --configs plain only): its `plain` against
this tree's `plain` is expected to show no difference beyond the parent's own run-to-run spread -- no existing kernel, kernarg or launch changes.  Run every
process twice, and one pair with the parent's process FIRST.  off / typical / topkp against plain are the price of the materialised logits (rows * L * 4 bytes
written and read back per tick) and of the selection; no figure is promised in advance.  Recorded: profiles/truncated_sampling_ab.txt.
"""
import argparse
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--configs", nargs="+", default=["plain", "off", "typical", "topkp"], choices=["plain", "off", "typical", "topkp"])
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
        sys.exit("truncated_sampling_ab.py needs a HIP device: nothing is timed without one")
    dev = torch.device("cuda", 0)
    cfg = bench.MODELS[a.model]
    m = paella_amd.Paella(**cfg)
    synth.randomize_(m, seed=0)
    m = m.to(dev)
    mk = lambda n, seed: synth.synth_conditioning(n, 0, cfg["byt5_embd"], cfg["clip_embd"], seed=seed, device=dev)
    H, steps = a.grid, 8
    admit_kw = {"plain": {}, "off": {}, "typical": {"typical_mass": 0.2}, "topkp": {"top_k": 64, "top_p": 0.9}}
    print("tree %s (paella_amd from %s), configurations %s, model %s, %dx%d tokens, CFG, %d-step requests, every slot busy; kernel sources %s"
          % (os.path.abspath(a.tree), os.path.dirname(paella_amd.__file__), a.configs, a.model, H, H, steps, bench.source_stamp()), flush=True)
    print("%6s %8s %14s %14s %14s   (ms per tick: a round = %d back-to-back graph replays between two synchronisations; %d rounds per configuration after one "
          "warm-up round, the configurations taking turns)" % ("batch", "config", "median", "min", "max", steps, a.rounds))
    for B in a.batches:
        streams = {c: paella_amd.RequestStream(m, mk(1, 2), mk(1, 3), (B, H, H), max_steps=steps, device=dev, **({} if c == "plain" else {"filtering": True}))
                   for c in a.configs}
        reqs = [dict(model_inputs=mk(1, 100 + 2 * b), unconditional_inputs=mk(1, 101 + 2 * b)) for b in range(min(B, 16))]
        per_tick = {c: [] for c in a.configs}
        for i in range(a.rounds + 1):
            for c in a.configs:
                st = streams[c]
                for b in range(B):
                    st.admit(seed=1000 * (b + 1) + i, steps=steps, **reqs[b % len(reqs)], **admit_kw[c])
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
