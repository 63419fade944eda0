"""What confidence-ordered renoise costs a `RequestStream` per tick, by the method of tools/truncated_sampling_ab.py: the bench.py 570M-class model, 32x32 tokens, CFG,
a FULL stream (all B slots busy, 8 steps each, ticks back to back, no decode), the configurations measured in ONE process, round-robin (a round of each in turn),
so that drift of the card lands on all of them alike:

    plain    RequestStream(): the fused head + tail, no logits tensor                                                          (b; with --tree PARENT: a)
    off      RequestStream(filtering=True), every filter off: logits forward + filtered stream tail                           (c)
    random   RequestStream(confidence=True), every request renoise="random": logits forward + statistics tail + renoise stage  (d)
    conf     every request renoise="confidence", confidence_noise=0                                                            (e)
    conf_g   every request renoise="confidence", confidence_noise=4.5                                                          (f)

    python tools/confidence_renoise_ab.py [--tree DIR] [--configs plain off random conf conf_g] [--batches 1 32] [--rounds 6]

--tree DIR imports paella_amd and bench from another checkout (the parent commit, built there; it has no confidence=True, so --configs plain or plain off only): its
`plain` against this tree's `plain` is expected to show no difference beyond the parent's own run-to-run spread -- no existing kernel, kernarg or launch changes.
Run every process twice, and alternate which tree's process goes first.  random / conf / conf_g are to be judged against `off`, which already pays for the
materialised logits: the difference is the statistics (two sums the row loop forms anyway, two stores) and the selection launch -- one workgroup per sample, about
48 workgroup reductions.  No figure is promised in advance.  Recorded: profiles/confidence_renoise_ab.txt.
"""
import argparse
import os
import sys
import time

CONFIGS = ["plain", "off", "random", "conf", "conf_g"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--configs", nargs="+", default=CONFIGS, choices=CONFIGS)
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
        sys.exit("confidence_renoise_ab.py needs a HIP device: nothing is timed without one")
    dev = torch.device("cuda", 0)
    cfg = bench.MODELS[a.model]
    m = paella_amd.Paella(**cfg)
    synth.randomize_(m, seed=0)
    m = m.to(dev)
    mk = lambda n, seed: synth.synth_conditioning(n, 0, cfg["byt5_embd"], cfg["clip_embd"], seed=seed, device=dev)
    H, steps = a.grid, 8
    stream_kw = {"plain": {}, "off": {"filtering": True}, "random": {"confidence": True}, "conf": {"confidence": True}, "conf_g": {"confidence": True}}
    admit_kw = {"plain": {}, "off": {}, "random": {"renoise": "random"}, "conf": {"renoise": "confidence"}, "conf_g": {"renoise": "confidence", "confidence_noise": 4.5}}
    print("tree %s (paella_amd from %s), configurations %s, model %s, %dx%d tokens, CFG, %d-step requests, every slot busy; kernel sources %s"
          % (os.path.abspath(a.tree), os.path.dirname(paella_amd.__file__), a.configs, a.model, H, H, steps, bench.source_stamp()), flush=True)
    print("%6s %8s %14s %14s %14s   (ms per tick: a round = %d back-to-back graph replays between two synchronisations; %d rounds per configuration after one "
          "warm-up round, the configurations taking turns)" % ("batch", "config", "median", "min", "max", steps, a.rounds))
    for B in a.batches:
        streams = {c: paella_amd.RequestStream(m, mk(1, 2), mk(1, 3), (B, H, H), max_steps=steps, device=dev, **stream_kw[c]) for c in a.configs}
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
