"""Same-process A/B: what a batch of independent requests costs against a batch of one request replicated.

Times `GraphRequestSampler` (per-request seed, guidance and temperature from device tables) against `GraphSampler` (one seed, scalar guidance and
temperature) on the SAME tree: the bench.py 570M-class model and VQGAN, 32x32 tokens, 8 steps, CFG, with decode, as captured graphs, at batch 1 / 32 /
128, heterogeneous request settings, alternating timed replays after a warm-up.  Prints one table; the per-batch ratio is request / scalar time.

    python tools/request_batch_ab.py [--batches 1 32 128] [--replays 3] [--model 570m]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 32, 128])
    ap.add_argument("--replays", type=int, default=3, help="timed replays per sampler and batch (>= 3), alternating")
    ap.add_argument("--model", default="570m", choices=["570m", "tiny"])
    ap.add_argument("--grid", type=int, default=32)
    ap.add_argument("--sample-steps", type=int, default=8)
    a = ap.parse_args()
    import torch

    import bench
    import paella_amd
    from paella_amd import synth
    if not torch.cuda.is_available():
        sys.exit("request_batch_ab.py needs a HIP device: nothing is timed without one")
    dev = torch.device("cuda", 0)
    m = paella_amd.Paella(**bench.MODELS[a.model])
    synth.randomize_(m, seed=0)
    m = m.to(dev)
    vq = paella_amd.VQModel(**bench.VQ[a.model])
    synth.randomize_(vq, seed=0)
    vq = vq.to(dev)
    mk = lambda n, seed: synth.synth_conditioning(n, 0, bench.MODELS[a.model]["byt5_embd"], bench.MODELS[a.model]["clip_embd"], seed=seed, device=dev)
    kw = dict(steps=a.sample_steps, renoise_steps=a.sample_steps - 1, device=dev, vqgan=vq)
    print("model %s, %dx%d tokens, %d steps, CFG, VQGAN decode, hip-graph replays; kernel sources %s" % (a.model, a.grid, a.grid, a.sample_steps, bench.source_stamp()))
    print("%6s %14s %14s %14s %14s %8s" % ("batch", "scalar ms", "request ms", "scalar img/s", "request img/s", "ratio"))
    for B in a.batches:
        c, u = mk(B, 2), mk(B, 3)
        shape = (B, a.grid, a.grid)
        gs = paella_amd.GraphSampler(m, c, u, shape, temperature=(1.0, 0.2), cfg=8.0, **kw)
        gr = paella_amd.GraphRequestSampler(m, c, u, shape, temperature=(1.0, 0.2), cfg=8.0, **kw)
        # heterogeneous requests: guidance 2 .. 9.5 (every fourth one a schedule), temperature ranges that differ per request
        cfgs = [((9.0, 5.0) if b % 4 == 3 else 2.0 + 7.5 * b / max(B - 1, 1)) for b in range(B)]
        temps = [(1.0 - 0.3 * (b % 3) / 2, 0.2 + 0.1 * (b % 4)) for b in range(B)]
        run_s = lambda i: gs(seed=1000 + i)
        run_r = lambda i: gr([1000 * (b + 1) + i for b in range(B)], cfg=cfgs, temperature=temps)
        for i in range(2):  # warm-up of both graphs
            run_s(i), run_r(i)
        torch.cuda.synchronize(dev)
        ts, tr = [], []
        for i in range(max(a.replays, 3)):
            for run, acc in ((run_s, ts), (run_r, tr)):
                t0 = time.perf_counter()
                run(10 + i)
                torch.cuda.synchronize(dev)
                acc.append(time.perf_counter() - t0)
        assert gs.captures == 1 and gr.captures == 1
        s, r = sum(ts) / len(ts), sum(tr) / len(tr)
        print("%6d %14.2f %14.2f %14.2f %14.2f %8.4f   (min scalar %.2f, min request %.2f ms)" % (B, s * 1e3, r * 1e3, B / s, B / r, r / s, min(ts) * 1e3, min(tr) * 1e3), flush=True)
        del gs, gr
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
