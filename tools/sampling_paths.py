"""Every launch path of the sampling step (paella_amd/sampling.py), once each, on seeded UNET_TINY weights: B = 3, 8x8 tokens, 4 steps of which 3 renoise.  Prints one
line per path -- its name, a SHA-256 of the tokens it returned and, where it returns statistics maps, one of those.  Two trees compute the same tokens when their
outputs are equal line by line.

    python tools/sampling_paths.py                     the hashes
    rocprofv3 --kernel-trace -d DIR -o t --output-format csv -- python tools/sampling_paths.py --markers
    python tools/sampling_paths.py --launches DIR      per path of that trace: the number of dispatches and a SHA-256 of their ordered (kernel name, grid) list

--markers launches one erfinv kernel (an op the sampler never uses) in front of every path, which is what --launches cuts the trace by."""
import argparse
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, H, SEED = 3, 8, 7
KW = dict(steps=4, renoise_steps=3)
STREAM_STEPS = [2, 4, 3, 6, 1]  # five requests of unequal step counts through three slots


def digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def paths(dev):
    """[(name, thunk)]; a thunk returns tokens, (tokens, {"logprob", "entropy"}) or a list of token grids"""
    import torch

    import paella_amd
    from oracle import golden_configs as G
    from tests.helpers import cond_for, to_dev, weights_for
    cfg = G.UNET_TINY
    m = paella_amd.Paella(**cfg)
    weights_for(m, sum(cfg["blocks"]))
    m = m.to(dev)
    shape = (B, H, H)
    cond = lambda n, byt5, img, seed: to_dev(cond_for(cfg, n, byt5, img, seed), dev)
    cs, us, ur = cond(B, 3, 0, 1), cond(B, 3, 0, 2), cond(B, 2, 1, 5)  # ur: another layout than cs (2 ByT5 rows and a clip_image)
    g = torch.Generator().manual_seed(3)
    known = torch.randint(0, cfg["num_labels"], shape, generator=g).to(dev)
    keep = (torch.rand(shape, generator=g) < 0.5).long().to(dev)
    init_x = torch.randint(0, cfg["num_labels"], shape, generator=g).to(dev)
    weights = [None, torch.tensor([2.0, 0.5]), (torch.tensor([1.5]), None)]
    seeds = [SEED, 5, 77]
    px = dict(device=dev, noise="philox", seed=SEED, **KW)
    pd = dict(noise="philox", seed=SEED, **KW)  # sample_distributed takes the device from its inputs
    sample, dist, requests = paella_amd.sample, paella_amd.sample_distributed, paella_amd.sample_requests
    rq = lambda **k: requests(m, cs, us, shape, seeds, device=dev, **KW, **k)

    class Foreign:  # a callable with the reference's signature that is no Paella
        num_labels = cfg["num_labels"]

        def __call__(self, x, r, **inputs):
            return m(x, r, **inputs)

    def stream(requests_kw, **stream_kw):
        one = lambda seed: (cond(1, 3, 0, seed), cond(1, 3, 0, seed + 100))
        st = paella_amd.RequestStream(m, *one(1), shape, max_steps=6, device=dev, **stream_kw)
        reqs = []
        for i, n in enumerate(STREAM_STEPS):
            c, u = one(10 + i)
            reqs.append(dict(model_inputs=c, unconditional_inputs=u, seed=100 + i, steps=n, cfg=(3.0 + i, 2.0), **requests_kw(i)))
        got = dict((r[0], r[1]) for r in st.drain(reqs))
        assert st.captures == 1
        return [got[i] for i in range(len(reqs))]

    edit = lambda i: dict(known=known[i % B], mask=keep[i % B], pin=("step", "final")[i % 2]) if i != 2 else {}
    conf = lambda i: dict(renoise=("confidence", "random")[i % 2], confidence_noise=float(i))
    half = torch.zeros(H, H, dtype=torch.bool)
    half[:, :H // 2] = True
    regions = lambda i: dict(regions=[(cond(1, 2, 0, 40 + i), half), (cond(1, 2, 0, 50 + i), ~half)][:i % 3] or None)
    return [
        ("A sample torch, one layout", lambda: sample(m, cs, shape, unconditional_inputs=us, device=dev, **KW)),
        ("A sample torch, two layouts", lambda: sample(m, cs, shape, unconditional_inputs=ur, device=dev, **KW)),
        ("B sample philox fused", lambda: sample(m, cs, shape, unconditional_inputs=us, fused_tail=True, **px)),
        ("B sample philox unfused", lambda: sample(m, cs, shape, unconditional_inputs=us, fused_tail=False, **px)),
        ("B sample philox argmax last", lambda: sample(m, cs, shape, unconditional_inputs=us, temperature=(1.0, 0.0), **px)),
        ("C sample philox ragged", lambda: sample(m, cs, shape, unconditional_inputs=ur, **px)),
        ("D sample philox cfg=0", lambda: sample(m, cs, shape, cfg=0, **px)),
        ("E distributed init_x cutoff pin", lambda: dist(m, cs, us, shape, init_x=init_x, sampling_conditional_steps=2, cfg=(8.0, 4.0), pin=(keep, known), **pd)),
        ("F sample top_k", lambda: sample(m, cs, shape, unconditional_inputs=us, top_k=5, **px)),
        ("F distributed typical_mass pin", lambda: dist(m, cs, us, shape, typical_mass=0.5, pin=(keep, known), **pd)),
        ("G sample confidence stats", lambda: sample(m, cs, shape, unconditional_inputs=us, renoise="confidence", confidence_noise=2.0, return_stats=True, **px)),
        ("G distributed confidence stats pin", lambda: dist(m, cs, us, shape, renoise="confidence", confidence_noise=2.0, return_stats=True, pin=(keep, known), **pd)),
        ("H sample shard (1, 5)", lambda: sample(m, cs, shape, unconditional_inputs=us, shard=(1, 5), **px)),
        ("I foreign model torch", lambda: sample(Foreign(), cs, shape, unconditional_inputs=us, device=dev, **KW)),
        ("J requests plain", lambda: rq()),
        ("J requests cfg per request", lambda: rq(cfg=[4.0, 2.0, (5.0, 3.0)])),
        ("J requests top_p per request", lambda: rq(top_p=[0.9, None, 0.5])),
        ("J requests renoise per request", lambda: rq(renoise=["confidence", "random", "confidence"], confidence_noise=[0.0, 1.0, 4.5])),
        ("J requests attn_weights per request", lambda: rq(attn_weights=weights)),
        ("K graph plain", lambda: paella_amd.GraphSampler(m, cs, us, shape, device=dev, **KW)(seed=SEED)),
        ("K graph top_k", lambda: paella_amd.GraphSampler(m, cs, us, shape, device=dev, top_k=5, **KW)(seed=SEED)),
        ("K graph stats", lambda: paella_amd.GraphSampler(m, cs, us, shape, device=dev, return_stats=True, **KW)(seed=SEED)),
        ("L graph requests filtering", lambda: paella_amd.GraphRequestSampler(m, cs, us, shape, device=dev, filtering=True, **KW)(seeds, top_k=[0, 5, 3])),
        ("L graph requests attn_weights", lambda: paella_amd.GraphRequestSampler(m, cs, us, shape, device=dev, max_attn_weights=4, **KW)(seeds, attn_weights=weights)),
        ("M stream plain", lambda: stream(lambda i: {})),
        ("M stream editing", lambda: stream(edit, editing=True)),
        ("M stream filtering", lambda: stream(lambda i: dict(top_k=(None, 5)[i % 2], top_p=(0.8, None)[i % 2]), filtering=True)),
        ("M stream confidence", lambda: stream(conf, confidence=True)),
        ("M stream confidence editing", lambda: stream(lambda i: dict(edit(i), **conf(i)), confidence=True, editing=True)),
        ("M stream regions", lambda: stream(regions, max_regions=2, max_cond_rows=24)),
    ]


def run(dev, markers):
    import torch
    mark = torch.full((1,), 0.5, device=dev)
    for n, (name, thunk) in enumerate(paths(dev)):
        torch.manual_seed(0)
        if markers:
            torch.erfinv(mark)
        res = thunk()
        torch.cuda.synchronize()
        maps = [v for r in (res if isinstance(res, tuple) else ()) if isinstance(r, dict) for _, v in sorted(r.items())]
        toks = res if isinstance(res, list) else [res[0] if isinstance(res, tuple) else res]
        print("%02d %-38s tokens %s%s" % (n, name, digest(toks), "  maps " + digest(maps) if maps else ""), flush=True)


def launches(directory):
    """the trace of a --markers run, cut at the markers: per path (numbered as the run prints them) the dispatches in start order"""
    from train_ab import _rows
    rows = sorted(_rows(directory, "kernel_trace.csv"), key=lambda r: int(r["Start_Timestamp"]))
    cuts = [i for i, r in enumerate(rows) if "erfinv" in r["Kernel_Name"]]
    if not cuts:
        sys.exit("no marker kernel in the trace: was it taken with --markers?")
    for n, (lo, hi) in enumerate(zip(cuts, cuts[1:] + [len(rows)])):
        seq = ["%s %sx%sx%s/%sx%sx%s" % (r["Kernel_Name"], r["Grid_Size_X"], r["Grid_Size_Y"], r["Grid_Size_Z"], r["Workgroup_Size_X"], r["Workgroup_Size_Y"],
                                         r["Workgroup_Size_Z"]) for r in rows[lo + 1:hi]]
        print("%02d launches %4d  %s" % (n, len(seq), hashlib.sha256("\n".join(seq).encode()).hexdigest()))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--device", default="cuda")
    ap.add_argument("--markers", action="store_true", help="launch a marker kernel in front of every path (for a kernel trace)")
    ap.add_argument("--launches", metavar="DIR", help="read the rocprofv3 kernel trace of a --markers run instead of running")
    args = ap.parse_args()
    launches(args.launches) if args.launches else run(args.device, args.markers)
