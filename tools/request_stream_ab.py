"""Same-process measurements around continuous request batching (paella_amd.RequestStream): the bench.py 570M-class model and VQGAN, 32x32 tokens, CFG.

    python tools/request_stream_ab.py --part a [--tree DIR]   images/s of GraphSampler and GraphRequestSampler (8 steps, with decode) at batch 1 / 32 / 128.
                                                             --tree DIR imports paella_amd and bench from another checkout (the parent commit, built there):
                                                             run it for both trees in one session, the parent three times -- its spread is the margin.
    python tools/request_stream_ab.py --part b               the price of the tick form: a FULL stream (all B slots busy, 8 steps each, ticks back to back, no
                                                             decode) against one GraphRequestSampler replay (8 steps, no decode) at the same B; plus what one
                                                             admit() and one result() with decode cost.
    python tools/request_stream_ab.py --part c               a synthetic arrival trace (fixed by --trace-seed, printed) served by the stream and by lock-step
                                                             GraphRequestSampler batches at B = 32; mean / worst completion latency and images/s of both.

Part c's clock is virtual where the server waits and real where it works: arrival times are fixed multiples of the measured full-stream tick time; every
admit / tick / result / batch replay is executed and timed (wall clock around a device synchronisation) and advances the clock by what it took.
  stream policy:    at every step boundary admit the arrived requests in arrival order while a slot is free; tick; collect (and decode) what finished.
                    With nothing running the clock jumps to the next arrival.
  lock-step policy: one GraphRequestSampler of B slots and 12 steps (an 8-step request cannot share a lock-step batch with a 12-step one: everyone takes 12).
                    A batch starts when B requests wait or when the oldest waiting request has waited --timeout-ticks tick times, whichever is first (empty
                    slots are padded and sampled like the others; near the end of the trace "B requests wait" means "the last request has arrived"); the requests of
                    a batch complete together at its end (decode inside the graph); arrivals during a replay wait.  The replay runs on the captured conditioning: no
                    per-request conditioning copy is charged to it, while the stream's admit prepares each request's own.
Recorded: profiles/request_stream_ab.txt.
"""
import argparse
import os
import random
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", required=True, choices=["a", "b", "c"])
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 32, 128])
    ap.add_argument("--replays", type=int, default=3)
    ap.add_argument("--model", default="570m", choices=["570m", "tiny"])
    ap.add_argument("--grid", type=int, default=32)
    ap.add_argument("--requests", type=int, default=192, help="part c: length of the trace")
    ap.add_argument("--arrivals-per-tick", type=float, default=2.0, help="part c: requests arriving per full-stream tick time")
    ap.add_argument("--timeout-ticks", type=float, default=8.0, help="part c: lock-step batching timeout, in tick times")
    ap.add_argument("--trace-seed", type=int, default=2024)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch

    import bench
    import paella_amd
    from paella_amd import synth
    if not torch.cuda.is_available():
        sys.exit("request_stream_ab.py needs a HIP device: nothing is timed without one")
    dev = torch.device("cuda", 0)
    cfg = bench.MODELS[a.model]
    m = paella_amd.Paella(**cfg)
    synth.randomize_(m, seed=0)
    m = m.to(dev)
    vq = paella_amd.VQModel(**bench.VQ[a.model])
    synth.randomize_(vq, seed=0)
    vq = vq.to(dev)
    mk = lambda n, seed: synth.synth_conditioning(n, 0, cfg["byt5_embd"], cfg["clip_embd"], seed=seed, device=dev)
    H = a.grid
    print("part %s, tree %s, model %s, %dx%d tokens, CFG; kernel sources %s" % (a.part, os.path.abspath(a.tree), a.model, H, H, bench.source_stamp()), flush=True)

    def timed(fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, out

    if a.part == "a":
        kw = dict(steps=8, renoise_steps=7, device=dev, vqgan=vq)
        print("%6s %16s %16s   (8 steps, with decode, hip-graph replays; mean of %d)" % ("batch", "scalar img/s", "request img/s", max(a.replays, 3)))
        for B in a.batches:
            c, u = mk(B, 2), mk(B, 3)
            gs = paella_amd.GraphSampler(m, c, u, (B, H, H), temperature=(1.0, 0.2), cfg=8.0, **kw)
            gr = paella_amd.GraphRequestSampler(m, c, u, (B, H, H), temperature=(1.0, 0.2), cfg=8.0, **kw)
            run_s = lambda i: gs(seed=1000 + i)
            run_r = lambda i: gr([1000 * (b + 1) + i for b in range(B)])
            for i in range(2):
                run_s(i), run_r(i)
            ts, tr = [], []
            for i in range(max(a.replays, 3)):
                ts.append(timed(lambda: run_s(10 + i))[0])
                tr.append(timed(lambda: run_r(10 + i))[0])
            print("%6d %16.2f %16.2f   (min ms: scalar %.2f, request %.2f)" % (B, B * len(ts) / sum(ts), B * len(tr) / sum(tr), min(ts) * 1e3, min(tr) * 1e3), flush=True)
            del gs, gr
            torch.cuda.empty_cache()
        return

    one = lambda seed: dict(model_inputs=mk(1, seed), unconditional_inputs=mk(1, seed + 1))
    if a.part == "b":
        steps = 8
        print("%6s %14s %14s %8s %14s %14s %16s" % ("batch", "request ms", "stream ms", "ratio", "ms per tick", "admit ms/req", "result+decode ms"))
        for B in a.batches:
            c, u = mk(B, 2), mk(B, 3)
            gr = paella_amd.GraphRequestSampler(m, c, u, (B, H, H), steps=steps, renoise_steps=steps - 1, temperature=(1.0, 0.2), cfg=8.0, device=dev)
            st = paella_amd.RequestStream(m, mk(1, 2), mk(1, 3), (B, H, H), max_steps=steps, device=dev, vqgan=vq)
            reqs = [one(100 + 2 * b) for b in range(B)]
            tr, tst, tad, tres = [], [], [], []
            for i in range(max(a.replays, 3) + 1):
                t_r = timed(lambda: gr([1000 * (b + 1) + i for b in range(B)]))[0]
                t_a = timed(lambda: [st.admit(seed=1000 * (b + 1) + i, steps=steps, **reqs[b]) for b in range(B)])[0]

                def ticks():
                    done = []
                    for _ in range(steps):
                        done += st.tick()
                    return done
                t_s, done = timed(ticks)
                assert sorted(done) == list(range(B))
                t_c = timed(lambda: [st.result(b) for b in done])[0]
                if i:  # the first round warms both up
                    tr.append(t_r), tst.append(t_s), tad.append(t_a / B), tres.append(t_c / B)
            assert gr.captures == 1 and st.captures == 1
            mean = lambda v: sum(v) / len(v)
            print("%6d %14.2f %14.2f %8.4f %14.3f %14.3f %16.3f   (min ms: request %.2f, stream %.2f)"
                  % (B, mean(tr) * 1e3, mean(tst) * 1e3, mean(tst) / mean(tr), mean(tst) * 1e3 / steps, mean(tad) * 1e3, mean(tres) * 1e3, min(tr) * 1e3, min(tst) * 1e3), flush=True)
            del gr, st
            torch.cuda.empty_cache()
        return

    # ---- part c
    B = 32
    rng = random.Random(a.trace_seed)
    trace_steps = [rng.choice((8, 12)) for _ in range(a.requests)]
    st = paella_amd.RequestStream(m, mk(1, 2), mk(1, 3), (B, H, H), max_steps=12, device=dev, vqgan=vq)
    gr = paella_amd.GraphRequestSampler(m, mk(B, 2), mk(B, 3), (B, H, H), steps=12, renoise_steps=11, temperature=(1.0, 0.2), cfg=8.0, device=dev, vqgan=vq)
    conds = [one(100 + 2 * (i % 16)) for i in range(16)]
    # the unit of the trace: one tick of the full stream
    for b in range(B):
        st.admit(seed=b, steps=12, **conds[b % 16])
    t_tick = []
    for i in range(12):
        t, done = timed(st.tick)
        t_tick.append(t)
    for b in range(B):
        st.result(b)
    tick = sorted(t_tick)[len(t_tick) // 2]
    arrive = [i * tick / a.arrivals_per_tick for i in range(a.requests)]
    print("trace: seed %d, %d requests, steps drawn from (8, 12) by random.Random(seed).choice: %d of 8, %d of 12; request i arrives at i * tick / %.2f; tick (median of 12 full "
          "ticks at B = %d) = %.3f ms; lock-step timeout %.1f ticks" % (a.trace_seed, a.requests, trace_steps.count(8), trace_steps.count(12), a.arrivals_per_tick, B, tick * 1e3,
                                                                       a.timeout_ticks))
    print("steps of the trace:", "".join("8" if s == 8 else "C" for s in trace_steps), "(C = 12)")

    def report(name, lat, end):
        print("%-10s mean latency %9.1f ms   worst %9.1f ms   %7.2f images/s over %.2f s" % (name, 1e3 * sum(lat) / len(lat), 1e3 * max(lat), len(lat) / end, end), flush=True)

    # stream
    now, nxt, lat, slot_of = 0.0, 0, [], {}
    while len(lat) < a.requests:
        if not slot_of and nxt < a.requests and arrive[nxt] > now:
            now = arrive[nxt]

        def work():
            nonlocal nxt
            while nxt < a.requests and arrive[nxt] <= now and st.free_slots:
                slot_of[st.admit(seed=5000 + nxt, steps=trace_steps[nxt], **conds[nxt % 16])] = nxt
                nxt += 1
            done = st.tick()
            for b in done:
                st.result(b)
            return done
        t, done = timed(work)
        now += t
        for b in done:
            lat.append(now - arrive[slot_of.pop(b)])
    report("stream", lat, now)
    assert st.captures == 1
    # lock-step
    now, nxt, lat = 0.0, 0, []
    while len(lat) < a.requests:
        first = arrive[nxt]
        full_at = arrive[min(nxt + B, a.requests) - 1]  # when B requests wait (or the trace's last one has arrived)
        start = max(now, min(full_at, first + a.timeout_ticks * tick))
        batch = [i for i in range(nxt, min(nxt + B, a.requests)) if arrive[i] <= start]
        t, _ = timed(lambda: gr([5000 + i for i in batch] + [0] * (B - len(batch))))
        now = start + t
        lat += [now - arrive[i] for i in batch]
        nxt += len(batch)
    report("lock-step", lat, now)


if __name__ == "__main__":
    main()
