#!/usr/bin/env python
"""Headline benchmark: images/sec + single-image ms for Paella sampling, 256x256 px (32x32 tokens) @ 8 steps.

Contract (driver):  python bench.py --gpus N --steps K --warmup W
    N = 1 runs in-process.  N > 1 needs one process per GPU: under torch.distributed.run (RANK / WORLD_SIZE set) this file is
    a rank; started plainly with --gpus N > 1 it re-launches ITSELF under `python -m torch.distributed.run --nproc-per-node N`
    on 127.0.0.1 and relays the ranks' output.
One "step" = one pass of the hot path over one batch of synthetic input:
    sample() -- 8 denoising steps, classifier-free guidance 8.0 (cond + uncond rows batched per evaluation),
    temperature 1.0 -> 0.2, renoise 7 -- followed by VQGAN f8 decode_indices to 256x256 px.
Workload = BASELINE.json configs[1]: the 573M-class denoiser (stand-in Paella(blocks=[4,8,4]) = 570.3M params),
32x32 token grid, CLIP-text-only conditioning (byt5 of length 0), batch 1 per GPU, fp32 end to end,
seeded synthetic weights and random embeddings, inputs resident in HBM when the timed region starts.
With N GPUs every rank generates its own batch (weak scaling); rank 0 owns the conditioning of all N*batch images and
broadcasts it once per step over RCCL (the only collective of the path).

Prints ONE JSON line on rank 0 (see DESIGN.md "Measurement" for every field).  A plain run measures the headline alone: set-up, warm-up, the timed steps,
--dump-outputs if given, the line; `roofline`, `throughput`, `fast_mode`, `cpu_baseline` and `best_256px_8step` are null.  --full adds everything else the
benchmark measures, each after the headline's timed steps: rank 0's event-bracketed roofline pass of the headline, `throughput` -- the same path at throughput
batch sizes, each with its own in-run roofline: batch 32 / 64 / 128 at configs[1]'s model and grid (the BASELINE metric "256x256 @ 8 steps" at the batch where a
GPU is busiest: `best_256px_8step`), BASELINE configs[2] (one GPU only), and the per-GPU shares of the two configurations BASELINE names for 8 GPUs: configs[3]
(1B, batch 256 / 8 = 32 per GPU, 64x64 tokens, ByT5 + CLIP text + CLIP image) and configs[4] (1B, batch 128 / 8 = 16 per GPU, 128x128 tokens, the inpainting
path) --, the opt-in bf16 fast mode and the CPU baseline; --no-roofline / --no-extra / --no-cpu-baseline leave parts of it out.  On N GPUs every throughput
workload goes through the SAME broadcast + shard path as the headline (rank 0 owns the conditioning of all N x batch images; whole-node images/s,
max-over-ranks timing, per-workload broadcast_ms).

Test-only flags (tests/test_gpu_dist.py): --rehearsal (every workload on the tiny model at small sizes, plus a sharded == unsharded check of the last
step's tokens and images; the throughput workloads with --full), --dist-backend gloo --share-device (N ranks on ONE device: the N > 1 code paths on a
1-GPU box), --inject-setup-failure R.
"""
import argparse
import ctypes
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MODELS = {
    "570m": dict(c_in=256, c_out=256, num_labels=8192, c_r=64, patch_size=2, c_cond=1024, c_hidden=[640, 1280, 1280],
                 nhead=[-1, 16, 16], blocks=[4, 8, 4], level_config=['CT', 'CTA', 'CTA'], clip_embd=1024, byt5_embd=1536,
                 clip_seq_len=4, kernel_size=3, dropout=0.1, self_attn=True),
    "tiny": dict(c_in=32, c_out=32, num_labels=64, c_r=16, patch_size=2, c_cond=64, c_hidden=[32, 64, 64], nhead=[-1, 4, 4],
                 blocks=[1, 2, 1], level_config=['CT', 'CTA', 'CTA'], clip_embd=48, byt5_embd=40, clip_seq_len=4, kernel_size=3,
                 dropout=0.1, self_attn=True),
}
MODELS["1b"] = dict(MODELS["570m"], blocks=[6, 16, 6])
VQ = {"570m": dict(levels=3, bottleneck_blocks=12, c_hidden=384, c_latent=4, codebook_size=8192, scale_factor=0.3764),
      "tiny": dict(levels=3, bottleneck_blocks=2, c_hidden=64, c_latent=4, codebook_size=64, scale_factor=0.3764)}
VQ["1b"] = VQ["570m"]
PEAK_FP32_MFMA_TFLOPS = 157.3   # MI355X_MICROARCH.md: v_mfma_f32_16x16x4_f32 / 32x32x2_f32, dense
PEAK_BF16_MFMA_TFLOPS = 2500.0  # dense bf16 MFMA (v_mfma_f32_16x16x32_bf16), MI355X_MICROARCH.md
WORKLOAD_TAG = {("570m", 1, 32, 8): "BASELINE configs[1]", ("570m", 64, 64, 12): "BASELINE configs[2]",
                ("1b", 32, 64, 12): "BASELINE configs[3] per-GPU share (batch 256 over 8 GPUs)", ("1b", 16, 128, 12): "BASELINE configs[4] per-GPU share (batch 128 over 8 GPUs)"}
# SURVEY.md section 8(d)/8(a), per image: 2 * steps * F_fwd(model, grid, S) + VQGAN f8 decode (+ encode for the inpainting path), in GFLOP (the GEMM-shaped work);
# 1B entries: F_fwd at S = 264 (ByT5 256 + CLIP text 4 + CLIP image 4) as SURVEY 8(a) measured it (588.6 / 2 164 GFLOP), the conditioning hoist NOT subtracted
# Of F_fwd the GEMM FAMILY's share is priced (that is the kernel whose time the roofline divides by): minus the attention core (QK^T / PV: 4 Lq Lk c per block, 32
# level-1 + 12 level-2 AttnBlocks: 23.1 GFLOP at 64x64, 224.3 at 128x128 -- attention_lds_kernel's work, reported in the traces), and the step-invariant conditioning
# projections (kv_mapper + K/V in-projection of the S rows in all 44 blocks: 0.418 GFLOP per conditioning row = 110.4 at S = 264) counted ONCE per
# conditioning set instead of once per forward, as SURVEY 8(d) prescribes for the hoisted form.  (For the 570M / S = 4 workloads both terms are < 3 %; their
# entries keep the plain 2 * steps * F_fwd of rounds 1-4.)
ALGO_GFLOP_PER_IMAGE = {("570m", 32, 8): 2 * 8 * 66.27 + 38.8, ("570m", 64, 12): 2 * 12 * 266.5 + 155.0,
                        ("1b", 64, 12): 2 * 12 * (588.6 - 110.4 - 23.1) + 2 * 110.4 + 155.0,
                        ("1b", 128, 12): 2 * 12 * (2164.0 - 110.4 - 224.3) + 2 * 110.4 + 621.0 + 16 * 12.2}
# the throughput-regime workloads reported next to the headline: (model, batch per GPU, token grid, sampling steps, S_byt5, CLIP image embedding, inpainting path,
# timed steps, warm-up steps, captured graph).  The 1B workloads run eagerly (one warm-up + one timed batch: a capture would cost three more passes of 4-7 s each).
EXTRA_WORKLOADS = [("570m", 32, 32, 8, 0, 0, False, 3, 1, True), ("570m", 64, 32, 8, 0, 0, False, 3, 1, True), ("570m", 128, 32, 8, 0, 0, False, 2, 1, True),
                   ("570m", 64, 64, 12, 0, 0, False, 2, 1, True),
                   ("1b", 32, 64, 12, 256, 1, False, 2, 1, True), ("1b", 16, 128, 12, 256, 1, True, 2, 1, True)]
# N > 1: everything except configs[2] (a one-GPU configuration) and batch 64; the two 1B entries are the per-GPU shares of BASELINE's 8-GPU configurations
EXTRA_DISTRIBUTED = [0, 2, 4, 5]
# --rehearsal: the same table on the tiny model (every code path, seconds instead of minutes)
REHEARSAL_WORKLOADS = [("tiny", 4, 16, 4, 0, 0, False, 2, 1, True), ("tiny", 3, 16, 4, 8, 1, False, 2, 1, True), ("tiny", 2, 16, 4, 8, 1, True, 2, 1, True)]
# the kernel sources the roofline's PMC traffic figure belongs to (profiles/*_pmc_traffic.json is stamped with their hash)
TRAFFIC_SOURCES = ["paella_amd/csrc/gemm.hip", "paella_amd/csrc/gemm_device.h", "paella_amd/csrc/philox.h", "paella_amd/csrc/tail.hip", "paella_amd/csrc/model.hip",
                   "paella_amd/csrc/common.h"]


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=1, help="images per GPU per step (BASELINE configs[1]: 1)")
    ap.add_argument("--model", default="570m", choices=sorted(MODELS))
    ap.add_argument("--grid", type=int, default=32, help="token grid side (32 = 256 px at f8)")
    ap.add_argument("--sample-steps", type=int, default=8)
    ap.add_argument("--noise", default="philox", choices=["philox", "torch"])
    ap.add_argument("--no-graph", action="store_true", help="eager launches instead of one captured HIP graph per image batch")
    ap.add_argument("--full", action="store_true",
                    help="after the headline also measure everything else: its roofline pass, the throughput workloads, the bf16 fast mode, the CPU baseline "
                         "(a plain run measures the headline alone)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-extra", action="store_true", help="with --full: skip the throughput workloads and the bf16 fast mode")
    ap.add_argument("--gemm", default="fp32", choices=["fp32", "bf16"],
                    help="fp32 = the exact path (the headline); bf16 = OPT-IN fast mode outside the parity contract (bf16 MFMA operands, fp32 accumulate)")
    ap.add_argument("--hook", action="append", default=[], metavar="NAME=INT",
                    help="A/B only: call the library's test hook paella_test_NAME(INT) before building the model (paella_amd/csrc/test_hooks.h); "
                         "recorded in the output line as `test_hooks` -- a line with hooks set is not the product configuration")
    ap.add_argument("--s-byt5", type=int, default=0, help="ByT5 conditioning rows (0 = CLIP-text only, the headline; 256 for the configs[3] / configs[4] shares)")
    ap.add_argument("--clip-image", type=int, default=0, help="number of CLIP image embeddings in the conditioning (configs[3] / configs[4]: 1)")
    ap.add_argument("--inpaint", action="store_true", help="the configs[4] path: VQGAN encode -> masked renoise -> sample(init_x, t_start 0.5) -> decode (eager)")
    ap.add_argument("--no-roofline", action="store_true", help="with --full, for profiling runs: skip rank 0's event-bracketed roofline passes -- the profiler then sees "
                                                               "the timed steps alone; the line's `roofline` is null")
    ap.add_argument("--force-dist", action="store_true", help="take the torch.distributed (RCCL) path even at world size 1 (launch under torchrun)")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"], help="TEST ONLY: gloo moves device tensors through the host, which lets N ranks share one GPU")
    ap.add_argument("--share-device", action="store_true", help="TEST ONLY: every rank uses cuda:0 (needs --dist-backend gloo; RCCL refuses two ranks on one device)")
    ap.add_argument("--rehearsal", action="store_true", help="TEST ONLY: every workload on the tiny model at small sizes + a sharded == unsharded check of the results; "
                                                             "the line is marked `rehearsal` and is not a measurement")
    ap.add_argument("--inject-setup-failure", type=int, default=-1, metavar="RANK", help="TEST ONLY: the set-up of every throughput workload fails on this rank")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the headline's last timed step returned (tokens, images; all ranks' shards gathered) as DIR/<name>.npy "
                         "in float32 / float64, at most 64 MB in all (a larger output is cut to a fixed seeded sample, its flat indices in DIR/<name>_index.npy)")
    a = ap.parse_args()
    if a.dump_outputs is not None and a.steps < 1:
        ap.error("--dump-outputs needs --steps >= 1 (it writes the last timed step's outputs)")
    return a


def self_launch(a):
    """`python bench.py --gpus N` with N > 1 and no launcher: become the launcher (one rank per GPU over RCCL on 127.0.0.1)."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")  # dmabuf IPC: RCCL across processes needs it on this platform
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(a.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    print("bench.py: --gpus %d without a launcher -> %s" % (a.gpus, " ".join(cmd)), file=sys.stderr, flush=True)
    return subprocess.call(cmd, env=env)


def source_stamp():
    h = hashlib.sha256()
    for rel in TRAFFIC_SOURCES:
        with open(os.path.join(ROOT, rel), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def load_traffic(model, batch, grid, sample_steps):
    """HBM bytes per GEMM launch from a committed rocprofv3 PMC pass of this workload (tools/pmc_traffic.py writes the file and
    stamps it with the hash of the kernel sources); a file measured on other sources is REFUSED, not silently reused."""
    import glob
    stamp = source_stamp()
    stale = None
    for path in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_traffic*.json")), reverse=True):
        try:
            tj = json.load(open(path))
        except Exception:
            continue
        w = tj.get("workload", {})
        if (w.get("model"), w.get("batch_per_gpu"), w.get("grid"), w.get("sample_steps")) != (model, batch, grid, sample_steps):
            continue
        if tj.get("source_stamp") != stamp:
            stale = os.path.basename(path)
            continue
        return tj["hbm_bytes_per_launch"], ("rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes (profiles/%s, kernel-source stamp %s): 2*FETCH+WRITE KiB per "
                                            "launch, gfx950 correction applied" % (os.path.basename(path), stamp))
    return None, ("no PMC traffic file for the current kernel sources (stamp %s)%s; run tools/pmc_traffic.py on a GPU box"
                  % (stamp, "; %s is stale and was refused" % stale if stale else ""))


def timed(fn, steps, warmup, distributed, device):
    import torch
    import torch.distributed as dist
    for _ in range(warmup):
        fn()
    if distributed:
        dist.barrier()
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize(device)
    if distributed:
        dist.barrier()
    dt = time.perf_counter() - t0
    per_rank = {"min": round(dt / max(steps, 1) * 1e3, 3), "max": round(dt / max(steps, 1) * 1e3, 3)}  # ms per step on the slowest / fastest rank
    if distributed:
        t = torch.tensor([dt, -dt], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        per_rank = {"min": round(-float(t[1].item()) / max(steps, 1) * 1e3, 3), "max": round(float(t[0].item()) / max(steps, 1) * 1e3, 3)}
        dt = float(t[0].item())
    return dt, per_rank


DUMP_BUDGET_BYTES = 64 << 20


def dump_outputs(directory, arrays, budget=DUMP_BUDGET_BYTES, seed=0):
    """--dump-outputs: write {name: numpy array} as directory/<name>.npy (float32 stays float32, integers become float64, which holds every token id exactly).
    When the arrays exceed `budget` bytes in all, every array is cut to the same fraction of its elements, drawn with a fixed seed (the same flat indices for
    the same shapes on every run and every build), and the indices are written next to it as <name>_index.npy."""
    import numpy as np
    os.makedirs(directory, exist_ok=True)
    arrays = {k: (v.astype(np.float32) if v.dtype == np.float32 else v.astype(np.float64)) for k, v in arrays.items()}
    total = sum(v.nbytes for v in arrays.values())
    room = budget - 2 * 4096 * len(arrays)  # .npy headers
    frac = 1.0 if total <= room else room / float(sum(v.size * (v.itemsize + 8) for v in arrays.values()))  # + 8 bytes per sampled element: its index
    written = {}
    for name, v in sorted(arrays.items()):
        flat = v.reshape(-1)
        if frac < 1.0:
            idx = np.sort(np.random.default_rng(seed).choice(flat.size, size=max(1, int(flat.size * frac)), replace=False))
            np.save(os.path.join(directory, name + "_index.npy"), idx.astype(np.float64))
            v = flat[idx]
        np.save(os.path.join(directory, name + ".npy"), v)
        written[name] = list(v.shape)
    return written


def cpu_baseline(model_cfg, vq_cfg, grid, sample_steps, unet_sd, vq_sd, cond, uncond):
    """The oracle (CPU restatement of the reference, oracle/paella_oracle.py: kind = "port") timed on this host's cores.
    Thread count: ONE sampling step (2 forwards + tail) is timed at {16, 32, 64, all} threads, the fastest setting then runs the
    whole image -- sample_steps x 2 forwards + sampling tails + f8 decode -- which is the reported figure."""
    import torch
    from oracle import paella_oracle as O
    L = model_cfg["num_labels"]
    all_threads = torch.get_num_threads()
    noise = O.replay_torch_noise(0, (1, grid, grid), L, sample_steps, sample_steps - 1)
    t_list = [float(v) for v in torch.linspace(1.0, 0.0, sample_steps + 1)]
    temps = [float(v) for v in torch.linspace(1.0, 0.2, sample_steps)]
    cf = (8.0, -7.0)
    fwd = lambda tk, rr, **i: O.unet_forward(unet_sd, model_cfg, tk, rr, **i)
    c1 = {k: (v[:1].cpu() if v is not None else None) for k, v in cond.items()}
    u1 = {k: (v[:1].cpu() if v is not None else None) for k, v in uncond.items()}

    def run(n_steps, decode):
        t0 = time.perf_counter()
        toks, _ = O.sample(fwd, L, c1, u1, (1, grid, grid), steps=n_steps, renoise_steps=n_steps - 1, temperatures=temps[:n_steps],
                           cfgs=[cf] * n_steps, t_list=t_list[:n_steps + 1], noise=noise)
        if decode:
            O.vq_decode_indices(vq_sd, vq_cfg, toks % vq_cfg["codebook_size"])
        return time.perf_counter() - t0

    sweep = {}
    try:
        with torch.no_grad():
            for n in sorted(set(t for t in (16, 32, 64, all_threads) if t <= all_threads)):
                torch.set_num_threads(n)
                run(1, False)                 # warm-up at this thread count (allocator, thread pool)
                sweep[n] = round(run(1, False), 3)
            best = min(sweep, key=sweep.get)
            torch.set_num_threads(best)
            dt = run(sample_steps, True)
    finally:
        torch.set_num_threads(all_threads)
    return {"value": round(1.0 / dt, 4), "unit": "images/sec", "cores": best, "kind": "port",
            "sample": "1 image: %d steps x 2 forwards (cond+uncond) + sampling tails + VQGAN f8 decode, torch CPU fp32, %.1f s at %d threads "
                      "(best of a one-step sweep, seconds per step by thread count: %s; host has %d)" % (sample_steps, dt, best, json.dumps(sweep), all_threads)}


def gemm_roofline(lib, run_once, device, model, batch, grid, sample_steps, gemm, with_traffic, with_latency_model=False):
    """Roofline of the dominant kernel family (fp32 MFMA GEMM): one extra identical pass with every GEMM launch bracketed by HIP
    events on its stream (eager launches; the timed region runs without the events)."""
    import torch
    lib.paella_prof_enable(1)
    run_once()
    torch.cuda.synchronize(device)
    latency_model = None
    if with_latency_model:  # per-launch records BEFORE collect() resets them: least-squares fit of t = fixed + flops / rate over the image's GEMM launches
        import numpy as np
        cap = 1 << 16
        us = np.zeros(cap, dtype=np.float32)
        shp = np.zeros(cap * 5, dtype=np.int32)
        k = int(lib.paella_prof_detail(us.ctypes.data_as(ctypes.c_void_p), shp.ctypes.data_as(ctypes.c_void_p), cap))
        if k > 8:
            sh = shp[:k * 5].reshape(k, 5).astype(np.float64)
            fl_i, t_i = 2.0 * sh[:, 0] * sh[:, 1] * sh[:, 2], us[:k].astype(np.float64)
            A = np.stack([np.ones(k), fl_i], axis=1)
            (c0, c1), *_ = np.linalg.lstsq(A, t_i, rcond=None)
            resid = t_i - A @ np.array([c0, c1])
            latency_model = {"form": "launch_us = fixed_us + flops / kloop_tflops, least squares over the GEMM launches of one image (event-bracketed eager pass: the brackets add "
                                     "~3.5 us per launch to fixed_us; rocprofv3 traces of the same launches: profiles/)",
                             "launches": k, "fixed_us": round(float(c0), 2), "kloop_tflops": round(1e-6 / float(c1), 1) if c1 > 0 else None,
                             "rms_residual_us": round(float(np.sqrt((resid ** 2).mean())), 2), "sum_fixed_ms": round(float(c0) * k / 1e3, 3),
                             "sum_kloop_ms": round(float((fl_i * c1).sum()) / 1e3, 3)}
    ms, fl, by, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_double(), ctypes.c_int64()
    lib.paella_prof_collect(ctypes.byref(ms), ctypes.byref(fl), ctypes.byref(by), ctypes.byref(n))
    lib.paella_prof_enable(0)
    executed = fl.value / (ms.value * 1e-3) / 1e12 if ms.value > 0 else 0.0
    traffic, traffic_note = load_traffic(model, batch, grid, sample_steps) if with_traffic else (None, "not collected for this workload")
    # algorithmic work of one image as the reference executes it = 2 x sample_steps full forwards
    # + one VQGAN decode.  The CFG de-duplication executes fewer FLOPs for the same result, so both
    # figures are reported: `achieved` prices the algorithmic work, `executed_tflops` what the launches really multiplied.
    algo = ALGO_GFLOP_PER_IMAGE.get((model, grid, sample_steps))
    peak = PEAK_FP32_MFMA_TFLOPS if gemm == "fp32" else PEAK_BF16_MFMA_TFLOPS
    ach = executed
    if algo is not None and ms.value > 0:
        ach = algo * batch * 1e9 / (ms.value * 1e-3) / 1e12
    return {"bound": "mfma", "kernel": ("gemm_nt_kernel (fp32 v_mfma_f32_16x16x4_f32, all tile configs, in-launch partial-tile combine included)" if gemm == "fp32"
                                        else "gemm_nt_kernel, bf16-operand instantiations (v_mfma_f32_16x16x32_bf16, fp32 accumulate) + the fp32 instantiations for the GEMMs outside the fast mode (embedding, conditioning, VQGAN)"),
            "achieved": round(ach, 2), "peak": peak, "unit": "TFLOP/s", "frac": round(ach / peak, 4),
            "achieved_basis": ("SURVEY 8(d) algorithmic GFLOP per image (2 x steps full forwards + decode) / summed GEMM launch time"
                               if algo is not None else "executed GEMM FLOPs / summed GEMM launch time"),
            "executed_tflops": round(executed, 2), "executed_frac": round(executed / peak, 4),
            "algorithmic_gflop_per_image": algo,
            "traffic": traffic, "traffic_source": traffic_note, "algorithmic_bytes_per_launch": round(by.value / max(n.value, 1)),
            "launches_per_step": int(n.value), "avg_launch_us": round(ms.value * 1e3 / max(n.value, 1), 2),
            "gemm_ms_per_step": round(ms.value, 3), "executed_gflop_per_step": round(fl.value / 1e9, 1),
            "algorithmic_gbytes_per_step": round(by.value / 1e9, 2),
            "hbm_equiv_gbs": round(by.value / (ms.value * 1e-3) / 1e9, 1) if ms.value > 0 else 0.0,
            "latency_model": latency_model}


class Ctx:
    """what every workload of one bench.py process shares: arguments, rank / world, device, the library handle, the model zoo"""

    def __init__(self, a, rank, world, device, distributed, lib):
        self.a, self.rank, self.world, self.device, self.distributed, self.lib = a, rank, world, device, distributed, lib
        self.zoo = {}
        self.use_graph = not a.no_graph and a.noise == "philox"

    def get_model(self, name):
        """(denoiser, VQGAN, their synthetic state dicts) for a model name; built once, seeded synthetic weights (no checkpoints exist offline)"""
        import paella_amd
        from paella_amd import synth
        if name not in self.zoo:
            m = paella_amd.Paella(**MODELS[name])
            msd = synth.randomize_(m, seed=0)
            m = m.to(self.device)
            v = paella_amd.VQModel(**VQ[name])
            vsd = synth.randomize_(v, seed=0)
            v = v.to(self.device)
            self.zoo[name] = (m, v, msd, vsd)
        return self.zoo[name]

    def mk_cond(self, n, seed, name, S_byt5, n_ci):
        from paella_amd import synth
        return synth.synth_conditioning(n, S_byt5, MODELS[name]["byt5_embd"], MODELS[name]["clip_embd"], seed=seed, n_clip_image=n_ci, device=self.device)


def synth_images(lo, hi, px, device):
    """rows [lo, hi) of the job's synthetic image batch: a function of the GLOBAL row (every rank draws only its own rows, rank 0 can redraw all of them)"""
    import torch
    return torch.stack([torch.rand(3, px, px, generator=torch.Generator().manual_seed(12000 + r)) for r in range(lo, hi)]).to(device)


class Runner:
    """One workload's step function on this rank: sample() (or the inpainting recipe) + VQGAN decode for `batch` images -- a captured HIP graph replayed per
    step, or eager launches (the profiling pass always launches eagerly).  Shard-exact noise: every rank keys its Philox draws with the SAME per-step seed and
    its GLOBAL row offset, so the N-GPU job produces exactly the images of the unsharded batch (tests/test_gpu_sample.py, tests/test_gpu_graph.py)."""

    def __init__(self, ctx, name, batch, grid, sample_steps, S_byt5, n_ci, inpaint, graph, seed_base):
        import torch

        import paella_amd
        self.ctx, self.name, self.batch, self.grid, self.sample_steps, self.inpaint, self.seed_base = ctx, name, batch, grid, sample_steps, inpaint, seed_base
        self.mdl, self.vqm = ctx.get_model(name)[:2]
        a, dev = ctx.a, ctx.device
        self.kw = dict(steps=sample_steps, renoise_steps=sample_steps - 1, temperature=(1.0, 0.2), cfg=8.0, device=dev)
        self.shard = (ctx.rank * batch, ctx.world * batch) if a.noise == "philox" else None
        self.counter = 0
        self.img = self.mask = None
        if inpaint:  # BASELINE configs[4]: VQGAN encode -> masked-token renoise -> sample(init_x, t_start < 1) -> decode (paella_amd/editing.py)
            self.img = synth_images(ctx.rank * batch, (ctx.rank + 1) * batch, grid * 8, dev)
            self.mask = self.hole(batch, grid, dev)
        self.sampler = None
        if ctx.use_graph and graph:  # capture once for these shapes; every step replays it with fresh conditioning / seed / shard offset
            c0, u0 = ctx.mk_cond(batch, 2, name, S_byt5, n_ci), ctx.mk_cond(batch, 3, name, S_byt5, n_ci)
            if inpaint:
                self.sampler = paella_amd.GraphInpainter(self.mdl, self.vqm, self.img, self.mask, c0, u0, steps=sample_steps, t_start=0.5, device=dev)
            else:
                self.sampler = paella_amd.GraphSampler(self.mdl, c0, u0, (batch, grid, grid), vqgan=self.vqm, **self.kw)
        self.submission = "hip-graph replay" if self.sampler is not None else "eager launches"

    @staticmethod
    def hole(batch, grid, dev):
        import torch
        mask = torch.zeros(batch, grid, grid, dtype=torch.int64, device=dev)
        mask[:, grid // 4:3 * grid // 4, grid // 4:3 * grid // 4] = 1
        return mask

    def eager(self, c, u, seed):
        import paella_amd
        if self.inpaint:
            return paella_amd.inpaint(self.mdl, self.vqm, self.img, self.mask, c, u, steps=self.sample_steps, t_start=0.5, noise="philox", seed=seed, shard=self.shard)
        toks = paella_amd.sample(self.mdl, c, (self.batch, self.grid, self.grid), unconditional_inputs=u, noise=self.ctx.a.noise, seed=seed, shard=self.shard, **self.kw)
        return toks, self.vqm.decode_indices(toks)

    def step(self, c, u):
        self.counter += 1
        seed = self.seed_base + 1000 * self.counter
        if self.sampler is None:
            return self.eager(c, u, seed)
        if self.inpaint:
            return self.sampler(self.img, self.mask, c, u, seed=seed, shard=self.shard)
        return self.sampler(c, u, seed=seed, shard=self.shard)

    def unsharded(self, cond_all, uncond_all, seed):
        """--rehearsal, rank 0: the same request as ONE batch of world x batch images (eager), to compare the gathered shards with"""
        import paella_amd
        total = self.batch * self.ctx.world
        if self.inpaint:
            img = synth_images(0, total, self.grid * 8, self.ctx.device)
            return paella_amd.inpaint(self.mdl, self.vqm, img, self.hole(total, self.grid, self.ctx.device), cond_all, uncond_all, steps=self.sample_steps, t_start=0.5,
                                      noise="philox", seed=seed)
        toks = paella_amd.sample(self.mdl, cond_all, (total, self.grid, self.grid), unconditional_inputs=uncond_all, noise="philox", seed=seed, **self.kw)
        return toks, self.vqm.decode_indices(toks)


def run_workload(ctx, spec, steps, warmup, seed_base, fatal, with_latency_model=False, keep_outputs=False):
    """One workload through the path the N-GPU job takes: set-up (local) -> readiness agreement -> timed steps, each = [conditioning broadcast from rank 0 +
    shard slicing] + sampler -> (rehearsal: sharded == unsharded check) -> rank 0's roofline pass -> barrier.
    Returns a dict of measurements, or {"error": ...} when the set-up failed on ANY rank (never for fatal=True, the headline: exceptions propagate).
    keep_outputs: the result also carries "outputs", host copies of what the last timed step returned (every rank's shard, gathered in row order)."""
    import torch
    import torch.distributed as dist

    from paella_amd.dist import broadcast_conditioning, cond_spec_layout, shard_bounds, shard_inputs
    name, batch, grid, sample_steps, S_byt5, n_ci, inpaint, graph = spec
    a, rank, world, device, distributed = ctx.a, ctx.rank, ctx.world, ctx.device, ctx.distributed
    total = batch * world
    err = run = cond_all = uncond_all = layout = None
    lo, hi = shard_bounds(total, rank, world)
    try:  # local set-up only (no collectives): models, rank 0's conditioning for the WHOLE job, graph capture
        if not fatal and a.inject_setup_failure == rank:
            raise RuntimeError("injected set-up failure on rank %d (--inject-setup-failure)" % rank)
        mdl = ctx.get_model(name)[0]
        if rank == 0:  # rank 0 owns the conditioning of all `total` images (as if it had run the text / image encoders) ...
            cond_all, uncond_all = ctx.mk_cond(total, 2, name, S_byt5, n_ci), ctx.mk_cond(total, 3, name, S_byt5, n_ci)
        # ... and every rank derives the broadcast layout from the request shapes alone, so the per-step exchange is ONE asynchronous broadcast
        layout = cond_spec_layout(mdl, total, S_byt5=S_byt5, clip=True, n_clip_image=n_ci) if distributed else None
        run = Runner(ctx, name, batch, grid, sample_steps, S_byt5, n_ci, inpaint, graph, seed_base)
    except Exception as e:
        if fatal:
            raise
        err = repr(e)
    if distributed and not fatal:  # every rank must be ready before the first collective of this workload: agree, or skip it together
        flag = torch.tensor([0 if err else 1], device=device)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        if int(flag.item()) == 0 and err is None:
            err = "set-up failed on another rank"
    if err is not None:
        del run
        torch.cuda.empty_cache()
        return {"error": err}

    ev = {"b": [], "r": []}  # per step: (start, after the conditioning broadcast + shard, after the sampler) events -> broadcast_ms / graph_replay_ms
    last = []  # the latest step's return value (a reference only: nothing is copied inside the timed region)

    def step():
        e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        e0.record()
        if distributed:
            c, u = broadcast_conditioning([cond_all, uncond_all] if rank == 0 else None, src=0, device=device, layout=layout)
            c, u = shard_inputs(c, lo, hi), shard_inputs(u, lo, hi)
        else:
            c, u = cond_all, uncond_all
        e1.record()
        out = run.step(c, u)
        e2.record()
        ev["b"].append((e0, e1)); ev["r"].append((e1, e2))
        last[:] = [out]
        return out

    dt, per_rank = timed(step, steps, warmup, distributed, device)
    outputs = None
    if keep_outputs:  # right after the timed steps, before anything else runs: a graph replay returns its static buffers, which the next replay overwrites
        toks, img = last[0]
        outputs = {}
        for key, t in (("tokens", toks), ("images", img)):
            if distributed:
                parts = [torch.empty_like(t) for _ in range(world)]
                dist.all_gather(parts, t.contiguous())
                t = torch.cat(parts)
            outputs[key] = t.cpu().numpy()
    ev_ms = lambda pairs: round(sum(x.elapsed_time(y) for x, y in pairs[-steps:]) / max(steps, 1), 4)
    res = {"dt": dt, "total": total, "per_rank_ms": per_rank, "broadcast_ms": ev_ms(ev["b"]) if distributed else 0.0, "sampler_ms": ev_ms(ev["r"]),
           "submission": run.submission, "broadcast_bytes": (layout[1] + 1) * 4 if distributed else 0, "outputs": outputs}

    if a.rehearsal and a.noise == "philox":  # TEST ONLY: one more step, gathered, against the unsharded request on rank 0
        toks, img = step()
        seed = run.seed_base + 1000 * run.counter
        toks, img = toks.clone(), img.clone()
        if distributed:
            tl, il = [torch.empty_like(toks) for _ in range(world)], [torch.empty_like(img) for _ in range(world)]
            dist.all_gather(tl, toks)
            dist.all_gather(il, img)
            toks, img = torch.cat(tl), torch.cat(il)
        if rank == 0:
            ft, fi = run.unsharded(cond_all, uncond_all, seed)
            res["rehearsal"] = {"tokens_equal_unsharded": bool(torch.equal(toks, ft)), "images_equal_unsharded": bool(torch.equal(img, fi)),
                                "tokens": int(toks.numel()), "row_offsets": [r * batch * grid * grid for r in range(world)]}

    if rank == 0 and a.full and not a.no_roofline:  # the roofline pass (eager launches, every GEMM bracketed by events) runs on rank 0 alone; the others wait at the barrier below
        c0, u0 = (cond_all, uncond_all) if not distributed else (shard_inputs(cond_all, lo, hi), shard_inputs(uncond_all, lo, hi))
        res["roofline"] = gemm_roofline(ctx.lib, lambda: run.eager(c0, u0, seed_base + 7), device, name, batch, grid, sample_steps, a.gemm, True,
                                        with_latency_model=with_latency_model)
    if distributed:
        dist.barrier()
    del run
    torch.cuda.empty_cache()
    return res


def main():
    a = parse()
    if a.gpus > 1 and "RANK" not in os.environ:
        sys.exit(self_launch(a))

    import torch
    import torch.distributed as dist
    distributed = a.gpus > 1 or int(os.environ.get("WORLD_SIZE", "1")) > 1 or (a.force_dist and "RANK" in os.environ)
    rank, world, local = 0, 1, 0
    if a.share_device and a.dist_backend != "gloo":
        sys.exit("bench.py: --share-device needs --dist-backend gloo (RCCL refuses two ranks on one device)")
    if distributed:
        rank, world, local = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"]), int(os.environ.get("LOCAL_RANK", "0"))
        if a.share_device:
            local = 0
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        torch.cuda.set_device(local)
        if a.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group("gloo")
        if world != a.gpus and rank == 0:
            print("bench.py: --gpus %d but the launcher started %d ranks; reporting the observed world size" % (a.gpus, world), file=sys.stderr)
    device = torch.device("cuda", local)
    torch.cuda.set_device(device)
    torch.manual_seed(0)  # --noise torch draws from the global generators: the same arguments give the same inputs on every run

    from paella_amd import _lib
    lib = _lib.load()  # fails loudly if the HIP library is missing
    hooks = {}
    for h in a.hook:
        name, val = h.split("=")
        _lib.check(getattr(lib, "paella_test_" + name)(int(val)))
        hooks[name] = int(val)
    if a.rehearsal:  # TEST ONLY: the tiny model everywhere
        a.model, a.grid, a.sample_steps = "tiny", 16, 4

    ctx = Ctx(a, rank, world, device, distributed, lib)
    model, vq, unet_sd, vq_sd = ctx.get_model(a.model)
    model.set_gemm_precision(a.gemm)  # per-model switch; "fp32" (default) = the exact path
    vq.set_gemm_precision(a.gemm)
    mcfg, vcfg = MODELS[a.model], VQ[a.model]

    # ---- the headline: BASELINE configs[1] unless flags say otherwise
    head = run_workload(ctx, (a.model, a.batch, a.grid, a.sample_steps, a.s_byt5, a.clip_image, a.inpaint, True), a.steps, a.warmup, 0, fatal=True,
                        with_latency_model=(a.batch == 1), keep_outputs=a.dump_outputs is not None)
    dumped = dump_outputs(a.dump_outputs, head["outputs"]) if a.dump_outputs is not None and rank == 0 else None
    total = head["total"]
    value = total * a.steps / head["dt"]
    ms_per_step = head["dt"] / a.steps * 1e3
    headline_cfg = (a.model == "570m" or a.rehearsal) and (a.batch, a.s_byt5, a.clip_image, a.inpaint) == (1, 0, 0, False) and (a.rehearsal or (a.grid, a.sample_steps) == (32, 8))

    # ---- the same path at throughput batch sizes and on BASELINE's other configurations, each with its own in-run roofline (module docstring).  N GPUs: the
    # SAME broadcast + shard path per workload (whole-node images/s, max-over-ranks timing); a set-up failure on any rank turns the entry into an `error`. ----
    throughput = None
    if a.full and not a.no_extra and headline_cfg:
        throughput = []
        table = REHEARSAL_WORKLOADS if a.rehearsal else ([EXTRA_WORKLOADS[i] for i in EXTRA_DISTRIBUTED] if distributed else EXTRA_WORKLOADS)
        for (en, eb, eg, es, sb, nci, inp, k, w, gr) in table:
            if a.gemm != "fp32" and en != "570m":
                continue
            ident = {"model": en, "batch": eb, "grid": eg, "sample_steps": es}
            try:
                r = run_workload(ctx, (en, eb, eg, es, sb, nci, inp, gr), k, w, 50000 * eb + eg, fatal=False)
            except Exception as e:
                if distributed:  # past the readiness agreement a failure may leave the other ranks inside a collective: do not pretend otherwise
                    raise
                r = {"error": repr(e)}
            if "error" in r:
                throughput.append(dict(ident, error=r["error"]))
                continue
            if rank != 0:
                continue
            tot_e, rf = r["total"], r["roofline"]
            npar = sum(p.numel() for p in ctx.get_model(en)[0].parameters())
            entry = dict(ident, workload="%s: %s (%.1fM params), batch %d per GPU, %dx%d tokens, %d steps, CFG 8.0, conditioning S = %d (ByT5 %d + CLIP text 4%s), %s+ VQGAN f8 decode"
                         % (WORKLOAD_TAG.get((en, eb, eg, es), "configs[1] model at a throughput batch"), "Paella v3 1B (default ctor)" if en == "1b" else ("tiny test model" if en == "tiny" else "573M-class stand-in"),
                            npar / 1e6, eb, eg, eg, es, sb + 4 + 4 * nci, sb, " + CLIP image 4" if nci else "",
                            "VQGAN encode + masked renoise + sample(init_x, t_start 0.5) + re-imposed known tokens " if inp else ""),
                         n_gpus=world, images_per_step=tot_e, steps=k, warmup=w, submission=r["submission"], scaling="weak",
                         images_per_sec=round(tot_e * k / r["dt"], 3), ms_per_image=round(r["dt"] / (tot_e * k) * 1e3, 3), per_rank_ms=r["per_rank_ms"],
                         broadcast_ms=r["broadcast_ms"], broadcast_mbytes=round(r["broadcast_bytes"] / 1e6, 2), sampler_ms=r["sampler_ms"],
                         roofline={kk: rf[kk] for kk in ("bound", "achieved", "peak", "unit", "frac", "executed_tflops", "executed_frac", "launches_per_step", "avg_launch_us",
                                                         "gemm_ms_per_step", "traffic", "traffic_source", "algorithmic_bytes_per_launch", "algorithmic_gflop_per_image")})
            if "rehearsal" in r:
                entry["rehearsal"] = r["rehearsal"]
            throughput.append(entry)
        if rank != 0:
            throughput = None

    # ---- the OPT-IN bf16 fast mode (per-model switch, outside the parity contract), driver-timed as a SEPARATE entry: the headline stays fp32 ----
    fast_mode = None
    if a.full and not a.no_extra and a.gemm == "fp32" and not distributed and not a.rehearsal and headline_cfg:
        try:
            def make_runner(eb, eg, es, seed_base):
                r = Runner(ctx, a.model, eb, eg, es, 0, 0, False, True, seed_base)
                return r.step, (lambda c, u: r.eager(c, u, seed_base + 7))
            fast_mode = run_fast_mode(lib, device, model, vq, lambda n, seed: ctx.mk_cond(n, seed, a.model, 0, 0), make_runner)
        except Exception as e:
            fast_mode = {"error": repr(e)}
        finally:
            model.set_gemm_precision("fp32")
            vq.set_gemm_precision("fp32")

    cpu = None
    if rank == 0 and world == 1 and a.full and not a.no_cpu_baseline and not a.rehearsal:  # the CPU baseline is an N = 1 figure
        try:
            c1, u1 = ctx.mk_cond(1, 2, a.model, a.s_byt5, a.clip_image), ctx.mk_cond(1, 3, a.model, a.s_byt5, a.clip_image)
            cpu = cpu_baseline(mcfg, vcfg, a.grid, a.sample_steps, unet_sd, vq_sd, c1, u1)
        except Exception as e:  # the baseline is informational; never lose the GPU line over it
            cpu = {"value": None, "unit": "images/sec", "cores": torch.get_num_threads(), "kind": "port", "sample": "failed: %r" % (e,)}

    if rank == 0:
        n_params = sum(p.numel() for p in model.parameters())
        # the BASELINE metric "images/sec, 256x256 @ 8 steps" at the batch where a GPU is busiest: the best of the headline and the 32x32-token
        # / 8-step throughput entries of THIS run
        best = None
        if a.full and a.model == "570m" and (a.grid, a.sample_steps) == (32, 8):
            cands = [{"batch_per_gpu": a.batch, "images_per_sec": round(value, 3), "ms_per_image": round(ms_per_step / total, 3), "executed_frac": (head.get("roofline") or {}).get("executed_frac")}]
            for t in throughput or []:
                if "error" not in t and (t["model"], t["grid"], t["sample_steps"]) == ("570m", 32, 8):
                    cands.append({"batch_per_gpu": t["batch"], "images_per_sec": t["images_per_sec"], "ms_per_image": t["ms_per_image"], "executed_frac": t["roofline"]["executed_frac"]})
            best = dict(max(cands, key=lambda c: c["images_per_sec"]), n_gpus=world, note="whole-job images/s of the 573M-class model at 32x32 tokens / 8 steps / CFG 8 + f8 decode, "
                        "fp32, at the best per-GPU batch measured in this run (the headline `value` stays batch 1 per GPU = BASELINE configs[1])")
        line = {
            "metric": "images/sec (whole node) + single-image ms, 256x256 @ 8 steps", "value": round(value, 4), "unit": "images/sec",
            "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(ms_per_step, 3),
            "single_image_ms": round(ms_per_step / a.batch, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32" if a.gemm == "fp32" else "bf16 MFMA operands / f32 accumulate and f32 everywhere else (opt-in fast mode, outside the parity contract)", "data": "synthetic (seeded random-init weights, random CLIP-text embeddings)",
            "config": {"workload": WORKLOAD_TAG.get((a.model, a.batch, a.grid, a.sample_steps), "custom") + ": Paella %s (%.1fM params), %dx%d tokens = %d px, "
                                   "%d steps, CFG 8.0, %s, batch %d per GPU, + VQGAN f8 decode"
                                   % ("573M-class (stand-in blocks=[4,8,4])" if a.model == "570m" else a.model, n_params / 1e6, a.grid, a.grid, a.grid * 8, a.sample_steps,
                                      "CLIP-H-text only (S=4)" if (a.s_byt5, a.clip_image) == (0, 0) else "S = %d (ByT5 %d + CLIP text 4%s)" % (a.s_byt5 + 4 + 4 * a.clip_image, a.s_byt5, " + CLIP image 4" if a.clip_image else ""),
                                      a.batch),
                       "denoiser": a.model,
                       "images_per_gpu_per_step": a.batch, "images_per_step": total, "token_grid": a.grid, "sample_steps": a.sample_steps,
                       "noise": a.noise, "submission": head["submission"],
                       "parallelism": "batch-shard x%d, one conditioning broadcast per step, shard-exact Philox noise (global-row keyed)" % world,
                       "world_size_observed": (dist.get_world_size() if distributed else 1),
                       "collective_backend": ((dist.get_backend() + (" (RCCL)" if dist.get_backend() == "nccl" else " (TEST ONLY: device tensors through the host)")) if distributed else None),
                       # attribution of a step (SCALE runs: a sub-linear point can be explained from this record): wall time per rank over the timed steps (ms per
                       # step, min / max over ranks), event-timed conditioning broadcast + shard slicing, event-timed sampler (graph replay or eager launches) on rank 0
                       "per_rank_ms": head["per_rank_ms"], "broadcast_ms": head["broadcast_ms"], "broadcast_mbytes": round(head["broadcast_bytes"] / 1e6, 3),
                       "graph_replay_ms": head["sampler_ms"]},
            "roofline": head.get("roofline"), "cpu_baseline": cpu, "best_256px_8step": best, "throughput": throughput, "fast_mode": fast_mode,
        }
        if a.rehearsal:
            line["rehearsal"] = dict(head.get("rehearsal", {}), note="TEST ONLY (--rehearsal): tiny model, small sizes -- exercises the N > 1 code paths, not a measurement")
        if a.share_device:
            line["config"]["share_device"] = True
        if hooks:
            line["test_hooks"] = hooks  # A/B run: NOT the product configuration
        if dumped is not None:
            line["dumped_outputs"] = {"dir": a.dump_outputs, "shapes": dumped}
        print(json.dumps(line), flush=True)
    if distributed:
        dist.destroy_process_group()


def run_fast_mode(lib, device, model, vq, mk_cond, make_runner):
    """The opt-in bf16 fast mode on the 570M workloads of the line (batch 1, batch 32, BASELINE configs[2]): images/s, executed GEMM TFLOP/s against the dense bf16
    MFMA peak, and the argmax-flip rate / logit deviation of one forward against the exact path on the same inputs."""
    import torch
    g = torch.Generator().manual_seed(3)
    x = torch.randint(0, 8192, (1, 32, 32), generator=g).to(device)
    r = torch.rand(1, generator=g).to(device)
    c = mk_cond(1, 7)
    with torch.no_grad():
        exact = model(x, r, **c).clone()
        model.set_gemm_precision("bf16")
        vq.set_gemm_precision("bf16")
        fast = model(x, r, **c)
    out = {"mode": "bf16 MFMA operands (v_mfma_f32_16x16x32_bf16), fp32 accumulate; bf16 shadow weights and bf16 activations between GEMMs; residual stream, statistics, attention, "
                   "logits and sampling tail fp32; per-model switch (Paella.set_gemm_precision), OUTSIDE the parity contract -- the headline `value` is the fp32 path",
           "argmax_flip_rate_one_forward": round(float((exact.argmax(1) != fast.argmax(1)).float().mean()), 5),
           "max_logit_deviation": round(float((exact - fast).abs().max()), 5), "logit_std": round(float(exact.std()), 4), "peak_tflops": PEAK_BF16_MFMA_TFLOPS, "workloads": []}
    del exact, fast
    for (eb, eg, es, k, w) in [(1, 32, 8, 10, 2), (32, 32, 8, 3, 1), (64, 64, 12, 2, 1)]:
        sfn, efn = make_runner(eb, eg, es, 70000 * eb)
        ce, ue = mk_cond(eb, 2), mk_cond(eb, 3)
        dte, _ = timed(lambda: sfn(ce, ue), k, w, False, device)
        rr = gemm_roofline(lib, lambda: efn(ce, ue), device, "570m", eb, eg, es, "bf16", False)
        out["workloads"].append({"workload": WORKLOAD_TAG.get(("570m", eb, eg, es), "configs[1] model at a throughput batch"), "batch": eb, "grid": eg, "sample_steps": es, "steps": k, "warmup": w,
                                 "images_per_sec": round(eb * k / dte, 3), "ms_per_image": round(dte / (eb * k) * 1e3, 3), "executed_tflops": rr["executed_tflops"],
                                 "executed_frac_of_bf16_peak": rr["executed_frac"], "gemm_ms_per_step": rr["gemm_ms_per_step"], "launches_per_step": rr["launches_per_step"]})
        del sfn, efn
        torch.cuda.empty_cache()
    return out


if __name__ == "__main__":
    main()
