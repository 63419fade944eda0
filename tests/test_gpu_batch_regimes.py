"""GPU: the UNet at the benchmark's throughput batches, checked against the CPU oracle sample by sample and launch by launch.

Every other full-size oracle comparison runs at batch 1 or 2.  From batch ~16 up the GEMM launch heuristic (gemm.hip: choose_config, choose_config_bf16)
takes other tiles and other work splits, a 64- to 256-row tile covers several samples at levels 1 and 2 (64 and 16 rows per sample), and every per-sample
epilogue / prologue feature (TimestepBlock scale / shift, the GRN apply, GRN and LayerNorm row partials) then indexes its sample by row inside the tile.

1. Per-sample parity: each sample of a batch has its own tokens, r and conditioning (seeded per sample), so a launch that reads a neighbour's scale, shift
   or statistics gives different numbers.  The UNet is row-independent per sample: the oracle evaluates only the checked samples, each at B = 1.
   Workloads: the 570M model on configs[1]'s 32x32 grid at B = 2 .. 256, configs[2]'s geometry (570M, 64x64, B = 64) and configs[3]'s per-GPU share
   (1B, 64x64, ByT5 256 + CLIP text + CLIP image, B = 32).  configs[4]'s share (1B, 128x128, B = 16) is NOT included: one oracle sample costs 2.2 TFLOP
   on the CPU, which does not fit this file's time budget; its geometry is covered at B = 1 by tests/test_gpu_unet.py.
2. Launch coverage: the per-launch records of the GEMM timing hook (paella_prof_detail / _epi / _grid) classify every launch of those forwards by tile,
   work split, prologue and epilogue class, and the test asserts that the sweep reached each branch of the launch rules.  Every distinct launch site is then
   replayed once through the op-level hooks with the heuristic tile, on the same split-K region size as the model (kSplitKBudget), asserting that the
   replay took the model's (tile, workgroups) and matches float64 on sampled rows.
3. The opt-in bf16 fast mode at B = 16, 64, 128, 256 against the exact path at the same batch, and its launch sites replayed against float64 on the rounded
   operands."""
import ctypes
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import paella_amd
from oracle import golden_configs as G
from oracle import paella_oracle as O
from paella_amd import _lib
from paella_amd.dist import shard_inputs
from tests.helpers import argmax_report, cond_for, to_dev, weights_for

pytestmark = pytest.mark.gpu
DEV = "cuda"

SWEEP_B = (2, 4, 8, 16, 32, 64, 128, 256)
BF16_B = (16, 64, 128, 256)   # (128: the one batch of the sweep whose level-1 MLP-out launch takes the 256x256 ping-pong tile, id 37)
# name -> (model config, token grid, ByT5 rows, CLIP image embeddings, forward batches, input seed)
WORKLOADS = {
    "570M 32x32": (G.UNET_570M, 32, 0, 0, SWEEP_B, 1000),
    "570M 64x64 (configs[2])": (G.UNET_570M, 64, 0, 0, (64,), 2000),
    "1B 64x64 S=260 (configs[3] share)": (G.UNET_1B, 64, 256, 1, (32,), 3000),
}
SPLIT_K_REGION = 96 << 20      # internal.h: kSplitKBudget, the split-K region every model GEMM launch gets
LN_PREPASS_MIN_ROWS = 2048     # gemm.hip: kLnPrepassMinRows
EPI_RUNTIME = 1 << 30
EPI_NAMES = ((1, "bias"), (2, "gelu"), (4, "resid"), (8, "ts"), (16, "rowstat"), (32, "sumsq"), (64, "grnfin"))
EPI_GRNFIN = 64
PRO_NAMES = {0: "plain", 1: "GRN", 2: "LN", 3: "conv", 4: "GRN-gx"}
# tile heights (gemm.hip kCfgs: wm * tm * 16) of the tiles the model launches; the row sample of a replay takes one row from every tile of that height
TILE_ROWS = {2: 64, 5: 32, 10: 128, 18: 64, 19: 32, 30: 32, 31: 32, 32: 32, 33: 64, 34: 64, 35: 32, 36: 256, 37: 256}


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check(lib, rc):
    assert rc == 0, lib.paella_last_error()


def _epi_name(c):
    if c == EPI_RUNTIME:
        return "runtime"
    return "+".join(n for b, n in EPI_NAMES if c & b) or "none"


def _split_mode(G_, T):
    return "one" if G_ == T else ("split" if G_ % T == 0 else "ranges")


# ---------------------------------------------------------------------------------------------------------------------
# inputs, oracle, records
# ---------------------------------------------------------------------------------------------------------------------
def _sample_inputs(cfg, grid, S, n_img, seed, b):
    """Sample b's own tokens, r and conditioning: a function of (seed, b) only, whatever the batch it sits in."""
    g = torch.Generator().manual_seed(seed * 100003 + b)
    x = torch.randint(0, cfg["num_labels"], (1, grid, grid), generator=g)
    r = torch.rand(1, generator=g)
    return x, r, cond_for(cfg, 1, S, n_img, seed * 100003 + b)


def _batch_inputs(cfg, grid, S, n_img, seed, B):
    parts = [_sample_inputs(cfg, grid, S, n_img, seed, b) for b in range(B)]
    c = {}
    for k, v in parts[0][2].items():
        if v is None:
            c[k] = None
        elif isinstance(v, (list, tuple)):
            c[k] = [torch.cat([p[2][k][i] for p in parts]) for i in range(len(v))]
        else:
            c[k] = torch.cat([p[2][k] for p in parts])
    return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]), c


def _checked_samples(B):
    g = torch.Generator().manual_seed(B)
    rnd = torch.randint(0, B, (2,), generator=g).tolist()
    return sorted({0, 1, B // 2 - 1, B // 2, B - 1, *rnd} & set(range(B)))


def _records(lib):
    n = lib.paella_prof_epi(None, 0)
    epi = np.zeros(3 * n, dtype=np.int32)
    grid = np.zeros(4 * n, dtype=np.int64)
    us = np.zeros(n, dtype=np.float32)
    shp = np.zeros(5 * n, dtype=np.int32)
    assert lib.paella_prof_epi(epi.ctypes.data_as(ctypes.c_void_p), n) == n
    assert lib.paella_prof_grid(grid.ctypes.data_as(ctypes.c_void_p), n) == n
    assert lib.paella_prof_detail(us.ctypes.data_as(ctypes.c_void_p), shp.ctypes.data_as(ctypes.c_void_p), n) == n
    epi, grid, shp = epi.reshape(n, 3), grid.reshape(n, 4), shp.reshape(n, 5)
    out = []
    for i in range(n):
        M, N, K, pro, tail = (int(v) for v in shp[i])
        cfg, G_, T, bf = (int(v) for v in grid[i])
        assert cfg == int(epi[i, 0]), "the work-split record and the epilogue record disagree on launch %d's tile" % i
        out.append(dict(M=M, N=N, K=K, pro=pro, tail=tail, cfg=cfg, G=G_, T=T, bf=bf, epi=int(epi[i, 2])))
    return out


def _recorded(lib, fn):
    _check(lib, lib.paella_prof_enable(1))
    try:
        out = fn()
        torch.cuda.synchronize()
        return out, _records(lib)
    finally:
        lib.paella_prof_enable(0)


_ORACLE = {}


def _oracle_sample(name, sd, cfg, x, r, c, b):
    """The oracle's logits of sample b (cached: a sample's inputs do not depend on the batch it sits in)."""
    key = (name, b)
    if key not in _ORACLE:
        with torch.no_grad():
            _ORACLE[key] = O.unet_forward(sd, cfg, x[b:b + 1], r[b:b + 1], **shard_inputs(c, b, b + 1))
    return _ORACLE[key]


@pytest.fixture(scope="module")
def lib(built_lib):
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return built_lib


@pytest.fixture(scope="module")
def sweep(lib):
    """Runs every forward of the file once: per (workload, B) the per-sample oracle maxima, the launch records of the fp32 forward and, on the 570M 32x32
    sweep at BF16_B, the bf16 fast mode's deviation, its launch records and the restore check."""
    t0 = time.time()
    res = {"parity": [], "records": [], "bf16": [], "bf16_records": [], "t_oracle": 0.0}
    for name, (cfg, grid, S, n_img, batches, seed) in WORKLOADS.items():
        m = paella_amd.Paella(**cfg)
        sd = weights_for(m, sum(cfg["blocks"]))
        m = m.to(DEV)
        x1, r1, c1 = _sample_inputs(cfg, grid, S, n_img, seed, 0)
        m(x1.to(DEV), r1.to(DEV), **to_dev(c1, DEV))      # first call: the model's one-time preparation launches stay out of the records
        for B in batches:
            x, r, c = _batch_inputs(cfg, grid, S, n_img, seed, B)
            xd, rd, cd = x.to(DEV), r.to(DEV), to_dev(c, DEV)
            exact, recs = _recorded(lib, lambda: m(xd, rd, **cd))
            res["records"] += [dict(rec, workload=name, B=B) for rec in recs]
            picks = _checked_samples(B)
            got = exact[picks].float().cpu()
            if name == "570M 32x32" and B in BF16_B:
                m.set_gemm_precision("bf16")
                try:
                    fast, brecs = _recorded(lib, lambda: m(xd, rd, **cd))
                finally:
                    m.set_gemm_precision("fp32")
                flips = (exact.argmax(1) != fast.argmax(1)).float().mean().item()
                bdiff = (fast - exact).abs().max().item()
                bstd = exact.std().item()
                finite = bool(torch.isfinite(fast).all())
                del fast
                again = m(xd, rd, **cd)
                restored = bool(torch.equal(again, exact))
                del again
                res["bf16"].append(dict(B=B, flips=flips, diff=bdiff, std=bstd, finite=finite, restored=restored))
                res["bf16_records"] += [dict(rec, workload=name, B=B) for rec in brecs]
            del exact
            torch.cuda.empty_cache()
            t1 = time.time()
            for j, b in enumerate(picks):
                ref = _oracle_sample(name, sd, cfg, x, r, c, b)
                diff = (got[j:j + 1] - ref).abs().max().item()
                std = ref.std().item()
                clear, near, n_near = argmax_report(ref, got[j:j + 1])
                res["parity"].append(dict(workload=name, B=B, b=b, diff=diff, std=std, clear=clear, near=near, n_near=n_near))
            res["t_oracle"] += time.time() - t1
        del m
        torch.cuda.empty_cache()
    res["t_total"] = time.time() - t0
    print("\nbatch-regime sweep: %.1f s (CPU oracle %.1f s, %d oracle samples)" % (res["t_total"], res["t_oracle"], len(_ORACLE)))
    return res


# ---------------------------------------------------------------------------------------------------------------------
# 1. per-sample oracle parity
# ---------------------------------------------------------------------------------------------------------------------
def test_per_sample_oracle_parity_at_throughput_batches(sweep):
    print("\n%-34s %5s %6s %11s %8s %11s %6s %s" % ("workload", "B", "sample", "max|diff|", "std", "bound", "clear", "near-tie (of)"))
    worst = {}
    for p in sweep["parity"]:
        bound = 5e-5 * max(1.0, p["std"])
        print("%-34s %5d %6d %11.3e %8.3f %11.3e %6d %d (%d)" % (p["workload"], p["B"], p["b"], p["diff"], p["std"], bound, p["clear"], p["near"], p["n_near"]))
        k = (p["workload"], p["B"])
        worst[k] = max(worst.get(k, 0.0), p["diff"])
    print("max|diff| per (workload, B): " + ", ".join("%s B=%d %.2e" % (w, B, d) for (w, B), d in worst.items()))
    for p in sweep["parity"]:
        assert p["std"] > 0.05, "degenerate logits"
        assert p["diff"] <= 5e-5 * max(1.0, p["std"]), "%s B=%d sample %d: max|diff| %.3e against the oracle" % (p["workload"], p["B"], p["b"], p["diff"])
        assert p["clear"] == 0, "%s B=%d sample %d: %d argmax mismatches with a clear reference margin" % (p["workload"], p["B"], p["b"], p["clear"])
    assert {(w, B) for w, (_, _, _, _, bs, _) in WORKLOADS.items() for B in bs} == set(worst)


# ---------------------------------------------------------------------------------------------------------------------
# 2. launch coverage
# ---------------------------------------------------------------------------------------------------------------------
# the fp32 branches of choose_config the throughput batches exist to reach (predicate over one launch record)
FP32_BRANCHES = {
    "ring tile 30/31 with a K split": lambda r: r["cfg"] in (30, 31) and r["G"] != r["T"],
    "tile 18, one tile per workgroup": lambda r: r["cfg"] == 18 and r["G"] == r["T"] and r["tail"] == 0 and r["N"] != 8192,
    "tile 18 on 512 / 1024 balanced ranges": lambda r: r["cfg"] == 18 and r["G"] in (512, 1024) and r["G"] != r["T"],
    "tile 10 on 256 persistent ranges, GRN prologue": lambda r: r["cfg"] == 10 and r["G"] == 256 and r["G"] != r["T"] and r["pro"] == 1,
    "tile 10, one tile per workgroup from 1024 tiles": lambda r: r["cfg"] == 10 and r["G"] == r["T"] and r["T"] >= 1024,
    "LayerNorm row pre-pass (>= 2048 rows)": lambda r: r["pro"] == 2 and r["M"] >= LN_PREPASS_MIN_ROWS,
    # (tile 19 / 5 -- the 1-deep tiles of small launches -- is not listed: with the ring tiles on, every model launch that lands in that class is allowed a ring
    # tile (K % 32 == 0, few samples per tile), so the class is reached only through paella_test_gemm_ring(0) or an explicit tile)
}
BF16_TILES = (34, 36, 37)


def _coverage_table(records):
    rows = {}
    for r in records:
        k = (r["bf"], r["cfg"], _split_mode(r["G"], r["T"]), PRO_NAMES.get(r["pro"], str(r["pro"])), _epi_name(r["epi"]))
        e = rows.setdefault(k, [0, set()])
        e[0] += 1
        e[1].add((r["workload"].split()[0], r["B"]))
    print("\n%-5s %4s %7s %7s %-26s %7s  %s" % ("bf16", "tile", "split", "pro", "epilogue (arguments)", "launches", "(model, B)"))
    for k in sorted(rows):
        print("%-5d %4d %7s %7s %-26s %7d  %s" % (k + (rows[k][0], " ".join("%s/%d" % wb for wb in sorted(rows[k][1])))))


def test_launch_coverage_of_the_throughput_rules(sweep):
    recs, brecs = sweep["records"], sweep["bf16_records"]
    _coverage_table(recs + brecs)
    fp32 = [r for r in recs if not r["bf"]]
    missing = [name for name, pred in FP32_BRANCHES.items() if not any(pred(r) for r in fp32)]
    assert not missing, "the sweep never reached: %s" % missing
    for tile in BF16_TILES:
        assert any(r["bf"] and r["cfg"] == tile for r in brecs), "the bf16 sweep never launched tile %d" % tile
    # the per-sample epilogue / prologue features inside multi-sample tiles: TimestepBlock scale / shift and the GRN apply on tiles that span samples
    assert any(r["epi"] != EPI_RUNTIME and r["epi"] & 8 and r["G"] != r["T"] for r in fp32), "no TimestepBlock epilogue on a split / stream-K launch"
    assert any(r["pro"] == 1 and r["M"] // r["B"] in (16, 64) and r["cfg"] in (10, 18) for r in fp32), "no GRN prologue on a multi-sample tile"


# ---------------------------------------------------------------------------------------------------------------------
# replays of every distinct launch site against float64 on sampled rows
# ---------------------------------------------------------------------------------------------------------------------
def _sampled_rows(M, cfg):
    """One row of every tile of the launch's height (rotating inside the tile), plus every row of the first and the last tile."""
    BM = TILE_ROWS.get(cfg, 32)
    tiles = (M + BM - 1) // BM
    rows = set(range(min(BM, M))) | set(range((tiles - 1) * BM, M))
    rows |= {min(M - 1, t * BM + (t * 37) % BM) for t in range(tiles)}
    return torch.tensor(sorted(rows))


def _sites(records):
    """Distinct (M, N, K, prologue) sites -> a representative record and the rows per sample of the forward it came from."""
    sites = {}
    for r in records:
        k = (r["M"], r["N"], r["K"], r["pro"], r["epi"] != EPI_RUNTIME and bool(r["epi"] & EPI_GRNFIN))
        rps = r["M"] // r["B"] if r["M"] % r["B"] == 0 else 0
        sites.setdefault(k, []).append(dict(r, rps=rps))
    return sites


def _last_grid(lib):
    n = lib.paella_prof_grid(None, 0)
    assert n > 0
    buf = np.zeros(4 * n, dtype=np.int64)
    lib.paella_prof_grid(buf.ctypes.data_as(ctypes.c_void_p), n)
    return tuple(int(v) for v in buf[-4:-1])


def _replay(lib, fn):
    _check(lib, lib.paella_prof_enable(1))
    try:
        _check(lib, fn())
        torch.cuda.synchronize()
        return _last_grid(lib)
    finally:
        lib.paella_prof_enable(0)


def _dev_gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _operands(M, N, K, g):
    # asymmetric (a transposed fragment shows), with |row mean| / std below ~0.6 and weight row sums of at most 0.02 K: the folded LayerNorm subtracts
    # mean * rowsum(W) from the accumulator, and a larger product would make the cancellation of that fold, not the launch, the dominant error
    A = torch.randn(M, K, device=DEV, generator=g) * 1.5 + 0.3 + torch.arange(K, device=DEV)[None, :] * (1.0 / K)
    W = torch.randn(N, K, device=DEV, generator=g) / K ** 0.5 + torch.arange(N, device=DEV)[:, None] * (0.02 / N)
    return A, W


def _replay_fp32(lib, M, N, K, pro, rps, cfg, splitk, ws, seed, model_cfg):
    """One launch of (M, N, K, prologue) through the op-level hooks; returns (cfg, G, T) it took and (sampled rows, output, fp64 reference) of them."""
    g = _dev_gen(seed)
    A, W = _operands(M, N, K, g)
    C = torch.full((M, N), float("nan"), device=DEV)
    rows = _sampled_rows(M, model_cfg)
    Ar = A[rows.to(DEV)].cpu().double()
    Wc = W.cpu().double()
    if pro == 0:
        bias = torch.randn(N, device=DEV, generator=g)
        R = torch.randn(M, N, device=DEV, generator=g)
        took = _replay(lib, lambda: lib.paella_op_gemm(_p(A), _p(W), _p(bias), _p(R), _p(C), M, N, K, 1, cfg, splitk, _p(ws), ws.numel(), _st()))
        ref = F.gelu(Ar @ Wc.t() + bias.cpu().double()) + R[rows.to(DEV)].cpu().double()
        del R
    elif pro == 1:
        B = M // rps
        scale = 1.0 + 0.3 * torch.randn(B, K, device=DEV, generator=g)
        shift = 0.2 * torch.randn(K, device=DEV, generator=g)
        took = _replay(lib, lambda: lib.paella_test_gemm_prologue(_p(A), _p(W), _p(C), M, N, K, 1, _p(scale), _p(shift), rps, None, cfg, splitk,
                                                                  _p(ws), ws.numel(), _st()))
        ref = (Ar * scale.cpu().double()[rows // rps] + shift.cpu().double()) @ Wc.t()
    else:
        blk = A.view(M, K // 16, 16)
        s = blk.sum(-1)
        stats = torch.stack([s, ((blk - (s / 16)[..., None]) ** 2).sum(-1)], dim=-1).contiguous()
        del blk, s
        # (mode 2 sums the weight rows with one extra M = 1 launch first: the LAST record is the launch under test)
        took = _replay(lib, lambda: lib.paella_test_gemm_prologue(_p(A), _p(W), _p(C), M, N, K, 2, None, None, 1, _p(stats), cfg, splitk,
                                                                  _p(ws), ws.numel(), _st()))
        ref = F.layer_norm(Ar, (K,), None, None, 1e-6) @ Wc.t()
    got = C[rows.to(DEV)].cpu()
    return took, rows, got, ref


def test_replay_every_fp32_launch_site_against_fp64(lib, sweep):
    recs = [r for r in sweep["records"] if not r["bf"]]
    sites = _sites(recs)
    ws = _lib.new_workspace(SPLIT_K_REGION, DEV)
    print("\n%8s %6s %6s %6s  %-24s %-24s %11s" % ("M", "N", "K", "pro", "model (cfg, G, T)", "replay (cfg, G, T)", "max|err|"))
    exempt, replayed = [], 0
    for (M, N, K, pro, grnfin), rs in sorted(sites.items()):
        r0 = rs[0]
        took_model = {(r["cfg"], r["G"], r["T"]) for r in rs}
        assert len(took_model) == 1, "site %s launched with different work splits inside the model: %s" % ((M, N, K, pro), took_model)
        if grnfin or pro == 4:
            exempt.append(((M, N, K, pro), "GRN finished in GEMM1's epilogue (force_ring) / read from its statistics: paella_test_mlp_grn_fused below"))
            continue
        if pro not in (0, 1, 2):
            exempt.append(((M, N, K, pro), "prologue %d has no op-level hook" % pro))
            continue
        # the head GEMM (N = num_labels) runs an explicit tile (gemm_tail_config, one tile per workgroup): replayed with that tile
        cfg, splitk = (r0["cfg"], 1) if N == 8192 and K == 256 else (-1, 1)
        rps = r0["rps"]
        if pro == 1 and (rps == 0 or M % rps):
            exempt.append(((M, N, K, pro), "rows per sample unknown"))
            continue
        took, rows, got, ref = _replay_fp32(lib, M, N, K, pro, rps, cfg, splitk, ws, M + 7 * N + 13 * K + pro, r0["cfg"])
        err = (got.double() - ref).abs().max().item()
        print("%8d %6d %6d %6s  %-24s %-24s %11.3e" % (M, N, K, PRO_NAMES[pro], (r0["cfg"], r0["G"], r0["T"]), took, err))
        assert took == (r0["cfg"], r0["G"], r0["T"]), "site %s: the replay took %s, the model %s" % ((M, N, K, pro), took, (r0["cfg"], r0["G"], r0["T"]))
        if pro == 0:
            np.testing.assert_allclose(got.numpy(), ref.float().numpy(), atol=2e-5 * max(1, K ** 0.5 / 8), rtol=1e-5, err_msg="site %s" % ((M, N, K, pro),))
        else:
            np.testing.assert_allclose(got.numpy(), ref.float().numpy(), atol=2e-4, rtol=2e-5, err_msg="site %s" % ((M, N, K, pro),))
        replayed += 1
        torch.cuda.empty_cache()
    print("replayed %d sites; exempt %d:" % (replayed, len(exempt)))
    for s, why in exempt:
        print("  %s: %s" % (s, why))
    # the fused GRN pair (rows per sample 16: the model's force_ring sites) through paella_test_mlp_grn_fused, against fp64 on its first and last samples
    pairs = sorted({(r["M"], r["K"], r["rps"]) for rs in sites.values() for r in rs if r["epi"] != EPI_RUNTIME and r["epi"] & EPI_GRNFIN})
    for M, c, rps in pairs:
        _check_mlp_grn_fused(lib, M, c, rps)
    assert replayed > 0


def _check_mlp_grn_fused(lib, M, c, rps):
    B = M // rps
    g = _dev_gen(M + c + rps)
    h = torch.randn(M, c, device=DEV, generator=g)
    W1 = torch.randn(4 * c, c, device=DEV, generator=g) / c ** 0.5
    b1 = 0.1 * torch.randn(4 * c, device=DEV, generator=g)
    gamma, beta = 0.5 * torch.randn(4 * c, device=DEV, generator=g), 0.3 * torch.randn(4 * c, device=DEV, generator=g)
    W2 = torch.randn(c, 4 * c, device=DEV, generator=g) / (4 * c) ** 0.5
    hidden = torch.full((M, 4 * c), float("nan"), device=DEV)
    gxd = torch.full((B, 4 * c), float("nan"), device=DEV)
    part = torch.full((B, 4 * c // 16), float("nan"), device=DEV)
    out = torch.full((M, c), float("nan"), device=DEV)
    ws = _lib.new_workspace(SPLIT_K_REGION, DEV)
    _check(lib, lib.paella_test_mlp_grn_fused(_p(h), _p(W1), _p(b1), _p(gamma), _p(beta), _p(W2), _p(hidden), _p(gxd), _p(part), _p(out), M, c, rps,
                                              _p(ws), ws.numel(), _st()))
    torch.cuda.synchronize()
    d = lambda t: t.cpu().double()
    err = 0.0
    for b in sorted({0, B - 1}):
        sl = slice(b * rps, (b + 1) * rps)
        hid = F.gelu(d(h[sl]) @ d(W1).t() + d(b1))
        gx = hid.pow(2).sum(dim=0, keepdim=True).sqrt()
        nx = gx / (gx.mean(dim=-1, keepdim=True) + 1e-6)
        ref = ((d(gamma) * (hid * nx) + d(beta) + hid) @ d(W2).t()).float()
        np.testing.assert_allclose(out[sl].cpu().numpy(), ref.numpy(), atol=2e-4 * max(1.0, float(ref.abs().max())), rtol=2e-5,
                                   err_msg="fused GRN pair M=%d c=%d rps=%d sample %d" % (M, c, rps, b))
        err = max(err, (out[sl].cpu() - ref).abs().max().item())
    print("fused GRN pair M=%d c=%d rows/sample=%d: max|err| %.3e (samples 0 and %d)" % (M, c, rps, err, B - 1))


# ---------------------------------------------------------------------------------------------------------------------
# 3. the bf16 fast mode at the same batches
# ---------------------------------------------------------------------------------------------------------------------
def test_bf16_fast_mode_at_throughput_batches(lib, sweep):
    for e in sweep["bf16"]:
        print("570M 32x32 B=%d bf16 fast mode: argmax-flip rate %.4f, max|logit diff| %.3e on logits of std %.3f, exact path restored: %s"
              % (e["B"], e["flips"], e["diff"], e["std"], e["restored"]))
    assert [e["B"] for e in sweep["bf16"]] == list(BF16_B)
    for e in sweep["bf16"]:
        assert e["finite"]
        assert 0 < e["diff"] <= 0.08 * max(1.0, e["std"]) and e["flips"] <= 0.03, e   # the bounds of test_bf16_forward_deviation_and_restore
        assert e["restored"], "B=%d: the exact path is not bit-identical after switching back" % e["B"]


def test_replay_every_bf16_launch_site_against_fp64(lib, sweep):
    brecs = [r for r in sweep["bf16_records"] if r["bf"]]
    sites = _sites(brecs)
    ws = _lib.new_workspace(SPLIT_K_REGION, DEV)
    print("\n%8s %6s %6s %6s  %-24s %-24s %11s" % ("M", "N", "K", "pro", "model (cfg, G, T)", "replay (cfg, G, T)", "max|err|"))
    for (M, N, K, pro, _), rs in sorted(sites.items()):
        r0 = rs[0]
        assert len({(r["cfg"], r["G"], r["T"]) for r in rs}) == 1
        assert pro in (0, 2), "bf16 launch with prologue %d" % pro
        cfg = r0["cfg"] if (N == 8192 and K == 256) else -1   # (the head: an explicit tile, as in fp32)
        g = _dev_gen(M + 7 * N + 13 * K + pro + 1)
        A, W = _operands(M, N, K, g)
        A16, W16 = A.bfloat16(), W.bfloat16()
        C = torch.full((M, N), float("nan"), device=DEV)
        rows = _sampled_rows(M, r0["cfg"])
        rd = rows.to(DEV)
        Ar, Wc = A16[rd].cpu().double(), W16.cpu().double()
        if pro == 0:
            bias = torch.randn(N, device=DEV, generator=g)
            R = torch.randn(M, N, device=DEV, generator=g)
            took = _replay(lib, lambda: lib.paella_test_gemm_bf16(_p(A16), _p(W16), _p(bias), _p(R), _p(C), None, M, N, K, 1, None, cfg, 1,
                                                                  _p(ws), ws.numel(), _st()))
            ref = F.gelu(Ar @ Wc.t() + bias.cpu().double()) + R[rd].cpu().double()
            del R
        else:
            blk = A.view(M, K // 16, 16)
            s = blk.sum(-1)
            stats = torch.stack([s, ((blk - (s / 16)[..., None]) ** 2).sum(-1)], dim=-1).contiguous()
            del blk, s
            took = _replay(lib, lambda: lib.paella_test_gemm_bf16_ln(_p(A16), _p(A), _p(W16), _p(C), M, N, K, _p(stats), cfg, 1, _p(ws), ws.numel(), _st()))
            A32r = A[rd].cpu().double()
            mu = A32r.mean(1, keepdim=True)
            rstd = 1.0 / torch.sqrt(A32r.var(1, unbiased=False, keepdim=True) + 1e-6)
            assert (mu.abs() * rstd).max() < 1.0          # every row takes the fold (threshold |mean| / std = 4: no operand-side guard)
            ref = ((Ar - mu) * rstd) @ Wc.t()
        got = C[rd].cpu()
        err = (got.double() - ref).abs().max().item()
        print("%8d %6d %6d %6s  %-24s %-24s %11.3e" % (M, N, K, PRO_NAMES[pro], (r0["cfg"], r0["G"], r0["T"]), took, err))
        assert took == (r0["cfg"], r0["G"], r0["T"]), "bf16 site %s: the replay took %s, the model %s" % ((M, N, K, pro), took, (r0["cfg"], r0["G"], r0["T"]))
        np.testing.assert_allclose(got.numpy(), ref.float().numpy(), atol=2e-3, rtol=2e-5, err_msg="bf16 site %s" % ((M, N, K, pro),))
        del A, W, A16, W16, C
        torch.cuda.empty_cache()
