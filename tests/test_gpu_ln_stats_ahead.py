"""GPU: the LayerNorm row statistics of a LayerNorm-consuming GEMM (gemm.hip: ln_issue / ln_row_stats).  On the fp32 ring tiles the producer's partials are
fetched ahead of the ring's prefetch and a row's chunks are split between the tile's two wave columns, which exchange fp64 triples through LDS; the
register-staged tile keeps the per-wave merge.  Small shapes that reach every branch of the merge: ln_nblk 3 (odd: the scalar tail), 4 (fewer chunks than
the 8 lanes that share a row) and 80 (every lane's whole batch), rows with |mean| / std 0 and 100 in one launch (the epilogue fold and the operand-side
guard), one tile per workgroup and a 2-way K split."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from paella_amd import _lib

pytestmark = pytest.mark.gpu

M, N = 48, 64  # three 16-row blocks (a full and a half-empty 32-row tile), two column tiles
BOUND = 6e-5   # tests/test_gpu_ops.py: test_layernorm_fold_error_bound_vs_row_mean, outputs of unit scale
RING_TILES = (30, 31)
REGISTER_STAGED_32x32 = 5


@pytest.fixture(scope="module")
def lib(built_lib):
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return built_lib


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def _case(K):
    """(A, W, partials, fp64 reference): rows 16..31 carry |mean| / std = 100 (their 16-row block takes the operand-side guard), the other rows 0 (the fold)."""
    g = torch.Generator().manual_seed(1000 + K)
    A = torch.randn(M, K, generator=g)
    A = A - A.mean(dim=1, keepdim=True)
    A = A * (1.0 + 0.5 * torch.rand(M, 1, generator=g))
    A[16:32] += 100.0 * A[16:32].std(dim=1, keepdim=True) * torch.sign(torch.randn(16, 1, generator=g))
    W = torch.randn(N, K, generator=g) / K ** 0.5
    ref = F.layer_norm(A.double(), (K,), None, None, 1e-6) @ W.double().t()
    blk = A.view(M, K // 16, 16)
    s = blk.sum(-1)
    stats = torch.stack([s, ((blk - (s / 16)[..., None]) ** 2).sum(-1)], dim=-1).contiguous()  # what a producing epilogue leaves: (sum, centred M2) per 16 columns
    return A, W, stats, ref


def _run(lib, cfg, K, splitk, count_guard=False):
    A, W, stats, _ = _case(K)
    Ad, Wd, sd = A.cuda(), W.cuda(), stats.cuda()
    C = torch.full((M, N), float("nan"), device="cuda")
    ws = _lib.new_workspace(16 << 20, "cuda")
    counter = torch.zeros(1, dtype=torch.int32, device="cuda")
    if count_guard:
        lib.paella_test_ln_guard_counter(_p(counter))
    try:
        rc = lib.paella_test_gemm_prologue(_p(Ad), _p(Wd), _p(C), M, N, K, 2, None, None, 1, _p(sd), cfg, splitk, _p(ws), ws.numel(), _st())
        torch.cuda.synchronize()
    finally:
        if count_guard:
            lib.paella_test_ln_guard_counter(None)
    return rc, C.cpu().double(), int(counter.item())


@pytest.mark.parametrize("K", [48, 64, 1280])
@pytest.mark.parametrize("cfg", RING_TILES + (REGISTER_STAGED_32x32,))
def test_ln_statistics_one_tile_and_split(lib, cfg, K):
    if cfg in RING_TILES and K % 32:
        # a ring tile moves whole 32-float K steps by LDS-DMA: K = 48 (ln_nblk 3) must be refused there, not run; the odd tail is the register-staged tile's case
        rc, _, _ = _run(lib, cfg, K, 1)
        err = lib.paella_last_error()
        assert rc != 0 and "K % 32" in (err.decode() if isinstance(err, bytes) else err)
        return
    _, _, _, ref = _case(K)
    rc, one, n_guard = _run(lib, cfg, K, 1, count_guard=True)
    assert rc == 0, lib.paella_last_error()
    assert n_guard > 0, "no wave took the operand-side path for the |mean| / std = 100 rows"
    rc, split, _ = _run(lib, cfg, K, 2)
    assert rc == 0, lib.paella_last_error()
    e_one, e_split, e_pair = float((one - ref).abs().max()), float((split - ref).abs().max()), float((split - one).abs().max())
    print("cfg %d K %d: one tile per workgroup %.2e  2-way split %.2e  split vs one tile %.2e" % (cfg, K, e_one, e_split, e_pair))
    assert e_one <= BOUND
    assert e_split <= BOUND
    assert e_pair <= BOUND  # the statistics do not depend on which workgroup derived them
