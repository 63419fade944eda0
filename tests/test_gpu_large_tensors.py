"""GPU: the kernels past the 2 GiB / 4 GiB / 8 GiB byte offsets, against a float64 CPU reference of the same operation on SAMPLED rows.

The kernels reach tensors this large through 32-bit mechanisms that stay right only while the code around them does: buffer descriptors re-based per tile
with clamped `unsigned` offsets and num_records (gemm.hip), the 2 GiB per-sample K / V span of the direct-to-LDS attention stagings (attention.hip: span32),
and int64 row indexing in the element-wise kernels.  A wrong base or clamp there reads ZEROS, not a fault -- so every test below fills the tensor regions
beyond each boundary with content a silent zero read would visibly change, and checks the rows around every row whose byte offset crosses 2^31, 2^32 or
2^33, the last rows, and ~1000 seeded random rows.  Inputs are made on the device with a seeded generator; only the sampled rows are copied to the host.
Tolerances are those of the small-shape op tests (tests/test_gpu_ops.py, tests/test_gpu_fastmode.py).
"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from paella_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
SPLITK_BUDGET = 96 << 20   # paella_amd/csrc/internal.h: kSplitKBudget, the split-K region of every model workspace
BOUNDARIES = (1 << 31, 1 << 32, 1 << 33)


@pytest.fixture(scope="module")
def lib(built_lib):
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return built_lib


@pytest.fixture(autouse=True)
def _free_device_memory():
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check(lib, rc):
    assert rc == 0, lib.paella_last_error()


def _sample_rows(M, row_bytes, seed, window=256, n_random=1000):
    """Row indices: a window around every row whose byte offset crosses a boundary in any of the tensors (row_bytes: one entry per tensor), the last
    `window` rows and `n_random` seeded random rows.  Sorted, unique, as a CPU int64 tensor."""
    rows = set(range(max(0, M - window), M))
    for rb in row_bytes:
        for b in BOUNDARIES:
            r = b // rb
            if r < M:
                rows.update(range(max(0, r - window // 2), min(M, r + window // 2)))
    g = torch.Generator().manual_seed(seed)
    rows.update(torch.randint(0, M, (n_random,), generator=g).tolist())
    return torch.tensor(sorted(rows), dtype=torch.int64)


def _region_scale(M, row_bytes):
    """A distinct factor per 2 GiB region of a tensor (1, 0.875, 0.75, ...): a row read from the wrong region, or as zeros, changes the result visibly."""
    r = torch.div(torch.arange(M, device=DEV, dtype=torch.int64) * row_bytes, 1 << 31, rounding_mode="floor")
    return (1.0 - 0.125 * r.float())[:, None]


def _randn(shape, seed):
    return torch.randn(*shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed))


def _ln_partials_device(A, chunk=1 << 18):
    """What a producing GEMM's epilogue leaves per row and 16-column block (sum, M2), computed on the device in row chunks (tests/test_gpu_ops.py: _ln_partials)."""
    M, K = A.shape
    out = torch.empty(M, K // 16, 2, device=DEV)
    for r0 in range(0, M, chunk):
        blk = A[r0:r0 + chunk].view(-1, K // 16, 16)
        s = blk.sum(-1)
        out[r0:r0 + chunk, :, 0] = s
        out[r0:r0 + chunk, :, 1] = ((blk - (s / 16)[..., None]) ** 2).sum(-1)
    return out


def _assert_rows(got, ref, rows, atol, rtol, what):
    """assert_allclose on sampled rows; the message names the worst row (so a failure says which region went wrong)."""
    got, ref = got.double(), ref.double()
    excess = ((got - ref).abs() - (atol + rtol * ref.abs())).amax(dim=1)
    worst = int(excess.argmax())
    assert torch.isfinite(got).all(), "%s: non-finite values in sampled rows" % what
    np.testing.assert_allclose(got.numpy(), ref.numpy(), atol=atol, rtol=rtol,
                               err_msg="%s: worst row %d (max |diff| there %.3e)" % (what, int(rows[worst]), float((got[worst] - ref[worst]).abs().max())))


# ---------------------------------------------------------------------------------------------------------------------
# 1. fp32 GEMM through paella_op_gemm: A, C and the residual each over 4 GiB
# ---------------------------------------------------------------------------------------------------------------------
def test_gemm_fp32_a_c_residual_over_4gib(lib):
    """M = 2^21 + 1237, K = N = 640: A, C and the residual are 5.4 GB each.  Bias + GELU + residual on every tile family the launch rule can pick at this M
    -- the 32x32 ring tiles (30 / 31, with their specialised epilogue class), the 64x64 direct-to-LDS tile (18, the rule's choice), the 8-wave 128x128 tile (10)
    -- and the rule itself, one tile per workgroup (at this M a split needs more slab space than the model's split-K region holds: see the long-K test)."""
    M, N, K = (1 << 21) + 1237, 640, 640
    rb = K * 4
    A = _randn((M, K), 1).mul_(_region_scale(M, rb))
    R = _randn((M, N), 2).mul_(_region_scale(M, N * 4))
    g = torch.Generator().manual_seed(3)
    W = torch.randn(N, K, generator=g) / K ** 0.5 + torch.arange(N)[:, None] * 2e-4   # asymmetric: transposed fragments show
    bias = torch.randn(N, generator=g)
    Wd, bd = W.to(DEV), bias.to(DEV)
    rows = _sample_rows(M, (rb, N * 4), seed=4)
    rd = rows.to(DEV)
    ref = F.gelu(A[rd].cpu().double() @ W.double().t() + bias.double()) + R[rd].cpu().double()
    ws = _lib.new_workspace(SPLITK_BUDGET, DEV)
    C = torch.empty(M, N, device=DEV)
    for cfg in (30, 31, 18, 10, -1):
        C[rd] = float("nan")
        _check(lib, lib.paella_op_gemm(_p(A), _p(Wd), _p(bd), _p(R), _p(C), M, N, K, 1, cfg, 1, _p(ws), ws.numel(), _st()))
        torch.cuda.synchronize()
        _assert_rows(C[rd].cpu(), ref, rows, atol=2e-5 * max(1, K ** 0.5 / 8), rtol=1e-5, what="fp32 GEMM tile %d" % cfg)


def test_gemm_fp32_long_k_split_over_4gib(lib):
    """The work splits need few tiles (the slabs and tickets of a split launch live in the 96 MiB split-K region): M = 8269, N = 96, K = 131072 puts A at
    4.3 GB with 512 KiB rows, so rows 4096 and 8192 cross 2^31 and 2^32.  Classic split-K (tiles 5 and 18), stream-K on a ring tile (31, 1500 workgroups over 777 tiles) and
    the launch rule, with bias + GELU + residual."""
    M, N, K = 8192 + 77, 96, 131072
    rb = K * 4
    A = _randn((M, K), 11).mul_(_region_scale(M, rb))
    g = torch.Generator().manual_seed(12)
    W = torch.randn(N, K, generator=g) / K ** 0.5 + torch.arange(N)[:, None] * 2e-6
    bias, R = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    Wd, bd, Rd = W.to(DEV), bias.to(DEV), R.to(DEV)
    rows = _sample_rows(M, (rb,), seed=13)
    rd = rows.to(DEV)
    ref = F.gelu(A[rd].cpu().double() @ W.double().t() + bias.double()) + R[rows].double()
    ws = _lib.new_workspace(SPLITK_BUDGET, DEV)
    C = torch.empty(M, N, device=DEV)
    for cfg, splitk in ((5, 3), (18, 2), (31, -1500), (-1, 1)):
        C.fill_(float("nan"))
        _check(lib, lib.paella_op_gemm(_p(A), _p(Wd), _p(bd), _p(Rd), _p(C), M, N, K, 1, cfg, splitk, _p(ws), ws.numel(), _st()))
        torch.cuda.synchronize()
        _assert_rows(C[rd].cpu(), ref, rows, atol=2e-5 * max(1, K ** 0.5 / 8), rtol=1e-5, what="fp32 GEMM K=%d tile %d splitk %d" % (K, cfg, splitk))


# ---------------------------------------------------------------------------------------------------------------------
# 2. Operand prologues at > 4 GiB A through paella_test_gemm_prologue
# ---------------------------------------------------------------------------------------------------------------------
def test_gemm_prologues_over_4gib(lib):
    """mode 1 = GRN apply a * scale[row / rows_per_sample][k] + shift[k] with 4112 rows per sample (the last samples' rows sit 5 GB from the base), mode 2 = the
    fp32 LayerNorm fold from [M, K/16, 2] partials, with whole 16-row blocks at |mean| / std ~ 100 (the operand-side guard) around every boundary.  A is 5.4 GB.
    Mode 2 runs without the row pre-pass (it does not fit the split-K region at this M) and, on the rule's tile, with it (a larger workspace)."""
    rps, B, N, K = 4112, 511, 64, 640
    M = rps * B   # 2 101 232 rows
    rb = K * 4
    A = _randn((M, K), 21).mul_(_region_scale(M, rb)).add_(0.3)
    g = torch.Generator().manual_seed(22)
    W = torch.randn(N, K, generator=g) / K ** 0.5 + torch.arange(N)[:, None] * 1e-3
    scale, shift = 1.0 + 0.3 * torch.randn(B, K, generator=g), 0.2 * torch.randn(K, generator=g)
    rows = _sample_rows(M, (rb,), seed=23)
    # mode 2: 16-row blocks far off-centre (|mean| / std ~ 100) at each boundary, at the end and at a few random places
    hot = sorted({(b // rb) // 16 for b in BOUNDARIES if b // rb < M} | {M // 16 - 1} | set(torch.randint(0, M // 16, (8,), generator=g).tolist()))
    hot_rows = torch.cat([torch.arange(16 * h, 16 * h + 16) for h in hot])
    rows = torch.unique(torch.cat([rows, hot_rows]))
    rd = rows.to(DEV)
    Wd, sc, sh = W.to(DEV), scale.to(DEV), shift.to(DEV)
    ws = _lib.new_workspace(SPLITK_BUDGET, DEV)
    C = torch.empty(M, N, device=DEV)
    A_s = A[rd].cpu().double()
    ref1 = (A_s * scale.double()[rows // rps] + shift.double()) @ W.double().t()
    for cfg, splitk in ((10, 1), (18, 1), (30, 1), (-1, 1)):
        C.fill_(float("nan"))
        _check(lib, lib.paella_test_gemm_prologue(_p(A), _p(Wd), _p(C), M, N, K, 1, _p(sc), _p(sh), rps, None, cfg, splitk, _p(ws), ws.numel(), _st()))
        torch.cuda.synchronize()
        _assert_rows(C[rd].cpu(), ref1, rows, atol=2e-4, rtol=2e-5, what="GRN-apply prologue tile %d" % cfg)
    hr = hot_rows.to(DEV)
    A[hr] += 100.0 * A[hr].std(dim=1, keepdim=True)
    stats = _ln_partials_device(A)
    A_s = A[rd].cpu().double()
    ratio = A_s.mean(1).abs() / A_s.std(1, unbiased=False)
    assert int((ratio > 50).sum()) == hot_rows.numel() and float(ratio[ratio <= 50].max()) < 4
    ref2 = F.layer_norm(A_s, (K,), None, None, 1e-6) @ W.double().t()
    ws_pre = _lib.new_workspace((160 << 20), DEV)   # room for the row pre-pass (80 MiB of slabs + 16 B per row)
    for cfg, splitk, w in ((18, 1, ws), (31, 1, ws), (10, 1, ws), (-1, 1, ws), (-1, 1, ws_pre)):
        C.fill_(float("nan"))
        _check(lib, lib.paella_test_gemm_prologue(_p(A), _p(Wd), _p(C), M, N, K, 2, None, None, 1, _p(stats), cfg, splitk, _p(w), w.numel(), _st()))
        torch.cuda.synchronize()
        _assert_rows(C[rd].cpu(), ref2, rows, atol=2e-4, rtol=2e-5, what="LayerNorm prologue tile %d, %d MiB workspace" % (cfg, w.numel() >> 20))


# ---------------------------------------------------------------------------------------------------------------------
# 3. bf16 operands: A16 over 4 GiB, the bf16 copy of C over 4 GiB, C over 8 GiB
# ---------------------------------------------------------------------------------------------------------------------
def test_gemm_bf16_over_4gib(lib):
    """M = 3 400 003, K = N = 640: A16 and the C16 copy are 4.35 GB, the fp32 C and residual 8.7 GB (rows 3 355 443 on cross 2^33).  Bias + GELU (the fast
    polynomial, inside atol) + residual, on the 64x64 direct-to-LDS tile (the rule's choice), a ring tile, the 256x128 and 256x256 tiles and the rule; reference:
    fp64 on the bf16-rounded operands (tests/test_gpu_fastmode.py)."""
    M, N, K = 3_400_003, 640, 640
    A16 = _randn((M, K), 31).mul_(_region_scale(M, K * 2)).bfloat16()
    torch.cuda.empty_cache()
    R = _randn((M, N), 32)
    g = torch.Generator().manual_seed(33)
    W16 = ((torch.randn(N, K, generator=g) + torch.arange(N)[:, None] * 0.02) / 8).bfloat16()
    bias = torch.randn(N, generator=g)
    W16d, bd = W16.to(DEV), bias.to(DEV)
    rows = _sample_rows(M, (K * 2, N * 4), seed=34)
    rd = rows.to(DEV)
    ref = F.gelu(A16[rd].cpu().double() @ W16.double().t() + bias.double()) + R[rd].cpu().double()
    ws = _lib.new_workspace(SPLITK_BUDGET, DEV)
    C = torch.empty(M, N, device=DEV)
    C16 = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
    for cfg in (18, 30, 36, 37, -1):
        C[rd] = float("nan")
        C16[rd] = 0
        _check(lib, lib.paella_test_gemm_bf16(_p(A16), _p(W16d), _p(bd), _p(R), _p(C), _p(C16), M, N, K, 1, None, cfg, 1, _p(ws), ws.numel(), _st()))
        torch.cuda.synchronize()
        got = C[rd].cpu()
        _assert_rows(got, ref, rows, atol=2e-3, rtol=2e-5, what="bf16 GEMM tile %d" % cfg)
        assert torch.equal(C16[rd].cpu(), got.bfloat16()), "bf16 GEMM tile %d: the bf16 copy is not the rounding of the fp32 output" % cfg


# ---------------------------------------------------------------------------------------------------------------------
# 4. bf16 LayerNorm fold above ~1.03 M rows: the row pre-pass no longer fits the split-K region
# ---------------------------------------------------------------------------------------------------------------------
def test_gemm_bf16_layernorm_fold_without_room_for_the_prepass(lib):
    """The model's bf16 LayerNorm-consuming launch (paella_test_gemm_bf16_ln: bf16 copy, fp32 statistics and the fp32 rows for the operand-side guard) at
    M = 2^20 + 37 with a workspace of exactly kSplitKBudget: the row pre-pass (80 MiB + 16 B per row) does not fit.  The 8-wave tiles (10, 36) and the
    ping-pong tile (37) take their statistics from the pre-pass only; the launcher runs such a launch on the 64x64 tile (18), which carries the guard in the
    kernel, instead of failing it.  Whole 16-row blocks at |mean| / std ~ 160 exercise that guard; the rest take the fold.  Reference as
    tests/test_gpu_fastmode.py::test_bf16_gemm_layernorm_guard_every_tile, and every result equals the forced 4-wave tile's within that path's tolerance."""
    M, N, K = (1 << 20) + 37, 640, 640
    A = _randn((M, K), 41).mul_(1.5).add_(0.3)
    g = torch.Generator().manual_seed(42)
    hot = sorted({(b // (K * 4)) // 16 for b in BOUNDARIES if b // (K * 4) < M} | {M // 16 - 1} | set(torch.randint(0, M // 16, (8,), generator=g).tolist()))
    hot_rows = torch.cat([torch.arange(16 * h, 16 * h + 16) for h in hot])
    hr = hot_rows.to(DEV)
    A[hr] += 240.0 + torch.arange(hot_rows.numel(), device=DEV)[:, None] % 16 * 0.5
    A16 = A.bfloat16()
    stats = _ln_partials_device(A)
    W = torch.randn(N, K, generator=g) / K ** 0.5 + torch.arange(N)[:, None] * 1e-3
    W16 = W.bfloat16()
    W16d = W16.to(DEV)
    rows = torch.unique(torch.cat([_sample_rows(M, (K * 4, K * 2, N * 4), seed=43), hot_rows]))
    rd = rows.to(DEV)
    A_s = A[rd].cpu().double()
    mu = A_s.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(A_s.var(1, unbiased=False, keepdim=True) + 1e-6)
    flagged = torch.isin(rows, hot_rows)
    ratio = (mu.abs() * rstd).view(-1)
    assert float(ratio[flagged].min()) > 100 and float(ratio[~flagged].max()) < 1.0
    ln = (A_s - mu) * rstd
    ref = torch.where(flagged[:, None], ln.float().bfloat16().double() @ W16.double().t(), ((A16[rd].cpu().double() - mu) * rstd) @ W16.double().t())
    ws = _lib.new_workspace(SPLITK_BUDGET, DEV)
    assert ws.numel() == SPLITK_BUDGET
    C = torch.empty(M, N, device=DEV)
    outs = {}
    for cfg in (18, 10, 36, 37, -1):
        C.fill_(float("nan"))
        A16w = A16.clone()   # a launch with the pre-pass rewrites flagged rows of its bf16 operand in place: every launch starts from the same copy
        _check(lib, lib.paella_test_gemm_bf16_ln(_p(A16w), _p(A), _p(W16d), _p(C), M, N, K, _p(stats), cfg, 1, _p(ws), ws.numel(), _st()))
        torch.cuda.synchronize()
        del A16w
        got = C[rd].cpu()
        outs[cfg] = got
        _assert_rows(got[~flagged], ref[~flagged], rows[~flagged], atol=2e-3, rtol=2e-5, what="bf16 LayerNorm fold tile %d, folded rows" % cfg)
        _assert_rows(got[flagged], ref[flagged], rows[flagged], atol=1e-2, rtol=2e-5, what="bf16 LayerNorm fold tile %d, guarded rows" % cfg)
    for cfg in (10, 36, 37, -1):
        _assert_rows(outs[cfg], outs[18], rows, atol=2e-3, rtol=2e-5, what="bf16 LayerNorm fold tile %d against the forced 4-wave tile" % cfg)


# ---------------------------------------------------------------------------------------------------------------------
# 5. Attention across span32: per-sample K / V spans just below and just above 2^31 bytes
# ---------------------------------------------------------------------------------------------------------------------
def _attention_reference(q_s, ks, vs, kc, vc, D, chunk=1 << 15):
    """fp64 attention of the queries q_s [nq, nh, D] of one sample over its self keys (device tensors [Ls, nh * D], streamed to the host in chunks) and
    conditioning keys [Lc, nh * D]."""
    nq, nh, _ = q_s.shape
    Ls = ks.shape[0]
    s = torch.empty(nq, nh, Ls + kc.shape[0], dtype=torch.float64)
    for c0 in range(0, Ls, chunk):
        k = ks[c0:c0 + chunk].cpu().double().view(-1, nh, D)
        s[:, :, c0:c0 + k.shape[0]] = torch.einsum("qhd,nhd->qhn", q_s, k)
    s[:, :, Ls:] = torch.einsum("qhd,nhd->qhn", q_s, kc.double().view(-1, nh, D))
    p = (s / D ** 0.5).softmax(-1)
    out = torch.einsum("qhn,nhd->qhd", p[:, :, Ls:], vc.double().view(-1, nh, D))
    for c0 in range(0, Ls, chunk):
        v = vs[c0:c0 + chunk].cpu().double().view(-1, nh, D)
        out += torch.einsum("qhn,nhd->qhd", p[:, :, c0:c0 + v.shape[0]], v)
    return out.reshape(nq, nh * D)


@pytest.mark.parametrize("Ls,kernel", [((1 << 19) - 1, "direct-to-LDS"), ((1 << 19) + 1, "register-fed")])
def test_attention_across_span32(lib, Ls, kernel):
    """16 heads x 64 (ld = 1024 floats = 4 KiB per key): Lself = 2^19 - 1 keeps a sample's K / V span just below 2^31 bytes (the direct-to-LDS staging with its
    2 GiB num_records), 2^19 + 1 puts it just above (the register-fed kernel with 64-bit pointers).  B = 2, so sample 1 starts 2 GiB into K and V; 256 queries
    (the non-split forms).  Three of the four reference queries per sample have a dominant key planted among the last keys of the sample -- past the 2 GiB
    offset of the tensor -- with a distinct value row: a key read as zeros loses its weight and the output moves by O(1)."""
    B, nh, D, Lq, Lc = 2, 16, 64, 256, 8
    C = nh * D
    q = _randn((B, Lq, C), 51)
    ks = _randn((B, Ls, C), 52)
    vs = _randn((B, Ls, C), 53)
    kc, vc = _randn((B, Lc, C), 54), _randn((B, Lc, C), 55)
    qi = [0, 77, 191, 255]
    for b in range(B):
        for j, i in enumerate(qi[:3]):
            p = Ls - 1 - 5 * j
            ks[b, p] = 4.0 * q[b, i]            # score 4 |q_h|^2 / 8 ~ 32 per head (>= ~20 on every head): dominates the ~5e5 keys of O(1) score (their sum ~ e^14)
            vs[b, p] = 3.0 + j + b              # a value row no other key has
    out = torch.full((B, Lq, C), float("nan"), device=DEV)
    _check(lib, lib.paella_op_attention(_p(q), _p(ks), _p(vs), _p(kc), _p(vc), _p(out), B, nh, D, Lq, Ls, Lc, None, 0, _st()))
    torch.cuda.synchronize()
    for b in range(B):
        ref = _attention_reference(q[b, qi].cpu().double().view(len(qi), nh, D), ks[b], vs[b], kc[b].cpu(), vc[b].cpu(), D)
        got = out[b, qi].cpu()
        assert float(ref[:3].abs().min()) > 1.0   # the planted keys carry the planted queries
        _assert_rows(got, ref, torch.tensor(qi), atol=2e-5, rtol=1e-4, what="attention (%s), sample %d" % (kernel, b))


# ---------------------------------------------------------------------------------------------------------------------
# 6. Element-wise kernels past 2^31 elements
# ---------------------------------------------------------------------------------------------------------------------
def test_layernorm_past_2pow31_elements(lib):
    """paella_op_layernorm on 3 360 001 rows of 640 (2.15e9 elements, 8.6 GB in and out): rows crossing 2^31, 2^32 and 2^33 bytes (= 2^31 elements)."""
    rows_n, C = 3_360_001, 640
    x = _randn((rows_n, C), 61).mul_(3).add_(1)
    y = torch.empty_like(x)
    _check(lib, lib.paella_op_layernorm(_p(x), _p(y), rows_n, C, 1e-6, _st()))
    torch.cuda.synchronize()
    rows = _sample_rows(rows_n, (C * 4,), seed=62)
    rd = rows.to(DEV)
    ref = F.layer_norm(x[rd].cpu().double(), (C,), eps=1e-6)
    _assert_rows(y[rd].cpu(), ref, rows, atol=3e-6, rtol=1e-5, what="layernorm")


@pytest.mark.parametrize("skip", [False, True])
def test_dwconv_ln_past_2pow31_elements(lib, skip):
    """paella_op_dwconv_ln (3x3 depthwise conv, zero padding, then LayerNorm over channels) on 822 images of 64 x 64 x 640 channels (2.15e9 elements per
    tensor), with and without the concatenated skip input.  Checked on whole image rows: those around each boundary, every border row of the last image
    and 256 random ones; a reference output row needs the three input rows around it."""
    B, H, W, C = 822, 64, 64, 640
    x = _randn((B, H, W, C), 71)
    sk = _randn((B, H, W, C), 72) if skip else None
    g = torch.Generator().manual_seed(73)
    w = torch.randn(C, 2 if skip else 1, 3, 3, generator=g) * 0.3
    bias = torch.randn(C, generator=g) * 0.1
    wk, bd = w.permute(1, 2, 3, 0).contiguous().to(DEV), bias.to(DEV)   # [J, 3, 3, C]
    y = torch.empty(B, H, W, C, device=DEV)
    _check(lib, lib.paella_op_dwconv_ln(_p(x), _p(sk), _p(wk), _p(bd), _p(y), B, H, W, C, 1e-6, _st()))
    torch.cuda.synchronize()
    img_rows = set()   # (b * H + y)
    for b_off in BOUNDARIES:
        p = b_off // (C * 4)
        if p < B * H * W:
            img_rows.update(range(max(0, p // W - 2), min(B * H, p // W + 3)))
    img_rows.update((B - 1) * H + yy for yy in (0, 1, H - 2, H - 1))
    img_rows.update(torch.randint(0, B * H, (256,), generator=g).tolist())
    ir = torch.tensor(sorted(img_rows), dtype=torch.int64)
    bb, yy = ir // H, ir % H
    ys = yy[:, None] + torch.arange(-1, 2)[None, :]                  # [n, 3] input rows
    valid = (ys >= 0) & (ys < H)
    ysc = ys.clamp(0, H - 1)
    flat = (bb[:, None] * H + ysc).reshape(-1).to(DEV)

    def gather(t):
        v = t.view(B * H, W, C)[flat].cpu().double().view(-1, 3, W, C) * valid[:, :, None, None]
        return v.permute(0, 3, 1, 2)                                  # [n, C, 3, W]
    inp = gather(x) if not skip else torch.cat([gather(x), gather(sk)], 1)
    conv = F.conv2d(inp, w.double(), bias.double(), padding=(0, 1), groups=C)   # [n, C, 1, W]
    ref = F.layer_norm(conv[:, :, 0].permute(0, 2, 1), (C,), None, None, 1e-6)  # [n, W, C]
    got = y.view(B * H, W, C)[ir.to(DEV)].cpu()
    _assert_rows(got.reshape(-1, C), ref.reshape(-1, C), (ir[:, None] * W + torch.arange(W)[None, :]).reshape(-1), atol=2e-5, rtol=1e-5,
                 what="dwconv_ln (skip=%s)" % skip)
