"""Plain references of the GEMM epilogue's stores, statistics and of the implicit-convolution gather (paella_amd/csrc/common.h: Epilogue / ConvGather,
gemm_device.h: epilogue_apply / epilogue_write / rowstat_block / RowStatAcc, gemm.hip: ep_row), written from the index formulas with arange / reshape / indexing
only.  tests/test_gemm_epilogue_refs.py holds each of them against an independent torch operator on the CPU; tests/test_gpu_gemm_epilogue_features.py holds the
kernels against them.

A store reference returns, for a value matrix [M, N], the int64 matrix [M, N] of flat element indices the epilogue writes them to: scatter(buffer, index, values)
is then the whole store, and every element the index does not name must keep its bits."""
import torch
import torch.nn.functional as F

STORE_PLAIN, STORE_D2S, STORE_PIXSHUF_NCHW = 0, 1, 2


def remap_rows(M, remap_in, remap_out, remap_off):
    """Output row of row m under the row remap of the plain store: (m / remap_in) * remap_out + m % remap_in + remap_off (remap_in == 0: m itself)."""
    m = torch.arange(M)
    if remap_in <= 0:
        return m
    return torch.div(m, remap_in, rounding_mode="floor") * remap_out + m % remap_in + remap_off


def plain_index(M, N, ldc, remap=(0, 0, 0)):
    """STORE_PLAIN: element (m, n) -> row(m) * ldc + n."""
    return remap_rows(M, *remap)[:, None] * ldc + torch.arange(N)[None, :]


def _grid(M, sH, sW):
    """rows m = (b, y, x) on an [sH, sW] source grid"""
    m = torch.arange(M)
    b = torch.div(m, sH * sW, rounding_mode="floor")
    rem = m - b * sH * sW
    y = torch.div(rem, sW, rounding_mode="floor")
    return b, y, rem - y * sW


def d2s_index(M, N, ldc, sH, sW, sC, n_seg_x, py=0, px=0):
    """STORE_D2S: column n = (segment, channel), segment = (dy, dx) with dx in [0, n_seg_x); the value lands in the [B, 2 sH, 2 sW, ldc] output at
    (b, 2y + dy + py, 2x + dx + px, channel)."""
    b, y, x = _grid(M, sH, sW)
    n = torch.arange(N)
    seg = torch.div(n, sC, rounding_mode="floor")
    co = n - seg * sC
    dy = torch.div(seg, n_seg_x, rounding_mode="floor")
    dx = seg - dy * n_seg_x
    orow = (b[:, None] * (2 * sH) + 2 * y[:, None] + dy[None, :] + py) * (2 * sW) + 2 * x[:, None] + dx[None, :] + px
    return orow * ldc + co[None, :]


def pixshuf_index(M, N, sH, sW, sC):
    """STORE_PIXSHUF_NCHW: column n = c * 4 + dy * 2 + dx -> out[b][c][2y + dy][2x + dx] of an NCHW [B, sC, 2 sH, 2 sW] image."""
    b, y, x = _grid(M, sH, sW)
    n = torch.arange(N)
    c, dy, dx = n >> 2, (n >> 1) & 1, n & 1
    return ((b[:, None] * sC + c[None, :]) * (2 * sH) + 2 * y[:, None] + dy[None, :]) * (2 * sW) + 2 * x[:, None] + dx[None, :]


def scatter(buffer, index, values):
    """A copy of `buffer` (any shape, contiguous) with values[m][n] stored at flat element index[m][n]."""
    out = buffer.clone()
    out.view(-1)[index.reshape(-1)] = values.reshape(-1).to(out.dtype)
    return out


def conv_gather(x, Ho, Wo, stride, ntaps, tw_log2, oy0, ox0, tsign):
    """The A operand of the implicit-convolution GEMM: x NHWC [B, Hi, Wi, C] -> [B * Ho * Wo, ntaps * C], row (b, yo, xo), K index = tap * C + c,
    tap t = (ty, tx) = (t >> tw_log2, t & (2^tw_log2 - 1)) reads x[b][yo * stride + oy0 + tsign * ty][xo * stride + ox0 + tsign * tx][c], 0 outside the grid."""
    B, Hi, Wi, C = x.shape
    t = torch.arange(ntaps)
    ty, tx = t >> tw_log2, t & ((1 << tw_log2) - 1)
    iy = torch.arange(Ho)[:, None] * stride + oy0 + tsign * ty[None, :]   # [Ho, ntaps]
    ix = torch.arange(Wo)[:, None] * stride + ox0 + tsign * tx[None, :]   # [Wo, ntaps]
    ok = ((iy >= 0) & (iy < Hi))[:, None, :] & ((ix >= 0) & (ix < Wi))[None, :, :]  # [Ho, Wo, ntaps]
    g = x[:, iy.clamp(0, Hi - 1)[:, None, :], ix.clamp(0, Wi - 1)[None, :, :], :]   # [B, Ho, Wo, ntaps, C]
    g = g * ok[None, :, :, :, None].to(x.dtype)
    return g.reshape(B * Ho * Wo, ntaps * C)


def convT4_phase_taps(py, px):
    """Kernel taps (ky, kx) of gather tap t = (ty, tx) of output phase (py, px) of ConvTranspose2d(k4, s2, p1), as vqmodel.hip packs the phase weights:
    ky = py ? {0, 2} : {1, 3} for ty = 0, 1; the same for kx."""
    pick = lambda p, t: (1, 3)[t] if p == 0 else (0, 2)[t]
    return [(pick(py, t >> 1), pick(px, t & 1)) for t in range(4)]


def convT4_phase_weight(w, py, px):
    """torch ConvTranspose2d weight [ci, co, 4, 4] -> the phase's GEMM weight [co, 4 * ci] (K index = tap * ci + c)."""
    return torch.cat([w[:, :, ky, kx].t() for ky, kx in convT4_phase_taps(py, px)], dim=1).contiguous()


def conv4s2_weight(w):
    """torch Conv2d weight [co, ci, 4, 4] -> the GEMM weight [co, 16 * ci] (K index = (ky * 4 + kx) * ci + c)."""
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


def convT2_weight(w):
    """torch ConvTranspose2d(k2, s2) weight [ci, co, 2, 2] -> the GEMM weight [4 * co, ci], row = (dy * 2 + dx) * co + c (model.hip: RP_CONVT_K2)."""
    return w.permute(2, 3, 1, 0).reshape(-1, w.shape[0]).contiguous()


def epilogue_value(acc, bias=None, gelu=False, alpha=1.0, residual=None, ts=None, rps=1):
    """bias -> GELU (erf) -> alpha -> residual -> TimestepBlock scale / shift, in the precision of `acc`; ts = (a [B, N], b [B, N]) for samples of rps rows."""
    v = acc
    if bias is not None:
        v = v + bias.to(v.dtype)
    if gelu:
        v = F.gelu(v)
    if alpha != 1.0:
        v = v * alpha
    if residual is not None:
        v = v + residual.to(v.dtype)
    if ts is not None:
        b = torch.div(torch.arange(v.shape[0]), rps, rounding_mode="floor")
        v = v * (1 + ts[0].to(v.dtype)[b]) + ts[1].to(v.dtype)[b]
    return v


def rowstat_partials(C):
    """Epilogue::rowstat_out of the stored values C [M, N] in fp64: [M, N / 16, 2] = per row and 16-column block (sum, M2 = sum of squared deviations from the block mean)."""
    blk = C.double().reshape(C.shape[0], C.shape[1] // 16, 16)
    s = blk.sum(-1)
    return torch.stack([s, ((blk - (s / 16)[..., None]) ** 2).sum(-1)], dim=-1)


def rowstat_combine(stats, eps=1e-6):
    """RowStatAcc: (mean, rstd) of every row of K = 16 * nblk values from its block partials, by the parallel-variance formula
    M2_total = sum_j M2_j + sum_j s_j^2 / 16 - S^2 / K."""
    stats = stats.double()
    K = 16 * stats.shape[1]
    S, Q, M2 = stats[..., 0].sum(-1), (stats[..., 0] ** 2).sum(-1), stats[..., 1].sum(-1)
    mean = S / K
    var = ((M2 + Q / 16 - S * mean) / K).clamp_min(0)
    return mean, 1.0 / torch.sqrt(var + eps)


def sumsq_groups(C, dtype=torch.float64):
    """Epilogue::sumsq_out of the stored values C [M, N]: [ceil(M / 16), N] = per 16-row group, column sums of the values squared (the last group counts the rows it has)."""
    M, N = C.shape
    G = (M + 15) // 16
    v = torch.zeros(G * 16, N, dtype=dtype)
    v[:M] = C.to(dtype)
    return v.reshape(G, 16, N).pow(2).sum(1)
