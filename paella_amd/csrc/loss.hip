// Training loss head: classifier (out_mapper, no bias) + label-smoothed cross-entropy fused, forward and backward, without a logits tensor.
//
//   l[m, n] = sum_k h[m, k] w[n, k]                        (v_mfma_f32_16x16x4_f32, the exact path of gemm.hip; "A" = weight rows, "B" = activation rows,
//                                                           so a lane holds 4 consecutive labels of one row)
//   forward : per 64 x 64 logit tile the epilogue reduces every row to (max, sum exp(l - max), sum l, best value, best label) and the tile that owns the
//             target's column leaves l[m, target]; head_loss_finalize_kernel merges a row's partials in ASCENDING tile order into loss, lse and argmax.
//   backward: d[m, n] = g[m] (exp(l[m, n] - lse[m]) - (1 - eps) [n == target[m]] - eps / N) is recomputed tile by tile from h, w and lse (after one pass that
//             renormalises exp(l - lse) by its own row sum: see head_loss_bwd_kernel), re-laid through LDS as
//             an MFMA operand and contracted at once: dh = d w (a workgroup owns 64 rows and walks the column tiles), dw = d^T h (a workgroup owns 64 labels
//             and walks a contiguous share of the row tiles; the shares of a column tile go to [N, K] slabs that one small kernel sums in share order).
// Nothing proportional to rows x N is ever stored; logits, probabilities and d live in registers and LDS.  No float atomics, no tickets: every combine runs in
// an order fixed by the shape alone (the row split of dw is a function of (rows, N, K), never of the device), so two runs give the same bits.
// A target outside [0, N) marks an ignored row: loss 0, d = 0, and neither w nor a partial is ever indexed with it.
#include "train_common.h"
#include <math.h>

namespace {

using namespace train;

constexpr int kTile = 64;        // rows and labels of a logit tile (4 waves, each a 32 x 32 quarter)
constexpr int kThreads = 256;
constexpr int kFwdBK = 64;       // K step of the forward tile
constexpr int kFwdStride = kFwdBK + 4;
constexpr int kPStride = kTile + 4;
constexpr int kPartWords = 5;    // (max, sum exp, sum l, best value, best label) per row and column tile
constexpr int kMaxSplit = 16;    // most row shares of a dw column tile
constexpr int kSplitTarget = 512;  // workgroups the dw launch aims at (two per CU)
constexpr int64_t kMaxRows = (int64_t)1 << 24;

struct Plan {
    int tiles_n;
    int64_t tiles_m;
    int split;           // row shares per dw column tile
    size_t tgt_off, part_off, fwd_bytes;  // forward: target logits [rows], partials [tiles_n, 5, rows] (tiles_n > 1 only)
    size_t corr_off, npart_off, slab_off; // backward: 1 / sum_n exp(l - lse) per row [rows], its per-tile partials [tiles_n, rows] (tiles_n > 1 only), ...
    size_t slab_bytes, bwd_bytes;         // ... and `split` slabs of [N, K] (split > 1 only)
    size_t bytes;
};

bool shape_ok(int64_t rows, int N, int K) {
    return rows >= 1 && rows <= kMaxRows && K >= 16 && K <= 256 && (K & 15) == 0 && N >= 16 && N <= 65536 && (N & 15) == 0;
}

// everything here depends on the shape only: the same shape always gets the same split, hence the same summation order
Plan make_plan(int64_t rows, int N, int K) {
    Plan p = {};
    p.tiles_n = (N + kTile - 1) / kTile;
    p.tiles_m = (rows + kTile - 1) / kTile;
    if (p.tiles_n > 1) {
        p.tgt_off = 0;
        p.part_off = align256((size_t)rows * sizeof(float));
        p.fwd_bytes = p.part_off + align256((size_t)p.tiles_n * kPartWords * (size_t)rows * sizeof(float));
    }
    p.slab_bytes = align256((size_t)N * K * sizeof(float));
    p.corr_off = 0;
    p.npart_off = align256((size_t)rows * sizeof(float));
    p.slab_off = p.npart_off + (p.tiles_n > 1 ? align256((size_t)p.tiles_n * (size_t)rows * sizeof(float)) : 0);
    int64_t s = (kSplitTarget + p.tiles_n - 1) / p.tiles_n;
    if (s > kMaxSplit) s = kMaxSplit;
    if (s > p.tiles_m) s = p.tiles_m;
    if (s < 1) s = 1;
    // from 4096 rows up the whole workspace stays under a quarter of one logits tensor (rows * N bytes); below that the slabs may dominate
    const size_t cap = (size_t)rows * (size_t)N;
    if (rows >= 4096)
        while (s > 1 && p.slab_off + (size_t)s * p.slab_bytes >= cap) --s;
    p.split = (int)s;
    p.bwd_bytes = p.slab_off + (p.split > 1 ? (size_t)p.split * p.slab_bytes : 0);
    p.bytes = p.fwd_bytes > p.bwd_bytes ? p.fwd_bytes : p.bwd_bytes;
    if (p.bytes < 256) p.bytes = 256;  // 0 is reserved for "unsupported shape"
    return p;
}

// rows [row0, row0 + 64) x columns [k0, k0 + kw) of a row-major [nrows, ld] matrix -> dst[64][stride]; rows past the matrix are zero.  kw % 16 == 0.
__device__ __forceinline__ void stage_tile(float* __restrict__ dst, int stride, const float* __restrict__ src, int ld, int64_t row0, int64_t nrows, int k0, int kw) {
    const int vpr = kw >> 2;          // 16-byte vectors per row
    const int total = kTile * vpr;    // a multiple of 256
    for (int base = (int)threadIdx.x; base < total; base += 4 * kThreads) {
        f32x4 v[4];
        int off[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = base + u * kThreads;
            const int row = idx / vpr, c = idx - row * vpr;
            off[u] = idx < total ? row * stride + c * 4 : -1;
            v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (idx < total && row0 + row < nrows) v[u] = *reinterpret_cast<const f32x4*>(src + (size_t)(row0 + row) * ld + k0 + c * 4);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (off[u] >= 0) *reinterpret_cast<f32x4*>(dst + off[u]) = v[u];
    }
}

// A logit as an unevaluated sum hi + lo of two fp32 numbers.  One fp32 multiply-add chain over all of K rounds every partial sum at the size the sum has reached:
// with logits of order 100 that is 3 ulp (5e-5) at K = 32 already, and it reaches the gradients through exp(l - lse) on every row that is not one-hot.  So the MFMA
// chain is cut every 16 columns of K -- a chain of 16 products starting from zero rounds at the size of ITS sum -- and the chunk sums are added with the
// error-free two-sum, the rounding errors of these additions collected in lo.  hi is then the fp32 number next to the sum of the chunk sums and lo what it misses.
struct Logits {
    f32x4 hi[2][2], lo[2][2];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) hi[i][j] = lo[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    __device__ __forceinline__ void add(int i, int j, f32x4 p) {  // two-sum (Knuth): hi + p = s + err exactly
        const f32x4 s = hi[i][j] + p;
        const f32x4 bb = s - hi[i][j];
        lo[i][j] += (hi[i][j] - (s - bb)) + (p - bb);
        hi[i][j] = s;
    }
    __device__ __forceinline__ void finish() {  // hi = fl(hi + lo), lo = the rest
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const f32x4 s = hi[i][j] + lo[i][j];
                lo[i][j] -= s - hi[i][j];
                hi[i][j] = s;
            }
    }
    // l - ref for a ref near l: the difference of the two fp32 numbers is exact, lo joins after it
    __device__ __forceinline__ float minus(int i, int j, int r, float ref) const { return (hi[i][j][r] - ref) + lo[i][j][r]; }
};

// this wave's 32 x 32 quarter of the logit tile over kw columns of the staged operands, ADDED to acc: acc.hi/lo[i][j][r] = l[row (wm * 2 + i) * 16 + r16][label (wn * 2 + j) * 16 + kq * 4 + r]
__device__ __forceinline__ void logit_mma(Logits& acc, const float* __restrict__ hs, const float* __restrict__ wt, int stride, int kw, int wm, int wn, int r16, int kq) {
    for (int kk = 0; kk < kw; kk += 16) {
        f32x4 a[2], b[2], p[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) p[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 2; ++i) a[i] = *reinterpret_cast<const f32x4*>(hs + ((wm * 2 + i) * 16 + r16) * stride + kk + kq * 4);
#pragma unroll
        for (int j = 0; j < 2; ++j) b[j] = *reinterpret_cast<const f32x4*>(wt + ((wn * 2 + j) * 16 + r16) * stride + kk + kq * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) p[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(b[j][e], a[i][e], p[i][j], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc.add(i, j, p[i][j]);
    }
}

__device__ __forceinline__ bool better(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }  // the lowest label wins a tie

// loss, lse and argmax of one row from its merged statistics
__device__ __forceinline__ void finish_row(int64_t m, float mx, float se, float sl, float tl, bool valid, int bi, int N, float eps, float* __restrict__ loss,
                                           float* __restrict__ lse, int* __restrict__ argmax) {
    const float lg = logf(se);
    lse[m] = mx + lg;
    if (argmax) argmax[m] = (unsigned)bi < (unsigned)N ? bi : 0;
    float v = 0.f;
    if (valid) {  // lse - x as (max - x) + log(sum): the small difference first, so that the rounding of max + log(sum) at the size of the logits stays out of the loss
        const float nll = (mx - tl) + lg;
        v = eps == 0.f ? nll : (1.f - eps) * nll + eps * ((mx - sl / (float)N) + lg);
    }
    loss[m] = v;
}

__global__ __launch_bounds__(kThreads) void head_loss_fwd_kernel(const float* __restrict__ h, const float* __restrict__ w, const int64_t* __restrict__ target, int64_t rows,
                                                                 int N, int K, int tiles_n, float eps, float* __restrict__ part, float* __restrict__ tgt_ws,
                                                                 float* __restrict__ loss, float* __restrict__ lse, int* __restrict__ argmax,
                                                                 const float* __restrict__ lse_in, float* __restrict__ corr) {
    __shared__ __attribute__((aligned(16))) float smem[2 * kTile * kFwdStride];
    __shared__ float red[2][kTile][8];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, r16 = lane & 15, kq = lane >> 4;
    const int tile_n = (int)(blockIdx.x % (unsigned)tiles_n);
    const int64_t m0 = (int64_t)(blockIdx.x / (unsigned)tiles_n) * kTile;
    const int n0 = tile_n * kTile;
    float* hs = smem;
    float* wt = smem + kTile * kFwdStride;

    Logits acc;
    acc.clear();
    for (int k0 = 0; k0 < K; k0 += kFwdBK) {
        const int kw = min(kFwdBK, K - k0);
        if (k0) __syncthreads();
        stage_tile(hs, kFwdStride, h, K, m0, rows, k0, kw);
        stage_tile(wt, kFwdStride, w, K, n0, N, k0, kw);
        __syncthreads();
        logit_mma(acc, hs, wt, kFwdStride, kw, wm, wn, r16, kq);
    }
    acc.finish();

    if (lse_in) {  // renormalisation pass of the backward (kernel-uniform): the tile's share of sum_n exp(l - lse), same reduction order as below
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = (wm * 2 + i) * 16 + r16;
            const float ls = m0 + row < rows ? lse_in[m0 + row] : 0.f;
            float se = 0.f;
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (n0 + (wn * 2 + j) * 16 + kq * 4 + r < N) se += expf(acc.minus(i, j, r, ls));
            se += __shfl_xor(se, 16, 64);
            se += __shfl_xor(se, 32, 64);
            if (kq == 0) red[wn][row][0] = se;
        }
        __syncthreads();
        if (tid < kTile && m0 + tid < rows) {
            const float se = red[0][tid][0] + red[1][tid][0];
            if (tiles_n == 1) corr[m0 + tid] = 1.f / se;
            else part[(size_t)tile_n * (size_t)rows + m0 + tid] = se;
        }
        return;
    }
    // per row of the tile: this wave's 32 labels -> LDS -> one thread per row merges the two wave columns (wn = 0 first)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = (wm * 2 + i) * 16 + r16;
        const int64_t m = m0 + row;
        const int64_t t = m < rows ? target[m] : -1;
        float mx = -INFINITY, sl = 0.f, bv = -INFINITY, tl = 0.f;
        int bi = 0x7fffffff, has = 0;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = n0 + (wn * 2 + j) * 16 + kq * 4 + r;
                const float v = acc.hi[i][j][r];
                if (n < N) {  // the masked tail: no exp, nothing to sum l, never the argmax
                    mx = fmaxf(mx, v);
                    sl += v;
                    if (v > bv) { bv = v; bi = n; }
                    if ((int64_t)n == t) { tl = v; has = 1; }
                }
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        float se = 0.f;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (n0 + (wn * 2 + j) * 16 + kq * 4 + r < N) se += expf(acc.minus(i, j, r, mx));
#pragma unroll
        for (int x = 16; x <= 32; x <<= 1) {
            se += __shfl_xor(se, x, 64);
            sl += __shfl_xor(sl, x, 64);
            const float ov = __shfl_xor(bv, x, 64);
            const int oi = __shfl_xor(bi, x, 64);
            if (better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
            const float ot = __shfl_xor(tl, x, 64);
            const int oh = __shfl_xor(has, x, 64);
            if (oh) { tl = ot; has = 1; }
        }
        if (kq == 0) {
            float* q = red[wn][row];
            q[0] = mx; q[1] = se; q[2] = sl; q[3] = bv; q[4] = __int_as_float(bi); q[5] = tl; q[6] = __int_as_float(has);
        }
    }
    __syncthreads();
    if (tid < kTile && m0 + tid < rows) {
        const int64_t m = m0 + tid;
        const float* a = red[0][tid];
        const float* b = red[1][tid];
        const float mx = fmaxf(a[0], b[0]);
        float se = a[1] * expf(a[0] - mx);          // the first 32 labels of a tile are never all masked (N % 16 == 0 and n0 < N): a[0] is finite for finite logits
        if (b[0] > -INFINITY) se += b[1] * expf(b[0] - mx);
        const float sl = a[2] + b[2];
        float bv = a[3];
        int bi = __float_as_int(a[4]);
        if (better(b[3], __float_as_int(b[4]), bv, bi)) { bv = b[3]; bi = __float_as_int(b[4]); }
        const bool has = __float_as_int(a[6]) | __float_as_int(b[6]);
        const float tl = __float_as_int(a[6]) ? a[5] : b[5];
        if (tiles_n == 1) {
            finish_row(m, mx, se, sl, tl, has, bi, N, eps, loss, lse, argmax);
        } else {
            float* q = part + (size_t)tile_n * kPartWords * (size_t)rows + m;
            q[0] = mx; q[(size_t)rows] = se; q[2 * (size_t)rows] = sl; q[3 * (size_t)rows] = bv; q[4 * (size_t)rows] = __int_as_float(bi);
            if (has) tgt_ws[m] = tl;
        }
    }
}

// one thread per row: the partials of its column tiles, in ascending tile order
__global__ __launch_bounds__(kThreads) void head_loss_finalize_kernel(const float* __restrict__ part, const float* __restrict__ tgt_ws, const int64_t* __restrict__ target,
                                                                      int64_t rows, int N, int tiles_n, float eps, float* __restrict__ loss, float* __restrict__ lse,
                                                                      int* __restrict__ argmax) {
    const int64_t m = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (m >= rows) return;
    const size_t R = (size_t)rows;
    float mx = -INFINITY, bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int t = 0; t < tiles_n; ++t) {
        const float* q = part + (size_t)t * kPartWords * R + m;
        mx = fmaxf(mx, q[0]);
        const float v = q[3 * R];
        const int i = __float_as_int(q[4 * R]);
        if (better(v, i, bv, bi)) { bv = v; bi = i; }
    }
    float se = 0.f, sl = 0.f;
    for (int t = 0; t < tiles_n; ++t) {
        const float* q = part + (size_t)t * kPartWords * R + m;
        se += q[R] * expf(q[0] - mx);
        sl += q[2 * R];
    }
    const int64_t tg = target[m];
    const bool valid = tg >= 0 && tg < N;
    finish_row(m, mx, se, sl, valid ? tgt_ws[m] : 0.f, valid, bi, N, eps, loss, lse, argmax);
}

// corr[m] = 1 / sum_n exp(l[m, n] - lse[m]) from the per-tile sums, in ascending tile order
__global__ __launch_bounds__(kThreads) void head_loss_renorm_kernel(const float* __restrict__ part, int64_t rows, int tiles_n, float* __restrict__ corr) {
    const int64_t m = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (m >= rows) return;
    float se = 0.f;
    for (int t = 0; t < tiles_n; ++t) se += part[(size_t)t * (size_t)rows + m];
    corr[m] = 1.f / se;
}

// Backward.  The probabilities are exp(l - lse) * corr with corr = 1 / sum_n exp(l - lse) from the renormalisation pass above: lse is ONE fp32 number per row, and
// with logits of order 100 its rounding (half an ulp of 100: 4e-6) would otherwise sit on every probability of the row -- on a near one-hot row as an absolute
// 4e-6 in p[target] - 1, against 6e-8 for a softmax normalised by its own sum.  The pass recomputes the logit tiles a third time and restores that normalisation.
// DW = false: dh of the 64 rows of row tile blockIdx.x (resident operand: the h tile; streamed: the w tiles).  DW = true: share blockIdx.x / tiles_n of
// dw of column tile blockIdx.x % tiles_n (resident: the w tile; streamed: the h tiles of the share).  Per streamed tile: logits -> d -> P in LDS (d[m][n] for dh,
// d^T[n][m] for dw) -> out[x][k] += sum_y P[x][y] S[y][k], S the streamed tile.  Wave v owns the 16 resident indices x = 16 v ... and all of K in KC chunks of 64:
// MFMA (kc, e, ke) takes "A"[i][y] = S[y0 + 4 kq + e][kc * 64 + 4 i + ke] (one ds_read_b128 per e serves the four ke) and "B"[y][x] = P[x][y0 + 4 kq + e], so
// accumulator (kc, ke) register r of lane (x, kq) is out[x][kc * 64 + 16 kq + 4 r + ke].  A chunk that overhangs K reads the tile's padding: those are "A" rows
// i of columns k >= K, which reach only accumulator rows that are never stored.
template <bool DW, int KC>
__global__ __launch_bounds__(kThreads, 1) void head_loss_bwd_kernel(const float* __restrict__ h, const float* __restrict__ w, const int64_t* __restrict__ target,
                                                                    const float* __restrict__ lse, const float* __restrict__ corr, const float* __restrict__ grad,
                                                                    int64_t rows, int N, int K,
                                                                    int tiles_n, int64_t tiles_m, int split, float eps, float* __restrict__ out, size_t slab_floats) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int stride = K + 4;
    const int tile_floats = kTile * stride + kTile;
    float* hs = lds;
    float* wt = lds + tile_floats;
    float* P = lds + 2 * tile_floats;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, r16 = lane & 15, kq = lane >> 4;
    const float smooth = eps / (float)N, hit = 1.f - eps;

    int64_t s0, s1;   // streamed tiles [s0, s1)
    int64_t res0;     // first resident index
    if (DW) {
        const int tile_n = (int)(blockIdx.x % (unsigned)tiles_n);
        const int share = (int)(blockIdx.x / (unsigned)tiles_n);
        s0 = tiles_m * share / split;
        s1 = tiles_m * (share + 1) / split;
        res0 = (int64_t)tile_n * kTile;
        out += (size_t)share * slab_floats;
        stage_tile(wt, stride, w, K, res0, N, 0, K);
    } else {
        s0 = 0;
        s1 = tiles_n;
        res0 = (int64_t)blockIdx.x * kTile;
        stage_tile(hs, stride, h, K, res0, rows, 0, K);
    }

    f32x4 acc[KC][4];
#pragma unroll
    for (int c = 0; c < KC; ++c)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[c][e] = f32x4{0.f, 0.f, 0.f, 0.f};

    float rg[2], rl[2], rc[2];
    int rt[2];  // target label of the lane's two rows, -1 = no contribution (ignored row, or past the matrix)
    auto load_rows = [&](int64_t m0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int64_t m = m0 + (wm * 2 + i) * 16 + r16;
            rg[i] = 0.f; rl[i] = 0.f; rc[i] = 0.f; rt[i] = -1;
            if (m < rows) {
                const int64_t t = target[m];
                if (t >= 0 && t < N) { rt[i] = (int)t; rg[i] = grad[m]; rl[i] = lse[m]; rc[i] = corr[m]; }
            }
        }
    };
    if (!DW) load_rows(res0);

    for (int64_t s = s0; s < s1; ++s) {
        __syncthreads();  // the previous tile's products are done with the streamed tile and with P
        const int64_t m0 = DW ? s * kTile : res0;
        const int n0 = DW ? (int)res0 : (int)s * kTile;
        if (DW) {
            stage_tile(hs, stride, h, K, m0, rows, 0, K);
            load_rows(m0);
        } else {
            stage_tile(wt, stride, w, K, n0, N, 0, K);
        }
        __syncthreads();
        Logits l;
        l.clear();
        logit_mma(l, hs, wt, stride, K, wm, wn, r16, kq);
        l.finish();
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = (wm * 2 + i) * 16 + r16;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int col = (wn * 2 + j) * 16 + kq * 4;
                f32x4 d;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int n = n0 + col + r;
                    float v = 0.f;
                    if (rt[i] >= 0 && n < N) v = rg[i] * (expf(l.minus(i, j, r, rl[i])) * rc[i] - (DW && n == rt[i] ? hit : 0.f) - smooth);  // dh: the target's term is applied once, at the store
                    d[r] = v;
                }
                if (DW) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) P[(col + r) * kPStride + row] = d[r];
                } else {
                    *reinterpret_cast<f32x4*>(P + row * kPStride + col) = d;
                }
            }
        }
        __syncthreads();
        const float* S = DW ? hs : wt;
#pragma unroll
        for (int y0 = 0; y0 < kTile; y0 += 16) {
            const f32x4 pv = *reinterpret_cast<const f32x4*>(P + (wave * 16 + r16) * kPStride + y0 + 4 * kq);
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                f32x4 sv[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) sv[e] = *reinterpret_cast<const f32x4*>(S + (y0 + 4 * kq + e) * stride + c * 64 + 4 * r16);
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int ke = 0; ke < 4; ++ke) acc[c][ke] = __builtin_amdgcn_mfma_f32_16x16x4f32(sv[e][ke], pv[e], acc[c][ke], 0, 0, 0);
            }
        }
    }

    // dh: - g (1 - eps) w[target] joins here and not inside d.  It is the one large term of a row (everything else is a probability times a weight); added to the
    // accumulator somewhere along the 8192-label chain it would set the rounding step of every later addition (measured on the fp64 model at 257 x 8192 x 256:
    // max error 2.2e-6 inside the chain, 9e-8 here)
    const int64_t x = res0 + wave * 16 + r16;
    if (x < (DW ? (int64_t)N : rows)) {
        float gh = 0.f;
        const float* wt_row = w;
        if (!DW) {
            const int64_t t = target[x];
            if (t >= 0 && t < N) { gh = grad[x] * hit; wt_row = w + (size_t)t * K; }
        }
#pragma unroll
        for (int c = 0; c < KC; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = c * 64 + 16 * kq + 4 * r;
                if (k < K) {
                    f32x4 v = f32x4{acc[c][0][r], acc[c][1][r], acc[c][2][r], acc[c][3][r]};
                    if (!DW) v -= gh * *reinterpret_cast<const f32x4*>(wt_row + k);
                    *reinterpret_cast<f32x4*>(out + (size_t)x * K + k) = v;
                }
            }
    }
}

// dw = slab 0 + slab 1 + ... in share order
__global__ __launch_bounds__(kThreads) void head_loss_dw_combine_kernel(const float* __restrict__ slabs, size_t slab_floats, int split, size_t n4, float* __restrict__ dw) {
    const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n4) return;
    f32x4 v = *reinterpret_cast<const f32x4*>(slabs + i * 4);
    for (int s = 1; s < split; ++s) v += *reinterpret_cast<const f32x4*>(slabs + (size_t)s * slab_floats + i * 4);
    *reinterpret_cast<f32x4*>(dw + i * 4) = v;
}

int check_common(const char* who, const void* h, const void* w, const void* target, int64_t rows, int N, int K, float eps) {
    if (!shape_ok(rows, N, K)) {
        paella_set_error("%s: unsupported shape rows=%lld N=%d K=%d (rows in 1...2^24, N a multiple of 16 in 16...65536, K a multiple of 16 in 16...256)", who,
                         (long long)rows, N, K);
        return PAELLA_ERR_ARG;
    }
    if (!(eps >= 0.f && eps < 1.f)) {  // false for NaN as well
        paella_set_error("%s: label_smoothing must lie in [0, 1) (got %g)", who, (double)eps);
        return PAELLA_ERR_ARG;
    }
    return check_required(who, h && w && target, "h, w and target");
}

int check_ws(const char* who, const Plan& p, const void* ws, size_t ws_bytes) {
    return check_workspace_size(who, ws, ws_bytes, p.bytes, "paella_head_loss_workspace_bytes asks for");
}

template <bool DW>
int launch_bwd(const float* h, const float* w, const int64_t* target, const float* lse, const float* corr, const float* grad, int64_t rows, int N, int K, const Plan& p,
               float eps, float* out, size_t slab_floats, hipStream_t st) {
    const size_t lds = (size_t)(2 * (kTile * (K + 4) + kTile) + kTile * kPStride) * sizeof(float);
    const unsigned grid = DW ? (unsigned)(p.tiles_n * p.split) : (unsigned)p.tiles_m;
    const int split = DW ? p.split : 1;
#define PAELLA_HEAD_BWD(KC_)                                                                                                                                    \
    {                                                                                                                                                           \
        auto kern = &head_loss_bwd_kernel<DW, KC_>;                                                                                                             \
        if (lds > 48 * 1024) HIP_CHECK_RET(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));     \
        hipLaunchKernelGGL(kern, dim3(grid), dim3(kThreads), lds, st, h, w, target, lse, corr, grad, rows, N, K, p.tiles_n, p.tiles_m, split, eps, out, slab_floats); \
    }
    switch ((K + 63) / 64) {
        case 1: PAELLA_HEAD_BWD(1) break;
        case 2: PAELLA_HEAD_BWD(2) break;
        case 3: PAELLA_HEAD_BWD(3) break;
        default: PAELLA_HEAD_BWD(4) break;
    }
#undef PAELLA_HEAD_BWD
    LAUNCH_CHECK_RET();
    return PAELLA_OK;
}

}  // namespace

extern "C" size_t paella_head_loss_workspace_bytes(int64_t rows, int N, int K) {
    if (!shape_ok(rows, N, K)) return 0;
    return make_plan(rows, N, K).bytes;
}

extern "C" int paella_head_loss_forward(const float* h, const float* w, const int64_t* target, int64_t rows, int N, int K, float label_smoothing, float* loss_out,
                                        float* lse_out, int* argmax_out, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "head_loss_forward";
    int rc = check_common(who, h, w, target, rows, N, K, label_smoothing);
    if (rc == PAELLA_OK) rc = check_required(who, loss_out && lse_out, "loss_out and lse_out");
    if (rc != PAELLA_OK) return rc;
    const Plan p = make_plan(rows, N, K);
    rc = check_ws(who, p, ws, ws_bytes);
    if (rc != PAELLA_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    float* tgt_ws = (float*)((char*)ws + p.tgt_off);
    float* part = (float*)((char*)ws + p.part_off);
    hipLaunchKernelGGL(head_loss_fwd_kernel, dim3((unsigned)(p.tiles_m * p.tiles_n)), dim3(kThreads), 0, st, h, w, target, rows, N, K, p.tiles_n, label_smoothing, part,
                       tgt_ws, loss_out, lse_out, argmax_out, (const float*)nullptr, (float*)nullptr);
    LAUNCH_CHECK_RET();
    if (p.tiles_n > 1) {
        hipLaunchKernelGGL(head_loss_finalize_kernel, dim3((unsigned)((rows + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, part, tgt_ws, target, rows, N, p.tiles_n,
                           label_smoothing, loss_out, lse_out, argmax_out);
        LAUNCH_CHECK_RET();
    }
    return PAELLA_OK;
}

extern "C" int paella_head_loss_backward(const float* h, const float* w, const int64_t* target, const float* lse, const float* grad_loss, int64_t rows, int N, int K,
                                         float label_smoothing, float* dh_out, float* dw_out, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "head_loss_backward";
    int rc = check_common(who, h, w, target, rows, N, K, label_smoothing);
    if (rc == PAELLA_OK) rc = check_required(who, lse && grad_loss, "lse and grad_loss");
    if (rc != PAELLA_OK) return rc;
    const Plan p = make_plan(rows, N, K);
    rc = check_ws(who, p, ws, ws_bytes);
    if (rc != PAELLA_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (!dh_out && !dw_out) return PAELLA_OK;
    float* corr = (float*)((char*)ws + p.corr_off);
    float* npart = (float*)((char*)ws + p.npart_off);
    float* slabs = (float*)((char*)ws + p.slab_off);
    hipLaunchKernelGGL(head_loss_fwd_kernel, dim3((unsigned)(p.tiles_m * p.tiles_n)), dim3(kThreads), 0, st, h, w, target, rows, N, K, p.tiles_n, label_smoothing, npart,
                       (float*)nullptr, (float*)nullptr, (float*)nullptr, (int*)nullptr, lse, corr);
    LAUNCH_CHECK_RET();
    if (p.tiles_n > 1) {
        hipLaunchKernelGGL(head_loss_renorm_kernel, dim3((unsigned)((rows + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, (const float*)npart, rows, p.tiles_n, corr);
        LAUNCH_CHECK_RET();
    }
    if (dh_out) {
        const int r = launch_bwd<false>(h, w, target, lse, corr, grad_loss, rows, N, K, p, label_smoothing, dh_out, 0, st);
        if (r != PAELLA_OK) return r;
    }
    if (dw_out) {
        const size_t slab_floats = p.slab_bytes / sizeof(float);
        float* dst = p.split > 1 ? slabs : dw_out;
        const int r = launch_bwd<true>(h, w, target, lse, corr, grad_loss, rows, N, K, p, label_smoothing, dst, slab_floats, st);
        if (r != PAELLA_OK) return r;
        if (p.split > 1) {
            const size_t n4 = (size_t)N * K / 4;
            hipLaunchKernelGGL(head_loss_dw_combine_kernel, dim3((unsigned)((n4 + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, (const float*)slabs, slab_floats, p.split,
                               n4, dw_out);
            LAUNCH_CHECK_RET();
        }
    }
    return PAELLA_OK;
}
