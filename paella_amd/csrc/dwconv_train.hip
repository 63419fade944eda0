// Training ResBlock front: depthwise Conv2d(k=3, zero padding, groups=C) + bias -> LayerNorm2d(C, no affine) as ONE op, forward and backward (the front of
// `training._res_block`).  NHWC fp32; with a skip the convolution is the grouped 2C -> C one over cat([x, skip]) and the two halves are read (and their gradients
// written) in place, never concatenated: output channel g reads concatenated channels J g + j, concatenated channel cc lives in x (cc < C) or in skip at cc - C.
// The weight arrives and its gradient leaves in the parameter's own layout [C, J, 3, 3].
//
//   forward : a = conv(xcat, w) + bias,  mean / var over C two-pass (as dwconv.hip),  rstd = 1 / sqrt(var + eps),  y = (a - mean) rstd;  rstd [B H W] is kept
//   backward: c1 = mean_c dy,  c2 = mean_c(dy y),  da = rstd (dy - c1 - y c2)
//             dbias_c = sum_pos da,  dw[c][j][tap] = sum_pos da[pos][c] xcat[pos + tap][J c + j],  dxcat[pos][J c + j] = sum_tap da[pos - tap][c] w[c][j][tap]
//
// Launches.  Forward: the weights repacked to [j][tap][C] in the workspace (so that every tap is one coalesced row read), then dwconv.hip's kernel shape -- one
// 256-thread workgroup per position, zero padding as a 0/1 factor on the tap, two block reductions.  Backward: (1) da into the workspace, one WAVE per position;
// (2) dx / dskip, one thread per 16-byte vector of da channels and a run of 8 positions along a row, its 36 J weights read once, contiguous in the parameter layout;
// (3) dw / dbias: one thread per (channel, tap) over a STRIP of positions, its sums carried in fp64, one fp32 partial per (strip, element) in the parameter layout;
// (4) the partials in ASCENDING strip order.  A tensor of one strip writes (3) straight into dw / dbias.
// No float atomics, no tickets: every combine is a launch.  The strips depend on (B, H, W, C, J) only (make_plan), never on the device; y, da, dx and dskip of a
// position depend on its own sample only, so a sample's bits depend neither on its index nor on the batch around it.
#include "train_common.h"

namespace {

using namespace train;

constexpr int kThreads = 256;
constexpr int kSumThreads = 64;   // (3): channels per workgroup (x 9 taps)
constexpr int kMaxStrips = 1024;  // bounds the finalize loop of a long tensor
constexpr int kRun = 8;           // (2): positions along a row per thread
constexpr int kMaxC = 8192, kMaxCSkip = 4096;

bool shape_ok(int B, int H, int W, int C, int has_skip) {
    if (B < 1 || H < 1 || W < 1 || (int64_t)B * H * W > 0x7fffffffll) return false;
    if (C < 4 || (C & 3) || C > kMaxC) return false;
    if (has_skip && ((C & 7) || C > kMaxCSkip)) return false;
    return true;
}

struct Plan {
    int J, rows_per_strip, strips;
    int64_t N;
    size_t pw_off, pb_off, fwd_bytes, bwd_bytes;  // da at 0 (backward); the repacked weights at 0 (forward)
};

// A strip is at least 8 (9 J + 1) positions, and there are two or more only when N exceeds one: strips (9 J + 1) < 2 N (9 J + 1) / rows <= N / 4, so the
// partials stay under a quarter of one activation tensor.  One strip needs no partials at all.
Plan make_plan(int B, int H, int W, int C, int has_skip) {
    Plan p = {};
    p.J = has_skip ? 2 : 1;
    p.N = (int64_t)B * H * W;
    const Strips s = plan_strips(p.N, 8 * (9 * p.J + 1), kMaxStrips);
    p.rows_per_strip = s.rows;
    p.strips = s.count;
    const size_t da = align256((size_t)p.N * C * sizeof(float));
    const size_t pw = p.strips > 1 ? align256((size_t)p.strips * C * 9 * p.J * sizeof(float)) : 0;
    const size_t pb = p.strips > 1 ? align256((size_t)p.strips * C * sizeof(float)) : 0;
    p.pw_off = da;
    p.pb_off = da + pw;
    p.bwd_bytes = da + pw + pb;
    p.fwd_bytes = align256((size_t)9 * p.J * C * sizeof(float));
    return p;
}

__device__ __forceinline__ f32x4 ldq(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

__device__ __forceinline__ float block_sum_256(float v, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) red[wave] = v;
    __syncthreads();
    const float s = (red[0] + red[1]) + (red[2] + red[3]);
    __syncthreads();
    return s;
}

// w [C, J, 9] (the parameter) -> wp [J, 9, C]
__global__ __launch_bounds__(kThreads) void dwconv_train_repack_kernel(const float* __restrict__ w, float* __restrict__ wp, int C, int J) {
    const int i = blockIdx.x * kThreads + threadIdx.x;  // index into wp
    if (i >= 9 * J * C) return;
    const int jt = i / C, c = i - jt * C;
    wp[i] = w[c * 9 * J + jt];
}

// Forward: dwconv.hip's dwconv_ln_block_kernel in its arithmetic (tap order, two-pass statistics, the block sums), plus the position's rstd.
template <int NV, bool SKIP>
__global__ __launch_bounds__(kThreads) void dwconv_ln_train_fwd_kernel(const float* __restrict__ x, const float* __restrict__ skip, const float* __restrict__ w,
                                                                       const float* __restrict__ bias, float* __restrict__ y, float* __restrict__ rstd_out, int H, int W,
                                                                       int C, float eps, FastDiv dW, FastDiv dH) {
    __shared__ float red[4];
    const int64_t pos = blockIdx.x;
    const int C4 = C >> 2;
    const unsigned prow = fast_div((unsigned)blockIdx.x, dW);  // b * H + y
    const int xx = (int)((unsigned)blockIdx.x - prow * (unsigned)W);
    const int yy = (int)(prow - fast_div(prow, dH) * (unsigned)H);
    const int64_t img = pos - (int64_t)yy * W - xx;  // row index of (b, 0, 0)
    int c4s[NV];
    bool live[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c4 = threadIdx.x + i * 256;
        live[i] = c4 < C4;
        c4s[i] = live[i] ? c4 : C4 - 1;
    }
    f32x4 acc[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) acc[i] = ldq(bias + c4s[i] * 4);
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int sy = yy + ky - 1;
        const int syc = min(max(sy, 0), H - 1);
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int sx = xx + kx - 1;
            const int sxc = min(max(sx, 0), W - 1);
            const float keep = (sy == syc && sx == sxc) ? 1.0f : 0.0f;  // zero padding
            const int64_t npos = img + (int64_t)syc * W + sxc;
            const int tap = ky * 3 + kx;
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                if (!SKIP) {
                    acc[i] += ldq(x + npos * C + c4s[i] * 4) * (ldq(w + tap * C + c4s[i] * 4) * keep);
                } else {
                    const int cc = 8 * c4s[i];  // out channels 4 c4 ... + 3 read cat channels 2g ... 2g + 7
                    const float* src = cc < C ? (x + npos * C + cc) : (skip + npos * C + (cc - C));
                    const f32x4 e0 = ldq(src), e1 = ldq(src + 4);
                    const f32x4 w0 = ldq(w + tap * C + c4s[i] * 4) * keep;
                    const f32x4 w1 = ldq(w + (9 + tap) * C + c4s[i] * 4) * keep;
                    acc[i][0] += e0[0] * w0[0] + e0[1] * w1[0];
                    acc[i][1] += e0[2] * w0[1] + e0[3] * w1[1];
                    acc[i][2] += e1[0] * w0[2] + e1[1] * w1[2];
                    acc[i][3] += e1[2] * w0[3] + e1[3] * w1[3];
                }
            }
        }
    }
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i)
        if (live[i]) s += (acc[i][0] + acc[i][1]) + (acc[i][2] + acc[i][3]);
    const float mean = block_sum_256(s, red) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i)
        if (live[i]) {
            f32x4 d = acc[i] - mean;
            d = d * d;
            q += (d[0] + d[1]) + (d[2] + d[3]);
        }
    const float rstd = 1.0f / sqrtf(block_sum_256(q, red) / (float)C + eps);
    if (threadIdx.x == 0) rstd_out[pos] = rstd;
#pragma unroll
    for (int i = 0; i < NV; ++i)
        if (live[i]) *reinterpret_cast<f32x4*>(y + pos * C + (threadIdx.x + i * 256) * 4) = (acc[i] - mean) * rstd;
}

// Backward (1): da = rstd (dy - c1 - y c2).  One wave per position, a lane takes 16-byte vectors lane, lane + 64, ...; the two sums by an xor butterfly.
__global__ __launch_bounds__(kThreads) void dwconv_ln_train_da_kernel(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ rstd,
                                                                      float* __restrict__ da, int64_t N, int C) {
    const int lane = threadIdx.x & 63;
    const int64_t pos = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (pos >= N) return;
    const int C4 = C >> 2;
    const float* dyp = dy + pos * C;
    const float* yp = y + pos * C;
    float s1 = 0.f, s2 = 0.f;
    for (int c4 = lane; c4 < C4; c4 += 64) {
        const f32x4 g = ldq(dyp + c4 * 4), v = ldq(yp + c4 * 4);
        s1 += (g[0] + g[1]) + (g[2] + g[3]);
        s2 += (g[0] * v[0] + g[1] * v[1]) + (g[2] * v[2] + g[3] * v[3]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        s1 += __shfl_xor(s1, o, 64);
        s2 += __shfl_xor(s2, o, 64);
    }
    const float c1 = s1 / (float)C, c2 = s2 / (float)C, r = rstd[pos];
    for (int c4 = lane; c4 < C4; c4 += 64) {
        const f32x4 g = ldq(dyp + c4 * 4), v = ldq(yp + c4 * 4);
        *reinterpret_cast<f32x4*>(da + pos * C + c4 * 4) = ((g - c1) - v * c2) * r;
    }
}

// Backward (2): dxcat[pos][J c + j] = sum_tap da[pos - tap][c] w[c][j][tap].  A workgroup is one run of up to kRun positions of one image row; a thread takes the
// da vectors t, t + 256, ... and reads its 4 channels' weights as 9 J contiguous 16-byte vectors of the parameter.  Taps in ascending (ky, kx), fp32 fma.
template <bool SKIP>
__global__ __launch_bounds__(kThreads) void dwconv_ln_train_dx_kernel(const float* __restrict__ da, const float* __restrict__ w, float* __restrict__ dx,
                                                                      float* __restrict__ dskip, int H, int W, int C, int nrun) {
    constexpr int J = SKIP ? 2 : 1;
    const int C4 = C >> 2;
    const unsigned row = blockIdx.x / (unsigned)nrun;  // b * H + y
    const int x0 = (int)(blockIdx.x - row * (unsigned)nrun) * kRun;
    const int x1 = min(W, x0 + kRun);
    const int yy = (int)(row % (unsigned)H);
    const int64_t rowpos = (int64_t)row * W;
    for (int c4 = threadIdx.x; c4 < C4; c4 += kThreads) {
        float* dst = dx;
        int cc = 4 * c4;
        if (SKIP) {
            cc = 8 * c4;
            if (cc >= C) {
                dst = dskip;
                cc -= C;
            }
        }
        if (!dst) continue;
        f32x4 wl[9 * J];
#pragma unroll
        for (int k = 0; k < 9 * J; ++k) wl[k] = ldq(w + (size_t)c4 * 36 * J + 4 * k);
        for (int xx = x0; xx < x1; ++xx) {
            float o[4 * J];
#pragma unroll
            for (int k = 0; k < 4 * J; ++k) o[k] = 0.f;
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int sy = yy - (ky - 1);
                const int syc = min(max(sy, 0), H - 1);
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    const int sx = xx - (kx - 1);
                    const int sxc = min(max(sx, 0), W - 1);
                    const bool in = sy == syc && sx == sxc;
                    f32x4 g = ldq(da + (rowpos + (int64_t)(syc - yy) * W + sxc) * C + c4 * 4);
                    if (!in) g = f32x4{0.f, 0.f, 0.f, 0.f};
                    const int tap = ky * 3 + kx;
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int j = 0; j < J; ++j) {
                            const int f = e * 9 * J + j * 9 + tap;
                            o[e * J + j] = fmaf(g[e], wl[f >> 2][f & 3], o[e * J + j]);
                        }
                }
            }
            float* p = dst + (rowpos + xx) * C + cc;
#pragma unroll
            for (int k = 0; k < J; ++k) *reinterpret_cast<f32x4*>(p + 4 * k) = f32x4{o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]};
        }
    }
}

// Backward (3): over the positions [p0, p1) of strip blockIdx.y, thread (c, tap): sum da[pos][c] xcat[pos + tap][J c + j] in fp64, positions ascending; the centre
// tap's thread also sums da[pos][c].  A workgroup is 64 channels x the 9 taps, one wave per tap (whether a tap is inside the image is wave-uniform): the strips
// are few, so the taps and the channels spread the work.  pw [strip][C][J][9] and pb [strip][C] are the partials, or dw / dbias themselves when there is one
// strip; a NULL one is not stored.
template <bool SKIP>
__global__ __launch_bounds__(kSumThreads * 9) void dwconv_ln_train_dw_kernel(const float* __restrict__ da, const float* __restrict__ x, const float* __restrict__ skip,
                                                                             float* __restrict__ pw, float* __restrict__ pb, int64_t N, int H, int W, int C,
                                                                             int rows_per_strip) {
    constexpr int J = SKIP ? 2 : 1;
    const int c = blockIdx.x * kSumThreads + threadIdx.x;
    if (c >= C) return;
    const int tap = threadIdx.y, ky = tap / 3, kx = tap - 3 * ky;
    const int64_t p0 = (int64_t)blockIdx.y * rows_per_strip;
    const int64_t p1 = min(N, p0 + rows_per_strip);
    int xx = (int)(p0 % W);
    int yy = (int)((p0 / W) % H);
    const float* src = x + c;
    if (SKIP) src = 2 * c < C ? x + 2 * c : skip + (2 * c - C);
    double acc0 = 0.0, acc1 = 0.0, accb = 0.0;
#pragma unroll 4
    for (int64_t p = p0; p < p1; ++p) {
        const double g = (double)da[p * C + c];
        const int sy = yy + ky - 1, sx = xx + kx - 1;
        const int syc = min(max(sy, 0), H - 1), sxc = min(max(sx, 0), W - 1);
        const bool in = sy == syc && sx == sxc;
        const float* q = src + (p + (int64_t)(syc - yy) * W + (sxc - xx)) * C;
        float v0 = q[0], v1 = 0.f;
        if (SKIP) v1 = q[1];
        if (!in) v0 = v1 = 0.f;  // zero padding: the clamped address is read, its value dropped
        acc0 = fma(g, (double)v0, acc0);
        if (SKIP) acc1 = fma(g, (double)v1, acc1);
        accb += g;
        if (++xx == W) {
            xx = 0;
            if (++yy == H) yy = 0;
        }
    }
    if (pw) {
        float* o = pw + ((size_t)blockIdx.y * C + c) * 9 * J + tap;
        o[0] = (float)acc0;
        if (SKIP) o[9] = (float)acc1;
    }
    if (pb && tap == 4) pb[(size_t)blockIdx.y * C + c] = (float)accb;
}

// Backward (4): dw [C J 9] and dbias [C] = the partials in ascending strip order, in fp64; one thread per element of either
__global__ __launch_bounds__(kThreads) void dwconv_ln_train_dw_finalize_kernel(const float* __restrict__ pw, const float* __restrict__ pb, int strips, int nw, int C,
                                                                               float* __restrict__ dw, float* __restrict__ dbias) {
    int i = blockIdx.x * kThreads + threadIdx.x;
    const float* part = pw;
    float* out = dw;
    int n = nw;
    if (i >= nw) {
        i -= nw;
        part = pb;
        out = dbias;
        n = C;
        if (i >= C) return;
    }
    if (!out) return;
    double s = 0.0;
#pragma unroll 8  // the loads of eight strips in flight; the additions keep their order
    for (int st = 0; st < strips; ++st) s += (double)part[(size_t)st * n + i];
    out[i] = (float)s;
}

int check_shape(const char* who, int B, int H, int W, int C, int has_skip) {
    if (shape_ok(B, H, W, C, has_skip)) return PAELLA_OK;
    paella_set_error("%s: unsupported shape B=%d H=%d W=%d C=%d%s (B, H, W >= 1 with B H W <= 2^31 - 1; C a multiple of 4 in 4...8192, with a skip a multiple of 8 in 8...4096)",
                     who, B, H, W, C, has_skip ? " with a skip" : "");
    return PAELLA_ERR_ARG;
}

int check_ws(const char* who, const void* ws, size_t ws_bytes, size_t need) {
    return check_workspace(who, ws, ws_bytes, need, "this call needs", " (paella_dwconv_ln_train_workspace_bytes covers both directions)");
}

}  // namespace

extern "C" size_t paella_dwconv_ln_train_workspace_bytes(int B, int H, int W, int C, int has_skip) {
    if (!shape_ok(B, H, W, C, has_skip)) return 0;
    const Plan p = make_plan(B, H, W, C, has_skip);
    return p.bwd_bytes > p.fwd_bytes ? p.bwd_bytes : p.fwd_bytes;
}

extern "C" int paella_dwconv_ln_train_forward(const float* x, const float* skip, const float* w, const float* bias, int B, int H, int W, int C, float eps, float* y,
                                              float* rstd, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "dwconv_ln_train_forward";
    int rc = check_shape(who, B, H, W, C, skip != nullptr);
    if (rc != PAELLA_OK) return rc;
    if (!(eps > 0.f) || !(eps < 1e30f)) {  // false for NaN as well
        paella_set_error("%s: eps must be positive and finite (got %g)", who, (double)eps);
        return PAELLA_ERR_ARG;
    }
    rc = check_required(who, x && w && bias && y && rstd, "x, w, bias, y and rstd");
    if (rc == PAELLA_OK) rc = check_tensors_aligned16(who, x, skip, w, bias, y, rstd);
    if (rc != PAELLA_OK) return rc;
    const Plan pl = make_plan(B, H, W, C, skip != nullptr);
    rc = check_ws(who, ws, ws_bytes, pl.fwd_bytes);
    if (rc != PAELLA_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    float* wp = (float*)ws;
    hipLaunchKernelGGL(dwconv_train_repack_kernel, dim3((unsigned)((9 * pl.J * C + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, w, wp, C, pl.J);
    LAUNCH_CHECK_RET();
    const int nv = (C / 4 + 255) / 256;
    const dim3 grid((unsigned)pl.N), block(kThreads);
    const FastDiv dW = fast_div_of((unsigned)W), dH = fast_div_of((unsigned)H);
#define DWT_LAUNCH(NVv)                                                                                                                                          \
    do {                                                                                                                                                         \
        if (skip) hipLaunchKernelGGL((dwconv_ln_train_fwd_kernel<NVv, true>), grid, block, 0, st, x, skip, (const float*)wp, bias, y, rstd, H, W, C, eps, dW, dH); \
        else hipLaunchKernelGGL((dwconv_ln_train_fwd_kernel<NVv, false>), grid, block, 0, st, x, skip, (const float*)wp, bias, y, rstd, H, W, C, eps, dW, dH);     \
    } while (0)
    if (nv <= 1) DWT_LAUNCH(1);
    else if (nv <= 2) DWT_LAUNCH(2);
    else if (nv <= 4) DWT_LAUNCH(4);
    else hipLaunchKernelGGL((dwconv_ln_train_fwd_kernel<8, false>), grid, block, 0, st, x, skip, (const float*)wp, bias, y, rstd, H, W, C, eps, dW, dH);  // (a skip stops at 4096)
#undef DWT_LAUNCH
    LAUNCH_CHECK_RET();
    return PAELLA_OK;
}

extern "C" int paella_dwconv_ln_train_backward(const float* x, const float* skip, const float* w, const float* y, const float* rstd, const float* dy, int B, int H, int W,
                                               int C, float* dx, float* dskip, float* dw, float* dbias, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "dwconv_ln_train_backward";
    int rc = check_shape(who, B, H, W, C, skip != nullptr);
    if (rc == PAELLA_OK) rc = check_required(who, x && w && y && rstd && dy, "x, w, y, rstd and dy");
    if (rc != PAELLA_OK) return rc;
    if (dskip && !skip) {
        paella_set_error("%s: dskip without a skip", who);
        return PAELLA_ERR_ARG;
    }
    rc = check_tensors_aligned16(who, x, skip, w, y, rstd, dy, dx, dskip, dw, dbias);
    if (rc != PAELLA_OK) return rc;
    const Plan pl = make_plan(B, H, W, C, skip != nullptr);
    rc = check_ws(who, ws, ws_bytes, pl.bwd_bytes);
    if (rc != PAELLA_OK) return rc;
    if (!dx && !dskip && !dw && !dbias) return PAELLA_OK;
    hipStream_t st = (hipStream_t)stream;
    float* da = (float*)ws;
    hipLaunchKernelGGL(dwconv_ln_train_da_kernel, dim3((unsigned)((pl.N + 3) / 4)), dim3(kThreads), 0, st, dy, y, rstd, da, pl.N, C);
    LAUNCH_CHECK_RET();
    if (dx || dskip) {
        const int nrun = (W + kRun - 1) / kRun;
        const dim3 grid((unsigned)((int64_t)B * H * nrun));  // <= B H W
        if (skip) hipLaunchKernelGGL((dwconv_ln_train_dx_kernel<true>), grid, dim3(kThreads), 0, st, (const float*)da, w, dx, dskip, H, W, C, nrun);
        else hipLaunchKernelGGL((dwconv_ln_train_dx_kernel<false>), grid, dim3(kThreads), 0, st, (const float*)da, w, dx, dskip, H, W, C, nrun);
        LAUNCH_CHECK_RET();
    }
    if (dw || dbias) {
        const bool one = pl.strips == 1;
        float* pw = one ? dw : (dw ? (float*)((char*)ws + pl.pw_off) : nullptr);
        float* pb = one ? dbias : (dbias ? (float*)((char*)ws + pl.pb_off) : nullptr);
        const dim3 grid((unsigned)((C + kSumThreads - 1) / kSumThreads), (unsigned)pl.strips);
        if (skip) hipLaunchKernelGGL((dwconv_ln_train_dw_kernel<true>), grid, dim3(kSumThreads, 9), 0, st, (const float*)da, x, skip, pw, pb, pl.N, H, W, C, pl.rows_per_strip);
        else hipLaunchKernelGGL((dwconv_ln_train_dw_kernel<false>), grid, dim3(kSumThreads, 9), 0, st, (const float*)da, x, skip, pw, pb, pl.N, H, W, C, pl.rows_per_strip);
        LAUNCH_CHECK_RET();
        if (!one) {
            const int nw = 9 * pl.J * C;
            hipLaunchKernelGGL(dwconv_ln_train_dw_finalize_kernel, dim3((unsigned)((nw + C + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, (const float*)pw,
                               (const float*)pb, pl.strips, nw, C, dw, dbias);
            LAUNCH_CHECK_RET();
        }
    }
    return PAELLA_OK;
}
