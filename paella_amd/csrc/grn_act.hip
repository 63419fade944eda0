// Training MLP activation: GELU -> GlobalResponseNorm -> Dropout of an MLP's [B, P, 4c] pre-activation as ONE op, forward and backward (the middle of
// `training._channelwise`).  With h = gelu_erf(u) (the engine's exact-path GELU, so train and eval agree on the activation):
//
//   forward : G[b, c] = sqrt(sum_p h^2),  M[b] = mean_c G,  n = G / (M + 1e-6),  y = h (1 + gamma_c n) + beta_c,  z = keep y / (1 - p)
//   backward: dy = keep dz / (1 - p),  dbeta_c = sum_{b, p} dy,  S[b, c] = sum_p dy h,  dgamma_c = sum_b n S,  dn = gamma_c S,
//             dG = dn / (M + eps) - (sum_c' dn G) / (C (M + eps)^2),  dh = dy (1 + gamma_c n) + (G > 0 ? dG / G : 0) h,  du = dh (Phi(u) + u phi(u))
//
// h is never stored: every pass recomputes it from u, and the only tensor the forward leaves for the backward is G [B, C].  The dropout mask is never stored
// either: element e (flat index in [B, P, C]) takes word e & 3 of philox4x32(seed ^ kDropoutSalt, e >> 2, 0), one Philox call per 16-byte vector, and is kept
// iff u01_half_open(word) >= p; both directions regenerate it.  The seed arrives by value, or -- the *_seed_dev entry points, for a captured training step whose
// every replay must draw other masks -- as the address of a 64-bit device word the kernels load themselves: the drawing kernels take (key, seed_dev) and use
// key ^ *seed_dev, with key = the salt alone in that form and seed ^ salt (seed_dev = NULL) in the by-value form, so a word that holds s gives the bits of seed = s.
//
// Each direction is two passes over the tensor around small finalize launches.  A workgroup is 4 waves over 256 channels (one 16-byte vector per lane: a wave
// touches 1 KiB of a row) and a STRIP of rows of one sample; wave w takes rows w, w + 4, ... of the strip.
//   pass A  column sums over the strip (forward: h^2; backward: dy h and dy), carried in fp64 per lane, the four waves added in wave order through LDS, one fp32
//           partial per (sample, strip, channel)
//   finalize (one workgroup per sample) the partials in ASCENDING strip order, then what needs a sum over the channels (M; backward: sum_c dn G) by a fixed tree;
//           backward only: one more small launch adds the per-sample terms of dgamma / dbeta in ASCENDING sample order
//   pass B  the apply
// No float atomics, no tickets: every combine is a launch, in an order fixed by the shape.  The strip count is a function of (P, C) only (make_plan), never
// of the device or of the batch, so two runs and two devices give the same bits, and the arithmetic of a sample depends neither on its index b nor on B.
#include "gemm_device.h"
#include "philox.h"
#include "train_common.h"
#include <math.h>

namespace {

using namespace train;

constexpr int kThreads = 256;
constexpr int kWaves = 4;
constexpr int kFinalThreads = 1024; // the per-sample finalize launches: B workgroups only, so each is as wide as a workgroup gets
constexpr int kFinalWaves = kFinalThreads / 64;
constexpr int kVecPerBlock = 64;    // 16-byte vectors (4 channels each) across a workgroup: 256 channels
constexpr int kMinStripRows = 8;    // two rows per wave: the partials of one pass are at most an eighth of the tensor
constexpr int kMaxStrips = 1024;    // bounds the partials of a long sample (P = 2^20: 1024 rows per strip)
constexpr int kTargetBlocks = 256;  // workgroups per SAMPLE passes A and B aim at (one per CU of a 256-CU part) -- a constant, not a device query
constexpr int kMaxB = 65535, kMaxP = 1 << 20, kMaxC = 16384;
constexpr float kGrnEps = 1e-6f;
// key salt of the dropout stream, next to the renoise (0x5bd1e9955bd1e995) and start-token (0x9e3779b97f4a7c15) salts of tail.hip
constexpr uint64_t kDropoutSalt = 0xa0761d6478bd642full;

struct Plan {
    int C4, nblk_c, rows_per_strip, strips;
    size_t part1_off, ns_off, d_off, k_off, m_off, bytes;  // part0 at 0
};

bool shape_ok(int B, int P, int C) { return B >= 1 && B <= kMaxB && P >= 1 && P <= kMaxP && C >= 4 && C <= kMaxC && (C & 3) == 0; }

// Everything here depends on the shape only, and the strips on (P, C) only: the same sample always gets the same strips, hence the same summation order and the
// same bits, whatever the batch around it.  B multiplies the grid, so the target is met by one sample alone wherever P allows it.
Plan make_plan(int B, int P, int C) {
    Plan p = {};
    p.C4 = C >> 2;
    p.nblk_c = (p.C4 + kVecPerBlock - 1) / kVecPerBlock;
    const int want = (kTargetBlocks + p.nblk_c - 1) / p.nblk_c;  // strips that would reach the target
    const int target_rows = (P + want - 1) / want;
    const Strips s = plan_strips(P, target_rows > kMinStripRows ? target_rows : kMinStripRows, kMaxStrips);
    p.rows_per_strip = s.rows;
    p.strips = s.count;
    const size_t part = align256((size_t)B * p.strips * C * sizeof(float));
    const size_t tab = align256((size_t)B * C * sizeof(float));
    p.part1_off = part;
    p.ns_off = 2 * part;
    p.d_off = p.ns_off + tab;
    p.k_off = p.d_off + tab;
    p.m_off = p.k_off + tab;
    p.bytes = p.m_off + align256((size_t)B * sizeof(float));
    return p;
}

struct Geo { int P, C, C4, rows_per_strip, strips; };

// the multiplier of the 4 elements of vector `quad` (its index among the 16-byte vectors of [B, P, C]): 1 / (1 - p) where kept, 0 where dropped
template <bool DROP>
__device__ __forceinline__ f32x4 keep_scale(uint64_t key, uint64_t quad, float p_drop, float scale) {
    f32x4 m = f32x4{1.f, 1.f, 1.f, 1.f};
    if (DROP) {
        uint32_t w[4];
        philox4x32(key, quad, 0ull, w);
#pragma unroll
        for (int e = 0; e < 4; ++e) m[e] = u01_half_open(w[e]) >= p_drop ? scale : 0.f;
    }
    return m;
}

// sum of v over the kFinalThreads threads of a finalize workgroup, every thread receiving it: xor butterfly inside a wave, then the waves in wave order
__device__ __forceinline__ double block_sum(double v, double* red) {
#pragma unroll
    for (int x = 1; x < 64; x <<= 1) v += __shfl_xor(v, x, 64);
    __syncthreads();  // red may still be read from an earlier sum
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = red[0];
#pragma unroll
    for (int w = 1; w < kFinalWaves; ++w) t += red[w];
    return t;
}

// Pass A.  grid (channel blocks, strips, B).  Forward: part0 [B, strips, C] = sum over the strip of h^2.  Backward: part0 = sum of dy h, part1 = sum of dy.
template <bool BWD, bool DROP>
__global__ __launch_bounds__(kThreads) void grn_act_sums_kernel(const float* __restrict__ u, const float* __restrict__ dz, Geo g, float p_drop, float scale, uint64_t key,
                                                                const uint64_t* __restrict__ seed_dev, float* __restrict__ part0, float* __restrict__ part1) {
    __shared__ double red[BWD ? 2 : 1][kWaves - 1][kVecPerBlock][4];
    if (DROP && seed_dev) key ^= *seed_dev;  // uniform: one scalar load
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c4 = blockIdx.x * kVecPerBlock + lane;
    const int strip = blockIdx.y, b = blockIdx.z;
    const bool on = c4 < g.C4;
    const int p0 = strip * g.rows_per_strip;
    const int p1 = min(g.P, p0 + g.rows_per_strip);
    double s[4] = {0.0, 0.0, 0.0, 0.0}, d[4] = {0.0, 0.0, 0.0, 0.0};
    if (on) {
        const size_t row0 = (size_t)b * g.P;
#pragma unroll 2
        for (int p = p0 + wave; p < p1; p += kWaves) {
            const size_t q = (row0 + p) * g.C4 + c4;
            const f32x4 x = reinterpret_cast<const f32x4*>(u)[q];
            if (BWD) {
                const f32x4 gz = reinterpret_cast<const f32x4*>(dz)[q];
                const f32x4 m = keep_scale<DROP>(key, q, p_drop, scale);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float dy = m[e] > 0.f ? gz[e] * m[e] : 0.f;
                    s[e] = fma((double)dy, (double)gelu_erf(x[e]), s[e]);
                    d[e] += (double)dy;
                }
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const double h = (double)gelu_erf(x[e]);
                    s[e] = fma(h, h, s[e]);
                }
            }
        }
    }
    if (wave > 0) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            red[0][wave - 1][lane][e] = s[e];
            if constexpr (BWD) red[1][wave - 1][lane][e] = d[e];
        }
    }
    __syncthreads();
    if (wave == 0 && on) {
        f32x4 o0, o1;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            o0[e] = (float)(((s[e] + red[0][0][lane][e]) + red[0][1][lane][e]) + red[0][2][lane][e]);
            if constexpr (BWD) o1[e] = (float)(((d[e] + red[1][0][lane][e]) + red[1][1][lane][e]) + red[1][2][lane][e]);
        }
        const size_t o = ((size_t)b * g.strips + strip) * g.C4 + c4;
        reinterpret_cast<f32x4*>(part0)[o] = o0;
        if (BWD) reinterpret_cast<f32x4*>(part1)[o] = o1;
    }
}

// the strips of vector c4 of sample b in ascending order
__device__ __forceinline__ void strip_sum(const float* __restrict__ part, const Geo& g, int b, int c4, double (&s)[4]) {
    s[0] = s[1] = s[2] = s[3] = 0.0;
    const f32x4* q = reinterpret_cast<const f32x4*>(part) + (size_t)b * g.strips * g.C4 + c4;
#pragma unroll 8  // the loads of eight strips in flight; the additions keep their order
    for (int st = 0; st < g.strips; ++st) {
        const f32x4 v = q[(size_t)st * g.C4];
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] += (double)v[e];
    }
}

// Forward finalize, one workgroup per sample: gx [B, C] = G, mtab [B] = M + eps.
__global__ __launch_bounds__(kFinalThreads) void grn_act_fwd_finalize_kernel(const float* __restrict__ part, Geo g, float* __restrict__ gx, float* __restrict__ mtab) {
    __shared__ double red[kFinalWaves];
    const int b = blockIdx.x;
    double sum_g = 0.0;
    for (int c4 = threadIdx.x; c4 < g.C4; c4 += kFinalThreads) {
        double s[4];
        strip_sum(part, g, b, c4, s);
        f32x4 G;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            G[e] = (float)sqrt(s[e]);
            sum_g += (double)G[e];
        }
        reinterpret_cast<f32x4*>(gx)[(size_t)b * g.C4 + c4] = G;
    }
    const double tot = block_sum(sum_g, red);
    if (threadIdx.x == 0) mtab[b] = (float)(tot / (double)g.C + (double)kGrnEps);
}

// Backward finalize, one workgroup per sample: S and D = the partials in strip order; M and T = sum_c gamma_c S G by the tree; then per channel
// tab_k = (G > 0 ? dG / G : 0), tab_ns = n S (this sample's term of dgamma), tab_d = D (its term of dbeta), mtab = M + eps.
// tab_ns holds S between the two phases: every thread reads back what it wrote itself.
__global__ __launch_bounds__(kFinalThreads) void grn_act_bwd_finalize_kernel(const float* __restrict__ part0, const float* __restrict__ part1, const float* __restrict__ gamma,
                                                                        const float* __restrict__ gx, Geo g, float* tab_ns, float* __restrict__ tab_d,
                                                                        float* __restrict__ tab_k, float* __restrict__ mtab) {
    __shared__ double red[kFinalWaves];
    const int b = blockIdx.x;
    double sum_g = 0.0, sum_t = 0.0;
    for (int c4 = threadIdx.x; c4 < g.C4; c4 += kFinalThreads) {
        double s[4], d[4];
        strip_sum(part0, g, b, c4, s);
        strip_sum(part1, g, b, c4, d);
        const f32x4 G = reinterpret_cast<const f32x4*>(gx)[(size_t)b * g.C4 + c4];
        const f32x4 ga = reinterpret_cast<const f32x4*>(gamma)[c4];
        f32x4 S, D;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            S[e] = (float)s[e];
            D[e] = (float)d[e];
            sum_g += (double)G[e];
            sum_t += (double)ga[e] * (double)S[e] * (double)G[e];
        }
        reinterpret_cast<f32x4*>(tab_ns)[(size_t)b * g.C4 + c4] = S;
        reinterpret_cast<f32x4*>(tab_d)[(size_t)b * g.C4 + c4] = D;
    }
    const double tot_g = block_sum(sum_g, red);
    const double tot_t = block_sum(sum_t, red);
    const float mp = (float)(tot_g / (double)g.C + (double)kGrnEps);
    if (threadIdx.x == 0) mtab[b] = mp;
    const double second = tot_t / ((double)g.C * (double)mp * (double)mp);
    for (int c4 = threadIdx.x; c4 < g.C4; c4 += kFinalThreads) {
        const f32x4 S = reinterpret_cast<const f32x4*>(tab_ns)[(size_t)b * g.C4 + c4];
        const f32x4 G = reinterpret_cast<const f32x4*>(gx)[(size_t)b * g.C4 + c4];
        const f32x4 ga = reinterpret_cast<const f32x4*>(gamma)[c4];
        f32x4 k, ns;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double dG = (double)ga[e] * (double)S[e] / (double)mp - second;
            k[e] = G[e] > 0.f ? (float)(dG / (double)G[e]) : 0.f;
            ns[e] = (G[e] / mp) * S[e];
        }
        reinterpret_cast<f32x4*>(tab_k)[(size_t)b * g.C4 + c4] = k;
        reinterpret_cast<f32x4*>(tab_ns)[(size_t)b * g.C4 + c4] = ns;
    }
}

// dgamma_c = sum_b tab_ns[b, c], dbeta_c = sum_b tab_d[b, c], in ascending b; one thread per 16-byte vector of channels
__global__ __launch_bounds__(kThreads) void grn_act_param_grad_kernel(const float* __restrict__ tab_ns, const float* __restrict__ tab_d, int B, int C4,
                                                                      float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int c4 = blockIdx.x * kThreads + threadIdx.x;
    if (c4 >= C4) return;
    for (int t = 0; t < 2; ++t) {
        const float* tab = t ? tab_d : tab_ns;
        float* out = t ? dbeta : dgamma;
        if (!out) continue;
        double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
        for (int b = 0; b < B; ++b) {
            const f32x4 v = reinterpret_cast<const f32x4*>(tab)[(size_t)b * C4 + c4];
#pragma unroll
            for (int e = 0; e < 4; ++e) s[e] += (double)v[e];
        }
        reinterpret_cast<f32x4*>(out)[c4] = f32x4{(float)s[0], (float)s[1], (float)s[2], (float)s[3]};
    }
}

// Pass B.  grid as pass A.  Forward: z.  Backward: du (tab_k from the backward finalize).
template <bool BWD, bool DROP>
__global__ __launch_bounds__(kThreads) void grn_act_apply_kernel(const float* __restrict__ u, const float* __restrict__ dz, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, const float* __restrict__ gx, const float* __restrict__ mtab,
                                                                 const float* __restrict__ tab_k, Geo g, float p_drop, float scale, uint64_t key,
                                                                 const uint64_t* __restrict__ seed_dev, float* __restrict__ out) {
    if (DROP && seed_dev) key ^= *seed_dev;  // uniform: one scalar load
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c4 = blockIdx.x * kVecPerBlock + lane;
    const int strip = blockIdx.y, b = blockIdx.z;
    if (c4 >= g.C4) return;
    const int p0 = strip * g.rows_per_strip;
    const int p1 = min(g.P, p0 + g.rows_per_strip);
    const f32x4 ga = reinterpret_cast<const f32x4*>(gamma)[c4];
    const f32x4 G = reinterpret_cast<const f32x4*>(gx)[(size_t)b * g.C4 + c4];
    const float mp = mtab[b];
    f32x4 a, k = f32x4{0.f, 0.f, 0.f, 0.f}, be = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) a[e] = fmaf(ga[e], G[e] / mp, 1.f);
    if (BWD) k = reinterpret_cast<const f32x4*>(tab_k)[(size_t)b * g.C4 + c4];
    else be = reinterpret_cast<const f32x4*>(beta)[c4];
    const size_t row0 = (size_t)b * g.P;
#pragma unroll 2
    for (int p = p0 + wave; p < p1; p += kWaves) {
        const size_t q = (row0 + p) * g.C4 + c4;
        const f32x4 x = reinterpret_cast<const f32x4*>(u)[q];
        f32x4 gz = f32x4{0.f, 0.f, 0.f, 0.f};
        if (BWD) gz = reinterpret_cast<const f32x4*>(dz)[q];
        const f32x4 m = keep_scale<DROP>(key, q, p_drop, scale);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float h = gelu_erf(x[e]);
            if (BWD) {
                const float dy = m[e] > 0.f ? gz[e] * m[e] : 0.f;
                const float dh = fmaf(dy, a[e], k[e] * h);
                // Phi(u) = h / u: h = u Phi(u) to one rounding, so the quotient is Phi to two -- the absolute accuracy gelu_erf itself has; Phi(0) = 1/2
                const float cdf = fabsf(x[e]) > 1e-30f ? h / x[e] : 0.5f;
                const float pdf = expf(-0.5f * x[e] * x[e]) * 0.39894228040143267794f;
                o[e] = dh * fmaf(x[e], pdf, cdf);
            } else {
                const float y = fmaf(h, a[e], be[e]);
                o[e] = DROP ? (m[e] > 0.f ? y * m[e] : 0.f) : y;
            }
        }
        reinterpret_cast<f32x4*>(out)[q] = o;
    }
}

int check_common(const char* who, float p_drop, const Plan& pl, const void* ws, size_t ws_bytes) {
    if (!(p_drop >= 0.f && p_drop < 1.f)) {  // false for NaN as well
        paella_set_error("%s: p_drop must lie in [0, 1) (got %g)", who, (double)p_drop);
        return PAELLA_ERR_ARG;
    }
    return check_workspace(who, ws, ws_bytes, pl.bytes, "paella_grn_act_workspace_bytes asks for");
}

int check_shape(const char* who, int B, int P, int C) {
    if (shape_ok(B, P, C)) return PAELLA_OK;
    paella_set_error("%s: unsupported shape B=%d P=%d C=%d (B in 1...65535, P in 1...2^20, C a multiple of 4 in 4...16384)", who, B, P, C);
    return PAELLA_ERR_ARG;
}

int forward_impl(const char* who, const float* u, const float* gamma, const float* beta, int B, int P, int C, float p_drop, uint64_t seed, const uint64_t* seed_dev,
                 bool by_pointer, float* z, float* gx, void* ws, size_t ws_bytes, void* stream) {
    int rc = check_shape(who, B, P, C);
    if (rc == PAELLA_OK) rc = check_required(who, u && gamma && beta && z && gx, "u, gamma, beta, z and gx");
    if (rc == PAELLA_OK) rc = check_tensors_aligned16(who, u, gamma, beta, z, gx);
    if (rc != PAELLA_OK) return rc;
    const Plan pl = make_plan(B, P, C);
    rc = check_common(who, p_drop, pl, ws, ws_bytes);
    if (rc == PAELLA_OK && by_pointer) rc = check_seed_dev(who, p_drop, seed_dev);
    if (rc != PAELLA_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Geo g = {P, C, pl.C4, pl.rows_per_strip, pl.strips};
    float* part0 = (float*)ws;
    float* mtab = (float*)((char*)ws + pl.m_off);
    const dim3 grid((unsigned)pl.nblk_c, (unsigned)pl.strips, (unsigned)B);
    const float scale = 1.0f / (1.0f - p_drop);
    const uint64_t key = seed ^ kDropoutSalt;  // by pointer: seed = 0, the kernels add the word
    hipLaunchKernelGGL((grn_act_sums_kernel<false, false>), grid, dim3(kThreads), 0, st, u, (const float*)nullptr, g, 0.f, 1.f, 0ull, (const uint64_t*)nullptr, part0, (float*)nullptr);
    LAUNCH_CHECK_RET();
    hipLaunchKernelGGL(grn_act_fwd_finalize_kernel, dim3((unsigned)B), dim3(kFinalThreads), 0, st, (const float*)part0, g, gx, mtab);
    LAUNCH_CHECK_RET();
    if (p_drop > 0.f)
        hipLaunchKernelGGL((grn_act_apply_kernel<false, true>), grid, dim3(kThreads), 0, st, u, (const float*)nullptr, gamma, beta, (const float*)gx, (const float*)mtab,
                           (const float*)nullptr, g, p_drop, scale, key, seed_dev, z);
    else
        hipLaunchKernelGGL((grn_act_apply_kernel<false, false>), grid, dim3(kThreads), 0, st, u, (const float*)nullptr, gamma, beta, (const float*)gx, (const float*)mtab,
                           (const float*)nullptr, g, 0.f, 1.f, 0ull, (const uint64_t*)nullptr, z);
    LAUNCH_CHECK_RET();
    return PAELLA_OK;
}

int backward_impl(const char* who, const float* u, const float* gamma, const float* gx, const float* dz, int B, int P, int C, float p_drop, uint64_t seed,
                  const uint64_t* seed_dev, bool by_pointer, float* du, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream) {
    int rc = check_shape(who, B, P, C);
    if (rc == PAELLA_OK) rc = check_required(who, u && gamma && gx && dz, "u, gamma, gx and dz");
    if (rc == PAELLA_OK) rc = check_tensors_aligned16(who, u, gamma, gx, dz, du, dgamma, dbeta);
    if (rc != PAELLA_OK) return rc;
    const Plan pl = make_plan(B, P, C);
    rc = check_common(who, p_drop, pl, ws, ws_bytes);
    if (rc == PAELLA_OK && by_pointer) rc = check_seed_dev(who, p_drop, seed_dev);
    if (rc != PAELLA_OK) return rc;
    if (!du && !dgamma && !dbeta) return PAELLA_OK;
    hipStream_t st = (hipStream_t)stream;
    const Geo g = {P, C, pl.C4, pl.rows_per_strip, pl.strips};
    float* part0 = (float*)ws;
    float* part1 = (float*)((char*)ws + pl.part1_off);
    float* tab_ns = (float*)((char*)ws + pl.ns_off);
    float* tab_d = (float*)((char*)ws + pl.d_off);
    float* tab_k = (float*)((char*)ws + pl.k_off);
    float* mtab = (float*)((char*)ws + pl.m_off);
    const dim3 grid((unsigned)pl.nblk_c, (unsigned)pl.strips, (unsigned)B);
    const bool drop = p_drop > 0.f;
    const float scale = 1.0f / (1.0f - p_drop);
    const uint64_t key = seed ^ kDropoutSalt;  // by pointer: seed = 0, the kernels add the word
    if (drop) hipLaunchKernelGGL((grn_act_sums_kernel<true, true>), grid, dim3(kThreads), 0, st, u, dz, g, p_drop, scale, key, seed_dev, part0, part1);
    else hipLaunchKernelGGL((grn_act_sums_kernel<true, false>), grid, dim3(kThreads), 0, st, u, dz, g, 0.f, 1.f, 0ull, (const uint64_t*)nullptr, part0, part1);
    LAUNCH_CHECK_RET();
    hipLaunchKernelGGL(grn_act_bwd_finalize_kernel, dim3((unsigned)B), dim3(kFinalThreads), 0, st, (const float*)part0, (const float*)part1, gamma, gx, g, tab_ns, tab_d, tab_k,
                       mtab);
    LAUNCH_CHECK_RET();
    if (dgamma || dbeta) {
        hipLaunchKernelGGL(grn_act_param_grad_kernel, dim3((unsigned)((pl.C4 + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, (const float*)tab_ns, (const float*)tab_d,
                           B, pl.C4, dgamma, dbeta);
        LAUNCH_CHECK_RET();
    }
    if (du) {
        if (drop)
            hipLaunchKernelGGL((grn_act_apply_kernel<true, true>), grid, dim3(kThreads), 0, st, u, dz, gamma, (const float*)nullptr, gx, (const float*)mtab,
                               (const float*)tab_k, g, p_drop, scale, key, seed_dev, du);
        else
            hipLaunchKernelGGL((grn_act_apply_kernel<true, false>), grid, dim3(kThreads), 0, st, u, dz, gamma, (const float*)nullptr, gx, (const float*)mtab,
                               (const float*)tab_k, g, 0.f, 1.f, 0ull, (const uint64_t*)nullptr, du);
        LAUNCH_CHECK_RET();
    }
    return PAELLA_OK;
}

}  // namespace

extern "C" size_t paella_grn_act_workspace_bytes(int B, int P, int C) {
    if (!shape_ok(B, P, C)) return 0;
    return make_plan(B, P, C).bytes;
}

extern "C" int paella_grn_act_forward(const float* u, const float* gamma, const float* beta, int B, int P, int C, float p_drop, uint64_t seed, float* z, float* gx, void* ws,
                                      size_t ws_bytes, void* stream) {
    return forward_impl("grn_act_forward", u, gamma, beta, B, P, C, p_drop, seed, nullptr, false, z, gx, ws, ws_bytes, stream);
}

extern "C" int paella_grn_act_forward_seed_dev(const float* u, const float* gamma, const float* beta, int B, int P, int C, float p_drop, const uint64_t* seed_dev, float* z,
                                               float* gx, void* ws, size_t ws_bytes, void* stream) {
    return forward_impl("grn_act_forward_seed_dev", u, gamma, beta, B, P, C, p_drop, 0ull, seed_dev, true, z, gx, ws, ws_bytes, stream);
}

extern "C" int paella_grn_act_backward(const float* u, const float* gamma, const float* gx, const float* dz, int B, int P, int C, float p_drop, uint64_t seed, float* du,
                                       float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream) {
    return backward_impl("grn_act_backward", u, gamma, gx, dz, B, P, C, p_drop, seed, nullptr, false, du, dgamma, dbeta, ws, ws_bytes, stream);
}

extern "C" int paella_grn_act_backward_seed_dev(const float* u, const float* gamma, const float* gx, const float* dz, int B, int P, int C, float p_drop,
                                                const uint64_t* seed_dev, float* du, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream) {
    return backward_impl("grn_act_backward_seed_dev", u, gamma, gx, dz, B, P, C, p_drop, 0ull, seed_dev, true, du, dgamma, dbeta, ws, ws_bytes, stream);
}
