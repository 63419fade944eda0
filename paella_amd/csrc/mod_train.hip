// Training timestep modulation: the joint between two blocks of a `C T [A]` unit in train mode -- the residual add that ends a ResBlock / FeedForwardBlock, the
// TimestepBlock's scale and shift, and the LayerNorm2d(C, no affine) that begins the next AttnBlock / FeedForwardBlock -- as ONE op, forward and backward.
// NHWC fp32, a sample is P = H W positions of C channels; ab [B, 2C] is the mapper's output as it is, a = ab[:, :C], b = ab[:, C:].
//
//   forward : u = x + residual,  x' = fma(u, 1 + a, b);  with the LayerNorm: mean / var of x' over C two-pass (as dwconv.hip),  rstd = 1 / sqrt(var + eps),
//             z = (x' - mean) rstd;  rstd [B P] is kept
//   backward: g = dx' + rstd (dz - mean_c dz - z mean_c(dz z)),  dx = dresidual = g (1 + a),  da[b][c] = sum_p g u,  db[b][c] = sum_p g;  u is recomputed from x
//             and residual, never recovered from x' (no division by 1 + a: a = -1 is an ordinary value)
//
// Launches.  Forward: one launch, one WAVE per position, a lane takes the 16-byte vectors lane, lane + 64, ...; x' is a pure function of (x, residual, ab) with one
// explicit fma, so the two statistics passes and the z pass recompute it from the inputs (cache hits) instead of holding a row of up to 8192 floats in registers;
// the sums by an xor butterfly.  Backward with dz: (1) g into the workspace and dx, one wave per position; (2) da / db: one thread per 16-byte vector of channels over
// a STRIP of positions of ONE sample, its sums carried in fp64, one fp32 partial per (sample, strip, channel); (3) the partials in ASCENDING strip order.  Backward
// without dz (the `C T` level, or a z nobody used): g is dx' itself, so (2) alone reads dx', x and residual once and writes dx next to its sums, then (3).  A sample
// of one strip writes (2) straight into dab and there is no (3).
// No float atomics, no tickets: every combine is a launch.  The strips depend on (P, C) only (make_plan), never on the device or on B; every value of a sample
// depends on that sample only, so its bits depend neither on its index nor on the batch around it.  The workspace needs no initialisation.
#include "train_common.h"

namespace {

using namespace train;

constexpr int kThreads = 256;     // four waves, one position each
constexpr int kSumThreads = 64;   // (2): 16-byte channel vectors per workgroup
constexpr int kMinRows = 16;      // (2): positions per strip at least -- the partials stay under an eighth of one activation tensor
constexpr int kMaxStrips = 1024;  // bounds the finalize loop of a long sample
constexpr int kMaxC = 8192, kMaxP = 1 << 20, kMaxB = 65535;

bool shape_ok(int B, int P, int C) {
    if (B < 1 || B > kMaxB || P < 1 || P > kMaxP || (int64_t)B * P > 0x7fffffffll) return false;
    return C >= 4 && !(C & 3) && C <= kMaxC;
}

struct Plan {
    int rows_per_strip, strips;
    int64_t N;
    size_t part_off, bytes;  // g at 0 (backward through the LayerNorm), then the partials (more than one strip)
};

Plan make_plan(int B, int P, int C, bool has_ln) {
    Plan p = {};
    p.N = (int64_t)B * P;
    const Strips s = plan_strips(P, kMinRows, kMaxStrips);
    p.rows_per_strip = s.rows;
    p.strips = s.count;
    p.part_off = has_ln ? align256((size_t)p.N * C * sizeof(float)) : 0;
    p.bytes = p.part_off + (p.strips > 1 ? align256((size_t)B * p.strips * 2 * C * sizeof(float)) : 0);
    return p;
}

__device__ __forceinline__ f32x4 ldq(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void stq(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// x' of one 16-byte vector: ONE rounding per element after the add, the same instruction wherever it is recomputed
template <bool RES>
__device__ __forceinline__ f32x4 modulated(const float* __restrict__ x, const float* __restrict__ res, const float* __restrict__ abp, int64_t off, int c, int C) {
    f32x4 u = ldq(x + off);
    if (RES) u = u + ldq(res + off);
    const f32x4 s = ldq(abp + c) + 1.0f, b = ldq(abp + C + c);
    return f32x4{fmaf(u[0], s[0], b[0]), fmaf(u[1], s[1], b[1]), fmaf(u[2], s[2], b[2]), fmaf(u[3], s[3], b[3])};
}

// Forward.  One wave per position; LN: the statistics two-pass over the recomputed x', then z and the position's rstd.
template <bool RES, bool LN>
__global__ __launch_bounds__(kThreads) void mod_ln_train_fwd_kernel(const float* __restrict__ x, const float* __restrict__ res, const float* __restrict__ ab,
                                                                    float* __restrict__ xp, float* __restrict__ z, float* __restrict__ rstd_out, int64_t N, int P, int C,
                                                                    float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t pos = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (pos >= N) return;  // (no workgroup barrier below)
    const int C4 = C >> 2;
    const float* abp = ab + (size_t)((unsigned)pos / (unsigned)P) * 2 * C;
    const int64_t row = pos * C;
    float s = 0.f;
    for (int c4 = lane; c4 < C4; c4 += 64) {
        const f32x4 v = modulated<RES>(x, res, abp, row + c4 * 4, c4 * 4, C);
        stq(xp + row + c4 * 4, v);
        s += (v[0] + v[1]) + (v[2] + v[3]);
    }
    if (!LN) return;
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
    for (int c4 = lane; c4 < C4; c4 += 64) {
        f32x4 d = modulated<RES>(x, res, abp, row + c4 * 4, c4 * 4, C) - mean;
        d = d * d;
        q += (d[0] + d[1]) + (d[2] + d[3]);
    }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)C + eps);
    if (lane == 0) rstd_out[pos] = rstd;
    for (int c4 = lane; c4 < C4; c4 += 64) stq(z + row + c4 * 4, (modulated<RES>(x, res, abp, row + c4 * 4, c4 * 4, C) - mean) * rstd);
}

// Backward (1): g = dx' + rstd (dz - c1 - z c2) with c1 = mean_c dz, c2 = mean_c(dz z); g (for the sums of (2)) and dx = g (1 + a) are stored where wanted.
// One wave per position, as dwconv_train.hip's da kernel.
__global__ __launch_bounds__(kThreads) void mod_ln_train_g_kernel(const float* __restrict__ dxp, const float* __restrict__ dz, const float* __restrict__ z,
                                                                  const float* __restrict__ rstd, const float* __restrict__ ab, float* __restrict__ g,
                                                                  float* __restrict__ dx, int64_t N, int P, int C) {
    const int lane = threadIdx.x & 63;
    const int64_t pos = (int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (pos >= N) return;
    const int C4 = C >> 2;
    const float* abp = ab + (size_t)((unsigned)pos / (unsigned)P) * 2 * C;
    const int64_t row = pos * C;
    float s1 = 0.f, s2 = 0.f;
    for (int c4 = lane; c4 < C4; c4 += 64) {
        const f32x4 d = ldq(dz + row + c4 * 4), v = ldq(z + row + c4 * 4);
        s1 += (d[0] + d[1]) + (d[2] + d[3]);
        s2 += (d[0] * v[0] + d[1] * v[1]) + (d[2] * v[2] + d[3] * v[3]);
    }
    const float c1 = wave_sum(s1) / (float)C, c2 = wave_sum(s2) / (float)C, r = rstd[pos];
    for (int c4 = lane; c4 < C4; c4 += 64) {
        const f32x4 d = ldq(dz + row + c4 * 4), v = ldq(z + row + c4 * 4);
        f32x4 gv = ((d - c1) - v * c2) * r;
        if (dxp) gv = gv + ldq(dxp + row + c4 * 4);
        if (g) stq(g + row + c4 * 4, gv);
        if (dx) stq(dx + row + c4 * 4, gv * (ldq(abp + c4 * 4) + 1.0f));
    }
}

// Backward (2): over the positions [p0, p1) of strip blockIdx.y of sample blockIdx.z, thread c4: da += g u and db += g in fp64, positions ascending, u = x + residual
// recomputed in fp32 as the forward formed it.  `part` [sample][strip][2C] takes the sums (da in [0, C), db in [C, 2C)) -- dab itself when a sample is one strip;
// NULL: no sums.  dx (the path without dz, where g is dx'): g (1 + a) is written on the way; NULL: not written.
template <bool RES>
__global__ __launch_bounds__(kSumThreads) void mod_ln_train_sum_kernel(const float* __restrict__ g, const float* __restrict__ x, const float* __restrict__ res,
                                                                       const float* __restrict__ ab, float* __restrict__ dx, float* __restrict__ part, int P, int C,
                                                                       int rows_per_strip) {
    const int c4 = blockIdx.x * kSumThreads + threadIdx.x;
    if (c4 >= (C >> 2)) return;
    const int b = blockIdx.z;
    const int p0 = blockIdx.y * rows_per_strip;
    const int p1 = min(P, p0 + rows_per_strip);
    const f32x4 s = ldq(ab + (size_t)b * 2 * C + c4 * 4) + 1.0f;
    int64_t off = ((int64_t)b * P + p0) * C + c4 * 4;
    double da0 = 0.0, da1 = 0.0, da2 = 0.0, da3 = 0.0, db0 = 0.0, db1 = 0.0, db2 = 0.0, db3 = 0.0;
#pragma unroll 4
    for (int p = p0; p < p1; ++p, off += C) {
        const f32x4 gv = ldq(g + off);
        if (dx) stq(dx + off, gv * s);
        if (part) {
            f32x4 u = ldq(x + off);
            if (RES) u = u + ldq(res + off);
            da0 = fma((double)gv[0], (double)u[0], da0);
            da1 = fma((double)gv[1], (double)u[1], da1);
            da2 = fma((double)gv[2], (double)u[2], da2);
            da3 = fma((double)gv[3], (double)u[3], da3);
            db0 += (double)gv[0];
            db1 += (double)gv[1];
            db2 += (double)gv[2];
            db3 += (double)gv[3];
        }
    }
    if (part) {
        float* o = part + ((size_t)b * gridDim.y + blockIdx.y) * 2 * C + c4 * 4;
        stq(o, f32x4{(float)da0, (float)da1, (float)da2, (float)da3});
        stq(o + C, f32x4{(float)db0, (float)db1, (float)db2, (float)db3});
    }
}

// Backward (3): dab [B, 2C] = the partials of its sample in ascending strip order, in fp64; one thread per element
__global__ __launch_bounds__(kThreads) void mod_ln_train_finalize_kernel(const float* __restrict__ part, int strips, int C2, int64_t total, float* __restrict__ dab) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= total) return;
    const int64_t b = i / C2;
    const float* p = part + (size_t)b * strips * C2 + (i - b * C2);
    double s = 0.0;
#pragma unroll 8  // the loads of eight strips in flight; the additions keep their order
    for (int st = 0; st < strips; ++st) s += (double)p[(size_t)st * C2];
    dab[i] = (float)s;
}

int check_shape(const char* who, int B, int P, int C) {
    if (shape_ok(B, P, C)) return PAELLA_OK;
    paella_set_error("%s: unsupported shape B=%d P=%d C=%d (B in 1...65535, P in 1...2^20 with B P <= 2^31 - 1; C a multiple of 4 in 4...8192)", who, B, P, C);
    return PAELLA_ERR_ARG;
}

}  // namespace

extern "C" size_t paella_mod_ln_train_workspace_bytes(int B, int P, int C, int has_layernorm) {
    if (!shape_ok(B, P, C)) return 0;
    const size_t need = make_plan(B, P, C, has_layernorm != 0).bytes;
    return need ? need : 256;  // 0 says "unsupported"
}

extern "C" int paella_mod_ln_train_forward(const float* x, const float* residual, const float* ab, int B, int P, int C, float eps, float* xp, float* z, float* rstd,
                                           void* ws, size_t ws_bytes, void* stream) {
    const char* who = "mod_ln_train_forward";
    (void)ws;
    (void)ws_bytes;  // the forward uses no workspace
    int rc = check_shape(who, B, P, C);
    if (rc != PAELLA_OK) return rc;
    if (!(eps > 0.f) || !(eps < 1e30f)) {  // false for NaN as well
        paella_set_error("%s: eps must be positive and finite (got %g)", who, (double)eps);
        return PAELLA_ERR_ARG;
    }
    rc = check_required(who, x && ab && xp, "x, ab and xp");
    if (rc != PAELLA_OK) return rc;
    if ((z == nullptr) != (rstd == nullptr)) {
        paella_set_error("%s: z and rstd go together (both, or both NULL)", who);
        return PAELLA_ERR_ARG;
    }
    rc = check_tensors_aligned16(who, x, residual, ab, xp, z, rstd);
    if (rc != PAELLA_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int64_t N = (int64_t)B * P;
    const dim3 grid((unsigned)((N + 3) / 4)), block(kThreads);
#define MOD_FWD(RESv, LNv) hipLaunchKernelGGL((mod_ln_train_fwd_kernel<RESv, LNv>), grid, block, 0, st, x, residual, ab, xp, z, rstd, N, P, C, eps)
    if (residual && z) MOD_FWD(true, true);
    else if (residual) MOD_FWD(true, false);
    else if (z) MOD_FWD(false, true);
    else MOD_FWD(false, false);
#undef MOD_FWD
    LAUNCH_CHECK_RET();
    return PAELLA_OK;
}

extern "C" int paella_mod_ln_train_backward(const float* x, const float* residual, const float* ab, const float* z, const float* rstd, const float* dxp, const float* dz,
                                            int B, int P, int C, float* dx, float* dab, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "mod_ln_train_backward";
    int rc = check_shape(who, B, P, C);
    if (rc == PAELLA_OK) rc = check_required(who, x && ab, "x and ab");
    if (rc != PAELLA_OK) return rc;
    if (!dxp && !dz) {
        paella_set_error("%s: at least one of dxp and dz is required", who);
        return PAELLA_ERR_ARG;
    }
    if (dz && !(z && rstd)) {
        paella_set_error("%s: dz needs z and rstd", who);
        return PAELLA_ERR_ARG;
    }
    rc = check_tensors_aligned16(who, x, residual, ab, z, rstd, dxp, dz, dx, dab);
    if (rc != PAELLA_OK) return rc;
    const Plan pl = make_plan(B, P, C, dz != nullptr);
    if (pl.bytes) {
        rc = check_workspace(who, ws, ws_bytes, pl.bytes, "paella_mod_ln_train_workspace_bytes asks for");
        if (rc != PAELLA_OK) return rc;
    }
    if (!dx && !dab) return PAELLA_OK;
    hipStream_t st = (hipStream_t)stream;
    const float* g = dxp;
    float* dx_of_sums = dx;  // without dz the summing pass is the only pass and writes dx as well
    if (dz) {
        float* gw = dab ? (float*)ws : nullptr;
        hipLaunchKernelGGL(mod_ln_train_g_kernel, dim3((unsigned)((pl.N + 3) / 4)), dim3(kThreads), 0, st, dxp, dz, z, rstd, ab, gw, dx, pl.N, P, C);
        LAUNCH_CHECK_RET();
        if (!dab) return PAELLA_OK;
        g = gw;
        dx_of_sums = nullptr;
    }
    const bool one = pl.strips == 1;
    float* part = !dab ? nullptr : one ? dab : (float*)((char*)ws + pl.part_off);
    const dim3 grid((unsigned)((C / 4 + kSumThreads - 1) / kSumThreads), (unsigned)pl.strips, (unsigned)B);
    if (residual) hipLaunchKernelGGL((mod_ln_train_sum_kernel<true>), grid, dim3(kSumThreads), 0, st, g, x, residual, ab, dx_of_sums, part, P, C, pl.rows_per_strip);
    else hipLaunchKernelGGL((mod_ln_train_sum_kernel<false>), grid, dim3(kSumThreads), 0, st, g, x, residual, ab, dx_of_sums, part, P, C, pl.rows_per_strip);
    LAUNCH_CHECK_RET();
    if (dab && !one) {
        const int64_t total = (int64_t)B * 2 * C;
        hipLaunchKernelGGL(mod_ln_train_finalize_kernel, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, (const float*)part, pl.strips, 2 * C,
                           total, dab);
        LAUNCH_CHECK_RET();
    }
    return PAELLA_OK;
}
