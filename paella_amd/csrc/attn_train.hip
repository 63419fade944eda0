// Training attention: softmax(Q K^T / sqrt(D)) V with dropout on the probabilities, forward and backward, flash style -- the attention core of every `A` block in
// train mode (`training._attn_block`), between the in-projection and the out-projection.  Everything fp32; both directions run on the exact-fp32 matrix cores
// (v_mfma_f32_16x16x4_f32), in the per-tile arithmetic of attention.hip (copied, not shared: that unit's code must not move).
//
//   forward : s = q k^T / sqrt(D),  lse = logsumexp_j s (online, the running row maximum subtracted),  pr = exp(s - lse),  o = (keep pr / (1 - p)) v
//   backward: delta_i = sum_c do_ic o_ic,  dpd = do v^T,  dp = keep dpd / (1 - p),  ds = pr (dp - delta),
//             dq = ds k / sqrt(D),  dk = ds^T q / sqrt(D),  dv = (keep pr / (1 - p))^T do
//
// The forward leaves o and lse [B, nhead, P] and nothing else; no [P, L] array ever exists in global memory.  The backward recomputes pr from q, k and lse and the
// dropout mask from its counter: element e (flat index in [B, nhead, P, L4], L4 = 4 ceil(L / 4), so a quad never straddles a row) takes word e & 3 of
// philox4x32(seed ^ kAttnDropoutSalt, e >> 2, 0) and is kept iff u01_half_open(word) >= p -- the rule of grn_act.hip under another salt.
//
// Every workgroup is ONE wave that owns a 16-wide tile of one (sample, head) and walks the other axis in ascending 16-wide tiles:
//   forward  owns 16 queries, walks the keys:   S^T[key][q] = K Q^T, the probabilities a lane holds are its B operand of O^T[d][q] += V^T P^T (as attention.hip)
//   dq       owns 16 queries, walks the keys:   S^T and dPd^T[key][q] = V dO^T in the same form, then dQ^T[d][q] += K^T dS^T
//   dk / dv  owns 16 keys, walks the queries:   S[q][key] = Q K^T and dPd[q][key] = dO V^T, then dV^T[d][key] += dO^T Pd and dK^T[d][key] += Q^T dS
// so the statistics of a query (forward, dq) or the owned key (dk / dv) sit on the lane, no product needs a transpose through LDS, and no sum crosses a
// workgroup: no float atomics, no tickets.  delta comes from a pre-pass into the workspace (one thread per (sample, query, head)).  Tails in P and L are bounds:
// loads come from clamped in-range rows, scores of keys past L and probabilities of queries past P are masked, stores are guarded.  The order of every sum is
// fixed by (B, nhead, P, L, D) alone, and everything a (sample, head) computes depends on that sample's data only.
#include "common.h"
#include "philox.h"
#include "train_common.h"
#include <math.h>

namespace {

using namespace train;

constexpr int kMaxB = 65535, kMaxHeads = 65535, kMaxP = 1 << 20, kMaxL = 1 << 20;
constexpr int64_t kMaxRows = 2147483647;  // B * nhead * P: lse / delta entries, and the pre-pass's threads
// key salt of the attention dropout stream, next to grn_act.hip's 0xa0761d6478bd642f
constexpr uint64_t kAttnDropoutSalt = 0xe7037ed1a0b428dbull;

// exp on the hardware exp2, as attention.hip: exp_fast(-inf) = 0
__device__ __forceinline__ float exp_fast(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896340736f); }

// exp(fp32(s * scale) - lse) for the backward's recomputed probabilities, the argument carried in two floats.  The rounded product is the score the forward's lse
// was summed over (the same bits: both directions run the same fma chain), so it is taken as it is; but it and lse are both of the size of the scores while their
// difference decides the probability: with the difference and the change to base 2 rounded on the way (each up to half an ulp of a number around |lse|), the
// largest probabilities of a row would be off by several 1e-7 relatively -- more than every other error of a short row.  The difference's error comes from TwoSum,
// the base change's from one fma; what is left is the hardware exp2's own ulp.  A query with one key gets exactly 1.
__device__ __forceinline__ float exp_diff(float s, float scale, float lse) {
    const float p = s * scale;
    const float d = p - lse;
    const float bb = d - p;
    const float de = (p - (d - bb)) + (-lse - bb);
    const float t = d * 1.44269504088896340736f;
    const float te = __builtin_fmaf(d, 1.44269504088896340736f, -t) + __builtin_fmaf(de, 1.44269504088896340736f, d * 1.92596299e-8f);  // log2 e = hi + lo
    const float r = __builtin_amdgcn_exp2f(t);
    return __builtin_fmaf(r, te * 0.69314718055994530942f, r);
}

// The gradient accumulators are flushed into a second set every kFlushTiles tiles of the walked axis: a sum over thousands of keys (queries) is then chains of at most
// 16 kFlushTiles fp32 fmas plus one addition per block instead of ONE chain whose every step rounds at the size of the whole sum.  Fixed by the shape: block b is
// tiles [b kFlushTiles, (b + 1) kFlushTiles), blocks are added in ascending order.
constexpr int kFlushTiles = 8;

struct Geo {
    int nhead, P, L;
    int ldq, ldk, ldv, ldg;  // ldg: the row pitch of the gradient(s) the kernel writes (dq; or dk)
    int ldg2;                // ... and of dv
    float scale;             // 1 / sqrt(D)
    float p_drop, keep_scale;
    uint64_t key;
    const uint64_t* seed_dev;  // the *_seed_dev forms: the seed is this device word and key the salt alone (NULL: key = seed ^ salt, by value)
    uint64_t quads;          // L4 / 4: Philox calls per (sample, head, query) row
};

// the multipliers of the 4 elements of one quad: 1 / (1 - p) where kept, 0 where dropped
__device__ __forceinline__ void quad_keep(const Geo& g, uint64_t key, uint64_t quad, float (&m)[4]) {
    uint32_t w[4];
    philox4x32(key, quad, 0ull, w);
#pragma unroll
    for (int e = 0; e < 4; ++e) m[e] = u01_half_open(w[e]) >= g.p_drop ? g.keep_scale : 0.f;
}

// the Philox key of a drawing kernel: uniform, so the word comes by one scalar load
__device__ __forceinline__ uint64_t dropout_key(const Geo& g) { return g.seed_dev ? g.key ^ *g.seed_dev : g.key; }

// Forward.  grid (query tiles, nhead, B), one wave.  Lane (r16, kq) holds S^T[key = 16 kt + 4 kq + r][q = q0 + r16]: the four keys of ONE dropout quad.
template <int DT, bool DROP>
__global__ __launch_bounds__(64) void attn_train_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, Geo g,
                                                            float* __restrict__ o, float* __restrict__ lse) {
    constexpr int D = DT * 16;
    const int lane = threadIdx.x;
    const int r16 = lane & 15, kq = lane >> 4;
    const int q0 = blockIdx.x * 16, h = blockIdx.y, b = blockIdx.z;
    const int P = g.P, L = g.L;
    uint64_t key = 0ull;
    if constexpr (DROP) key = dropout_key(g);
    const int qi = min(q0 + r16, P - 1);  // rows past P are clamped; their outputs are not stored
    const size_t row = ((size_t)b * g.nhead + h) * P + qi;
    f32x4 qf[DT];
    {
        const float* qp = q + ((size_t)b * P + qi) * g.ldq + h * D + kq * 4;
#pragma unroll
        for (int j = 0; j < DT; ++j) qf[j] = *reinterpret_cast<const f32x4*>(qp + j * 16);
    }
    const float* kb = k + (size_t)b * L * g.ldk + h * D;
    const float* vb = v + (size_t)b * L * g.ldv + h * D;
    f32x4 oacc[DT];
#pragma unroll
    for (int j = 0; j < DT; ++j) oacc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;
    const int ntiles = (L + 15) / 16;
    for (int kt = 0; kt < ntiles; ++kt) {
        f32x4 kf[DT];
        float vf[DT][4];
        {
            const float* kp = kb + (size_t)min(kt * 16 + r16, L - 1) * g.ldk + kq * 4;
#pragma unroll
            for (int j = 0; j < DT; ++j) kf[j] = *reinterpret_cast<const f32x4*>(kp + j * 16);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float* vp = vb + (size_t)min(kt * 16 + kq * 4 + e, L - 1) * g.ldv + r16;
#pragma unroll
                for (int j = 0; j < DT; ++j) vf[j][e] = vp[j * 16];
            }
        }
        f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < DT; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) s = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[j][e], qf[j][e], s, 0, 0, 0);
        float p[4];
        float mt = -INFINITY;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            p[r] = kt * 16 + kq * 4 + r < L ? s[r] * g.scale : -INFINITY;
            mt = fmaxf(mt, p[r]);
        }
        mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
        const float m_new = fmaxf(m_run, mt);  // finite: every tile has a key inside L
        const float alpha = exp_fast(m_run - m_new);  // first tile: exp(-inf) = 0
        float psum = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            p[r] = exp_fast(p[r] - m_new);  // masked keys: exp(-inf) = 0, which also zeroes their (clamped) V rows
            psum += p[r];
        }
        l_run = l_run * alpha + psum;  // per-lane partial of the UNdropped sum; lanes of equal r16 are combined at the end
        m_run = m_new;
        if constexpr (DROP) {
            float m[4];
            quad_keep(g, key, (uint64_t)row * g.quads + (uint64_t)(kt * 4 + kq), m);
#pragma unroll
            for (int r = 0; r < 4; ++r) p[r] = m[r] > 0.f ? p[r] * m[r] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < DT; ++j) {
            oacc[j] *= alpha;
#pragma unroll
            for (int e = 0; e < 4; ++e) oacc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[j][e], p[e], oacc[j], 0, 0, 0);
        }
    }
    float l = l_run;
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    if (q0 + r16 < P) {
        const float inv = 1.0f / l;
        float* op = o + ((size_t)b * P + qi) * ((size_t)g.nhead * D) + h * D + kq * 4;
#pragma unroll
        for (int j = 0; j < DT; ++j) *reinterpret_cast<f32x4*>(op + j * 16) = oacc[j] * inv;
        if (kq == 0) lse[row] = m_run + logf(l);
    }
}

// delta [B, nhead, P] = sum_c do o over the head's D channels.  One thread per (b, q, h), h fastest: neighbours read neighbouring memory.
__global__ __launch_bounds__(256) void attn_train_delta_kernel(const float* __restrict__ o, const float* __restrict__ dout, int nhead, int P, int D, int64_t total,
                                                               float* __restrict__ delta) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int h = (int)(i % nhead);
    const int64_t bq = i / nhead;
    const int64_t b = bq / P, qi = bq - b * P;
    const f32x4* op = reinterpret_cast<const f32x4*>(o + (size_t)i * D);
    const f32x4* gp = reinterpret_cast<const f32x4*>(dout + (size_t)i * D);
    // one fma chain in the channel order of the matrix core's dpd = do v^T (per 16 channels: 0, 4, 8, 12, 1, 5, ...), and the backward kernels put the dropout
    // scale on v (dp = keep (do (v / (1 - p))^T), one rounding per element of v, as the forward's o has): where the softmax of a query is one-hot -- a single key,
    // or saturated scores -- o is that key's fp32(v / (1 - p)), delta is dp bit for bit, and ds, dq and dk's share are exactly the zeros they are, not rounding noise
    float s = 0.f;
    for (int j = 0; j < D / 16; ++j) {
        f32x4 a[4], d[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            a[c] = op[4 * j + c];
            d[c] = gp[4 * j + c];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int c = 0; c < 4; ++c) s = fmaf(d[c][e], a[c][e], s);
    }
    delta[((size_t)b * nhead + h) * P + qi] = s;
}

// dq.  grid (query tiles, nhead, B), one wave; lane layout as the forward.
template <int DT, bool DROP>
__global__ __launch_bounds__(64) void attn_train_dq_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                           const float* __restrict__ lse, const float* __restrict__ dout, const float* __restrict__ delta, Geo g,
                                                           float* __restrict__ dq) {
    constexpr int D = DT * 16;
    const int lane = threadIdx.x;
    const int r16 = lane & 15, kq = lane >> 4;
    const int q0 = blockIdx.x * 16, h = blockIdx.y, b = blockIdx.z;
    const int P = g.P, L = g.L;
    uint64_t key = 0ull;
    if constexpr (DROP) key = dropout_key(g);
    const int qi = min(q0 + r16, P - 1);
    const size_t row = ((size_t)b * g.nhead + h) * P + qi;
    f32x4 qf[DT], gf[DT];
    {
        const float* qp = q + ((size_t)b * P + qi) * g.ldq + h * D + kq * 4;
        const float* gp = dout + ((size_t)b * P + qi) * ((size_t)g.nhead * D) + h * D + kq * 4;
#pragma unroll
        for (int j = 0; j < DT; ++j) {
            qf[j] = *reinterpret_cast<const f32x4*>(qp + j * 16);
            gf[j] = *reinterpret_cast<const f32x4*>(gp + j * 16);
        }
    }
    const float lse_q = lse[row], delta_q = delta[row];
    const float* kb = k + (size_t)b * L * g.ldk + h * D;
    const float* vb = v + (size_t)b * L * g.ldv + h * D;
    f32x4 acc[DT], tot[DT];
#pragma unroll
    for (int j = 0; j < DT; ++j) acc[j] = tot[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int ntiles = (L + 15) / 16;
    for (int kt = 0; kt < ntiles; ++kt) {
        if (kt && kt % kFlushTiles == 0) {
#pragma unroll
            for (int j = 0; j < DT; ++j) {
                tot[j] += acc[j];
                acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
        f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f}, dp = f32x4{0.f, 0.f, 0.f, 0.f};
        {
            const size_t kr = (size_t)min(kt * 16 + r16, L - 1);
            const float* kp = kb + kr * g.ldk + kq * 4;
            const float* vp = vb + kr * g.ldv + kq * 4;
#pragma unroll
            for (int j = 0; j < DT; ++j) {
                const f32x4 kf = *reinterpret_cast<const f32x4*>(kp + j * 16);
                f32x4 vf = *reinterpret_cast<const f32x4*>(vp + j * 16);
                if constexpr (DROP) vf *= g.keep_scale;  // dp = keep (do (v / (1 - p))^T): see delta
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    s = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[e], qf[j][e], s, 0, 0, 0);
                    dp = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[e], gf[j][e], dp, 0, 0, 0);
                }
            }
        }
        float m[4] = {1.f, 1.f, 1.f, 1.f};
        if constexpr (DROP) quad_keep(g, key, (uint64_t)row * g.quads + (uint64_t)(kt * 4 + kq), m);
        float ds[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float pr = kt * 16 + kq * 4 + r < L ? exp_diff(s[r], g.scale, lse_q) : 0.f;
            ds[r] = pr * ((m[r] > 0.f ? dp[r] : 0.f) - delta_q);
        }
        // K^T operand: K[16 kt + 4 kq + e][16 j + r16]
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float* kp = kb + (size_t)min(kt * 16 + kq * 4 + e, L - 1) * g.ldk + r16;
#pragma unroll
            for (int j = 0; j < DT; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(kp[j * 16], ds[e], acc[j], 0, 0, 0);
        }
    }
    if (q0 + r16 < P) {
        float* op = dq + ((size_t)b * P + qi) * g.ldg + h * D + kq * 4;
#pragma unroll
        for (int j = 0; j < DT; ++j) *reinterpret_cast<f32x4*>(op + j * 16) = (tot[j] + acc[j]) * g.scale;
    }
}

// dk / dv.  grid (key tiles, nhead, B), one wave that owns 16 keys and walks the query tiles in ascending order.  Lane (r16, kq) holds
// S[q = 16 qt + 4 kq + r][key = k0 + r16].  The mask of that element is word r16 & 3 of the quad (q, key >> 2): lane (r16, kq) draws the quad of
// (q = 16 qt + 4 kq + (r16 & 3), keys 4 (r16 >> 2) ...) ONCE, as four keep bits, and the lanes fetch the bit they need by shuffle -- one Philox call per lane and tile.
template <int DT, bool DROP>
__global__ __launch_bounds__(64) void attn_train_dkv_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                            const float* __restrict__ lse, const float* __restrict__ dout, const float* __restrict__ delta, Geo g,
                                                            float* __restrict__ dk, float* __restrict__ dv) {
    constexpr int D = DT * 16;
    const int lane = threadIdx.x;
    const int r16 = lane & 15, kq = lane >> 4;
    const int k0 = blockIdx.x * 16, h = blockIdx.y, b = blockIdx.z;
    const int P = g.P, L = g.L;
    uint64_t key = 0ull;
    if constexpr (DROP) key = dropout_key(g);
    const int ki = min(k0 + r16, L - 1);  // keys past L are clamped; their probabilities are masked and their rows not stored
    const bool key_ok = k0 + r16 < L;
    const size_t row0 = ((size_t)b * g.nhead + h) * P;
    const size_t ldo = (size_t)g.nhead * D;
    f32x4 kf[DT], vf[DT];
    {
        const float* kp = k + ((size_t)b * L + ki) * g.ldk + h * D + kq * 4;
        const float* vp = v + ((size_t)b * L + ki) * g.ldv + h * D + kq * 4;
#pragma unroll
        for (int j = 0; j < DT; ++j) {
            kf[j] = *reinterpret_cast<const f32x4*>(kp + j * 16);
            vf[j] = *reinterpret_cast<const f32x4*>(vp + j * 16);
            if constexpr (DROP) vf[j] *= g.keep_scale;  // dp = keep (do (v / (1 - p))^T): see delta
        }
    }
    const float* qb = q + (size_t)b * P * g.ldq + h * D;
    const float* gb = dout + (size_t)b * P * ldo + h * D;
    f32x4 acck[DT], accv[DT], totk[DT], totv[DT];
#pragma unroll
    for (int j = 0; j < DT; ++j) acck[j] = accv[j] = totk[j] = totv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int ntiles = (P + 15) / 16;
    for (int qt = 0; qt < ntiles; ++qt) {
        if (qt && qt % kFlushTiles == 0) {
#pragma unroll
            for (int j = 0; j < DT; ++j) {
                totk[j] += acck[j];
                totv[j] += accv[j];
                acck[j] = accv[j] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
        f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f}, dp = f32x4{0.f, 0.f, 0.f, 0.f};
        {
            const size_t qr = (size_t)min(qt * 16 + r16, P - 1);
            const float* qp = qb + qr * g.ldq + kq * 4;
            const float* gp = gb + qr * ldo + kq * 4;
#pragma unroll
            for (int j = 0; j < DT; ++j) {
                const f32x4 qf = *reinterpret_cast<const f32x4*>(qp + j * 16);
                const f32x4 gf = *reinterpret_cast<const f32x4*>(gp + j * 16);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    s = __builtin_amdgcn_mfma_f32_16x16x4f32(qf[e], kf[j][e], s, 0, 0, 0);
                    dp = __builtin_amdgcn_mfma_f32_16x16x4f32(gf[e], vf[j][e], dp, 0, 0, 0);
                }
            }
        }
        int bits = 15;
        if constexpr (DROP) {
            const int qd = min(qt * 16 + kq * 4 + (r16 & 3), P - 1);
            uint32_t w[4];
            philox4x32(key, (uint64_t)(row0 + qd) * g.quads + (uint64_t)((k0 >> 2) + (r16 >> 2)), 0ull, w);
            bits = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) bits |= (u01_half_open(w[e]) >= g.p_drop ? 1 : 0) << e;
        }
        float pd[4], ds[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int qi = qt * 16 + kq * 4 + r;
            const int qc = min(qi, P - 1);
            const float lse_q = lse[row0 + qc], delta_q = delta[row0 + qc];
            const float pr = key_ok && qi < P ? exp_diff(s[r], g.scale, lse_q) : 0.f;
            bool keep = true;
            if constexpr (DROP) keep = (__shfl(bits, (lane & ~3) | r, 64) >> (r16 & 3)) & 1;  // every lane takes part: never under a divergent test
            pd[r] = keep ? pr * g.keep_scale : 0.f;
            ds[r] = pr * ((keep ? dp[r] : 0.f) - delta_q);
        }
        // dO^T and Q^T operands: row 16 qt + 4 kq + e, column 16 j + r16
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const size_t qr = (size_t)min(qt * 16 + kq * 4 + e, P - 1);
            const float* gp = gb + qr * ldo + r16;
            const float* qp = qb + qr * g.ldq + r16;
            if (dv) {
#pragma unroll
                for (int j = 0; j < DT; ++j) accv[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(gp[j * 16], pd[e], accv[j], 0, 0, 0);
            }
            if (dk) {
#pragma unroll
                for (int j = 0; j < DT; ++j) acck[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(qp[j * 16], ds[e], acck[j], 0, 0, 0);
            }
        }
    }
    if (key_ok) {
        if (dk) {
            float* op = dk + ((size_t)b * L + ki) * g.ldg + h * D + kq * 4;
#pragma unroll
            for (int j = 0; j < DT; ++j) *reinterpret_cast<f32x4*>(op + j * 16) = (totk[j] + acck[j]) * g.scale;
        }
        if (dv) {
            float* op = dv + ((size_t)b * L + ki) * g.ldg2 + h * D + kq * 4;
#pragma unroll
            for (int j = 0; j < DT; ++j) *reinterpret_cast<f32x4*>(op + j * 16) = totv[j] + accv[j];
        }
    }
}

bool shape_ok(int B, int nhead, int P, int L, int D) {
    return B >= 1 && B <= kMaxB && nhead >= 1 && nhead <= kMaxHeads && P >= 1 && P <= kMaxP && L >= 1 && L <= kMaxL && D >= 16 && D <= 128 && (D & 15) == 0 &&
           (int64_t)B * nhead * P <= kMaxRows && (int64_t)nhead * D <= (1 << 24);
}

// the workspace: delta [B, nhead, P]
size_t plan_bytes(int B, int nhead, int P) { return align256((size_t)B * nhead * P * sizeof(float)); }

int check_shape(const char* who, int B, int nhead, int P, int L, int D) {
    if (shape_ok(B, nhead, P, L, D)) return PAELLA_OK;
    paella_set_error("%s: unsupported shape B=%d nhead=%d P=%d L=%d D=%d (D a multiple of 16 in 16...128, B and nhead in 1...65535, P and L in 1...2^20, "
                     "B nhead P <= 2^31 - 1, nhead D <= 2^24)", who, B, nhead, P, L, D);
    return PAELLA_ERR_ARG;
}

// a row pitch: a multiple of 4 floats that holds the nhead * D floats of a row
int check_ld(const char* who, const char* name, int ld, int C) {
    if (ld >= C && (ld & 3) == 0) return PAELLA_OK;
    paella_set_error("%s: %s = %d must be a multiple of 4 and at least nhead * D = %d", who, name, ld, C);
    return PAELLA_ERR_ARG;
}

int check_p(const char* who, float p_drop) {
    if (p_drop >= 0.f && p_drop < 1.f) return PAELLA_OK;  // false for NaN as well
    paella_set_error("%s: p_drop must lie in [0, 1) (got %g)", who, (double)p_drop);
    return PAELLA_ERR_ARG;
}

Geo make_geo(int nhead, int P, int L, int D, int ldq, int ldk, int ldv, float p_drop, uint64_t seed, const uint64_t* seed_dev) {
    Geo g = {};
    g.nhead = nhead; g.P = P; g.L = L;
    g.ldq = ldq; g.ldk = ldk; g.ldv = ldv;
    g.scale = 1.0f / sqrtf((float)D);
    g.p_drop = p_drop;
    g.keep_scale = 1.0f / (1.0f - p_drop);
    g.key = p_drop > 0.f ? seed ^ kAttnDropoutSalt : 0ull;  // by pointer: seed = 0, the kernels add the word
    g.seed_dev = p_drop > 0.f ? seed_dev : nullptr;
    g.quads = (uint64_t)((L + 3) / 4);
    return g;
}

template <int DT>
void launch_fwd(bool drop, dim3 grid, hipStream_t st, const float* q, const float* k, const float* v, const Geo& g, float* o, float* lse) {
    if (drop) hipLaunchKernelGGL((attn_train_fwd_kernel<DT, true>), grid, dim3(64), 0, st, q, k, v, g, o, lse);
    else hipLaunchKernelGGL((attn_train_fwd_kernel<DT, false>), grid, dim3(64), 0, st, q, k, v, g, o, lse);
}
template <int DT>
void launch_dq(bool drop, dim3 grid, hipStream_t st, const float* q, const float* k, const float* v, const float* lse, const float* dout, const float* delta, const Geo& g,
               float* dq) {
    if (drop) hipLaunchKernelGGL((attn_train_dq_kernel<DT, true>), grid, dim3(64), 0, st, q, k, v, lse, dout, delta, g, dq);
    else hipLaunchKernelGGL((attn_train_dq_kernel<DT, false>), grid, dim3(64), 0, st, q, k, v, lse, dout, delta, g, dq);
}
template <int DT>
void launch_dkv(bool drop, dim3 grid, hipStream_t st, const float* q, const float* k, const float* v, const float* lse, const float* dout, const float* delta, const Geo& g,
                float* dk, float* dv) {
    if (drop) hipLaunchKernelGGL((attn_train_dkv_kernel<DT, true>), grid, dim3(64), 0, st, q, k, v, lse, dout, delta, g, dk, dv);
    else hipLaunchKernelGGL((attn_train_dkv_kernel<DT, false>), grid, dim3(64), 0, st, q, k, v, lse, dout, delta, g, dk, dv);
}

// the head widths: D = 16 DT
#define ATTN_TRAIN_DISPATCH(DT_VALUE, CALL)    \
    switch (DT_VALUE) {                        \
        case 1: { constexpr int DT = 1; CALL; } break; \
        case 2: { constexpr int DT = 2; CALL; } break; \
        case 3: { constexpr int DT = 3; CALL; } break; \
        case 4: { constexpr int DT = 4; CALL; } break; \
        case 5: { constexpr int DT = 5; CALL; } break; \
        case 6: { constexpr int DT = 6; CALL; } break; \
        case 7: { constexpr int DT = 7; CALL; } break; \
        default: { constexpr int DT = 8; CALL; } break; \
    }

}  // namespace

extern "C" size_t paella_attn_train_workspace_bytes(int B, int nhead, int P, int L, int D) {
    if (!shape_ok(B, nhead, P, L, D)) return 0;
    return plan_bytes(B, nhead, P);
}

namespace {

int forward_impl(const char* who, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, int B, int nhead, int P, int L, int D, float p_drop,
                 uint64_t seed, const uint64_t* seed_dev, bool by_pointer, float* o, float* lse, void* ws, size_t ws_bytes, void* stream) {
    int rc = check_shape(who, B, nhead, P, L, D);
    if (rc == PAELLA_OK) rc = check_required(who, q && k && v && o && lse, "q, k, v, o and lse");
    if (rc == PAELLA_OK) rc = check_ld(who, "ldq", ldq, nhead * D);
    if (rc == PAELLA_OK) rc = check_ld(who, "ldk", ldk, nhead * D);
    if (rc == PAELLA_OK) rc = check_ld(who, "ldv", ldv, nhead * D);
    if (rc == PAELLA_OK) rc = check_tensors_aligned16(who, q, k, v, o, lse);
    if (rc == PAELLA_OK) rc = check_p(who, p_drop);
    if (rc == PAELLA_OK && by_pointer) rc = check_seed_dev(who, p_drop, seed_dev);
    if (rc == PAELLA_OK) rc = check_workspace(who, ws, ws_bytes, plan_bytes(B, nhead, P), "paella_attn_train_workspace_bytes asks for");
    if (rc != PAELLA_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    const Geo g = make_geo(nhead, P, L, D, ldq, ldk, ldv, p_drop, seed, seed_dev);
    const dim3 grid((unsigned)((P + 15) / 16), (unsigned)nhead, (unsigned)B);
    ATTN_TRAIN_DISPATCH(D / 16, launch_fwd<DT>(p_drop > 0.f, grid, st, q, k, v, g, o, lse));
    LAUNCH_CHECK_RET();
    return PAELLA_OK;
}

int backward_impl(const char* who, const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* o, const float* lse, const float* dout, int B,
                  int nhead, int P, int L, int D, float p_drop, uint64_t seed, const uint64_t* seed_dev, bool by_pointer, float* dq, int lddq, float* dk, int lddk,
                  float* dv, int lddv, void* ws, size_t ws_bytes, void* stream) {
    int rc = check_shape(who, B, nhead, P, L, D);
    if (rc == PAELLA_OK) rc = check_required(who, q && k && v && o && lse && dout, "q, k, v, o, lse and do");
    if (rc == PAELLA_OK) rc = check_ld(who, "ldq", ldq, nhead * D);
    if (rc == PAELLA_OK) rc = check_ld(who, "ldk", ldk, nhead * D);
    if (rc == PAELLA_OK) rc = check_ld(who, "ldv", ldv, nhead * D);
    if (rc == PAELLA_OK && dq) rc = check_ld(who, "lddq", lddq, nhead * D);
    if (rc == PAELLA_OK && dk) rc = check_ld(who, "lddk", lddk, nhead * D);
    if (rc == PAELLA_OK && dv) rc = check_ld(who, "lddv", lddv, nhead * D);
    if (rc == PAELLA_OK) rc = check_tensors_aligned16(who, q, k, v, o, lse, dout, dq, dk, dv);
    if (rc == PAELLA_OK) rc = check_p(who, p_drop);
    if (rc == PAELLA_OK && by_pointer) rc = check_seed_dev(who, p_drop, seed_dev);
    if (rc == PAELLA_OK) rc = check_workspace(who, ws, ws_bytes, plan_bytes(B, nhead, P), "paella_attn_train_workspace_bytes asks for");
    if (rc != PAELLA_OK) return rc;
    if (!dq && !dk && !dv) return PAELLA_OK;
    hipStream_t st = (hipStream_t)stream;
    Geo g = make_geo(nhead, P, L, D, ldq, ldk, ldv, p_drop, seed, seed_dev);
    float* delta = (float*)ws;
    const int64_t rows = (int64_t)B * nhead * P;
    hipLaunchKernelGGL(attn_train_delta_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, o, dout, nhead, P, D, rows, delta);
    LAUNCH_CHECK_RET();
    const bool drop = p_drop > 0.f;
    if (dq) {
        g.ldg = lddq;
        const dim3 grid((unsigned)((P + 15) / 16), (unsigned)nhead, (unsigned)B);
        ATTN_TRAIN_DISPATCH(D / 16, launch_dq<DT>(drop, grid, st, q, k, v, lse, dout, (const float*)delta, g, dq));
        LAUNCH_CHECK_RET();
    }
    if (dk || dv) {
        g.ldg = lddk;
        g.ldg2 = lddv;
        const dim3 grid((unsigned)((L + 15) / 16), (unsigned)nhead, (unsigned)B);
        ATTN_TRAIN_DISPATCH(D / 16, launch_dkv<DT>(drop, grid, st, q, k, v, lse, dout, (const float*)delta, g, dk, dv));
        LAUNCH_CHECK_RET();
    }
    return PAELLA_OK;
}

}  // namespace

extern "C" int paella_attn_train_forward(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, int B, int nhead, int P, int L, int D, float p_drop,
                                         uint64_t seed, float* o, float* lse, void* ws, size_t ws_bytes, void* stream) {
    return forward_impl("attn_train_forward", q, ldq, k, ldk, v, ldv, B, nhead, P, L, D, p_drop, seed, nullptr, false, o, lse, ws, ws_bytes, stream);
}

extern "C" int paella_attn_train_forward_seed_dev(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, int B, int nhead, int P, int L, int D,
                                                  float p_drop, const uint64_t* seed_dev, float* o, float* lse, void* ws, size_t ws_bytes, void* stream) {
    return forward_impl("attn_train_forward_seed_dev", q, ldq, k, ldk, v, ldv, B, nhead, P, L, D, p_drop, 0ull, seed_dev, true, o, lse, ws, ws_bytes, stream);
}

extern "C" int paella_attn_train_backward(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* o, const float* lse, const float* dout,
                                          int B, int nhead, int P, int L, int D, float p_drop, uint64_t seed, float* dq, int lddq, float* dk, int lddk, float* dv,
                                          int lddv, void* ws, size_t ws_bytes, void* stream) {
    return backward_impl("attn_train_backward", q, ldq, k, ldk, v, ldv, o, lse, dout, B, nhead, P, L, D, p_drop, seed, nullptr, false, dq, lddq, dk, lddk, dv, lddv, ws,
                         ws_bytes, stream);
}

extern "C" int paella_attn_train_backward_seed_dev(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, const float* o, const float* lse,
                                                   const float* dout, int B, int nhead, int P, int L, int D, float p_drop, const uint64_t* seed_dev, float* dq, int lddq,
                                                   float* dk, int lddk, float* dv, int lddv, void* ws, size_t ws_bytes, void* stream) {
    return backward_impl("attn_train_backward_seed_dev", q, ldq, k, ldk, v, ldv, o, lse, dout, B, nhead, P, L, D, p_drop, 0ull, seed_dev, true, dq, lddq, dk, lddk, dv,
                         lddv, ws, ws_bytes, stream);
}
