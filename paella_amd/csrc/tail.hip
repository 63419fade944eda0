// Sampling tail of Paella's sample() loop for gfx950 (reference src/utils.py:45-54,
// src_distributed/utils.py:116-125) and add_noise (reference src/modules.py:277-283).
//
//   l       = l_c*cfg + l_u*(1-cfg)                (two roundings, no FMA: matches torch's two ops)
//   x       = l / T                                (IEEE division, as tensor.div)
//   token   = categorical(softmax(x))              == argmax_i exp(x_i - max)/q_i, q ~ Exp(1)
//             (torch.multinomial(p, 1) is argmax(p / q) with q = empty_like(p).exponential_(1))
//   renoise = u <= t_next ? init_noise : token     (torch.rand_like(x.float()) <= t)
//
// HBM-bound: one 256-thread workgroup per position streams the position's 2 x L logits with 16-byte
// lanes; max / argmax reductions are wave64 shuffles plus one LDS hop across the 4 waves.
// Noise comes either from caller-provided tensors (parity mode: bit-identical draws to torch given the
// same q / u) or from an in-kernel Philox4x32-10 stream keyed by (seed, offset).
#include "internal.h"
#include "test_hooks.h"
#include "philox.h"
#include "../../include/paella_hip.h"
#include <math.h>

#pragma clang fp contract(off)

// two roundings, as torch's two ops: plain operators under this file's contract(off) (__fmul_rn / __fadd_rn are header functions the
// pragma does not reach -- the score hook below had them fused into an fma)
__device__ __forceinline__ float mix_logit(float lc, float lu, float cfg, float omc, bool has_u) {
    return has_u ? lc * cfg + lu * omc : lc;
}

// renoise (src/utils.py:54 -> src/modules.py:277-283 with random_x = init_noise): u <= t_next ? init_noise : token
__device__ __forceinline__ int64_t tail_row_offset(const TailArgs& a) { return a.row_offset + (a.row_offset_ptr ? *a.row_offset_ptr : 0); }

// What a row draws with.  Scalar form: the launch's seed (+ device word), counters from the global row, the launch's cfg pair, temperature, step word and renoise threshold.
// Request form (REQ): everything from the tables of the row's request b = row / rows_per_sample, counters from the position inside the sample; the stream tables
// (step word, renoise threshold, active flag per request) are optional, null = the launch's scalar (kernel-uniform checks).
struct RowKey { uint64_t seed, step; int64_t ctr_row; float cfg, omc, temperature, t_next; bool active; };

// ctr_row: the row the Philox counter is built from -- the GLOBAL row (row + row offset), or in the request form the position inside the sample
__device__ __forceinline__ int64_t renoise_token(const TailArgs& a, const RowKey& k, int64_t row, int64_t tok) {
    if (a.init_noise) {
        float u;
        if (a.mask_u) {
            u = a.mask_u[row];
        } else {
            uint32_t rb[4];
            philox4x32(k.seed ^ 0x5bd1e9955bd1e995ull, (uint64_t)k.ctr_row, k.step, rb);
            u = u01_half_open(rb[0]);
        }
        if (u <= k.t_next) tok = a.init_noise[row];  // a negative per-request threshold never renoises: u >= 0
    }
    return tok;
}
// the optional pin (common.h: TailArgs::pin_keep / pin_tokens / pin_on), applied by the storing lane after the renoise and only when the row tables are there:
// the known token of a row whose mask says "known", in the request form only for the slots whose flag is set
template <bool REQ>
__device__ __forceinline__ int64_t pin_token(const TailArgs& a, int64_t row, int64_t tok) {
    if constexpr (REQ) {
        if (a.pin_on && a.pin_on[fast_div((unsigned)row, a.rq.rps_div)] == 0) return tok;
    }
    return a.pin_keep[row] == 0 ? a.pin_tokens[row] : tok;
}
template <bool REQ>
__device__ __forceinline__ RowKey tail_row_key(const TailArgs& a, int64_t row) {
    RowKey k;
    if constexpr (REQ) {
        const unsigned b = fast_div((unsigned)row, a.rq.rps_div);
        k.seed = a.rq.seeds[b];
        k.ctr_row = row - (int64_t)b * a.rq.rows_per_sample;
        k.cfg = a.rq.cfg_pairs ? a.rq.cfg_pairs[2 * b] : 1.f;
        k.omc = a.rq.cfg_pairs ? a.rq.cfg_pairs[2 * b + 1] : 0.f;
        k.temperature = a.rq.temperature[b];
        k.step = a.rq.step ? (uint64_t)a.rq.step[b] : a.offset;
        k.t_next = a.rq.t_next ? a.rq.t_next[b] : a.t_next;
        k.active = a.rq.active ? a.rq.active[b] != 0 : true;
    } else {
        k.seed = a.seed + (a.seed_ptr ? *a.seed_ptr : 0ull);
        k.ctr_row = row + tail_row_offset(a);
        k.cfg = a.cfg; k.omc = a.one_minus_cfg; k.temperature = a.temperature;
        k.step = a.offset; k.t_next = a.t_next; k.active = true;
    }
    return k;
}

template <bool REQ>
__global__ __launch_bounds__(256) void sample_tail_kernel(TailArgs a) {
    __shared__ float red_v[4];
    __shared__ int red_i[4];
    const int64_t row = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = a.L, L4 = L >> 2;
    const float* lc = a.logits_c + row * L;
    const float* lu = a.logits_u ? a.logits_u + row * L : nullptr;
    const bool has_u = lu != nullptr;
    const bool argmax_mode = a.mode == 1;
    const RowKey rk = tail_row_key<REQ>(a, row);
    const uint64_t seed = rk.seed;
    const float* nq = a.noise_q ? a.noise_q + row * L : nullptr;

    // pass 1 (explicit-noise parity mode only): max of x = mix / T for the softmax numerator exp(x - max).
    // The argmax and the counter-based mode never need it: argmax(x - log q) is invariant to a per-row shift.
    float mx = 0.f;
    if (nq && !argmax_mode) {
        mx = -INFINITY;
        for (int i4 = tid; i4 < L4; i4 += 256) {
            const f32x4 c = *reinterpret_cast<const f32x4*>(lc + i4 * 4);
            const f32x4 u = has_u ? *reinterpret_cast<const f32x4*>(lu + i4 * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < 4; ++e) mx = fmaxf(mx, __fdiv_rn(mix_logit(c[e], u[e], rk.cfg, rk.omc, has_u), rk.temperature));
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        if (lane == 0) red_v[wave] = mx;
        __syncthreads();
        mx = fmaxf(fmaxf(red_v[0], red_v[1]), fmaxf(red_v[2], red_v[3]));
        __syncthreads();
    }

    // pass 2: best score (first index wins ties)
    const float inv_t = tail_inv_temperature(rk.temperature);  // counter-based mode (philox.h: tail_score_gumbel)
    float best = -INFINITY;
    int best_i = 0x7fffffff;
    for (int i4 = tid; i4 < L4; i4 += 256) {
        const f32x4 c = *reinterpret_cast<const f32x4*>(lc + i4 * 4);
        const f32x4 u = has_u ? *reinterpret_cast<const f32x4*>(lu + i4 * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
        f32x4 q = f32x4{1.f, 1.f, 1.f, 1.f};
        if (!argmax_mode) {
            if (nq) {
                q = *reinterpret_cast<const f32x4*>(nq + i4 * 4);
            } else {
                uint32_t rb[4];
                philox4x32(seed, (uint64_t)rk.ctr_row * L4 + i4, rk.step, rb);
#pragma unroll
                for (int e = 0; e < 4; ++e) q[e] = log_exp1(rb[e]);
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float x = mix_logit(c[e], u[e], rk.cfg, rk.omc, has_u);
            float score;
            if (argmax_mode) {
                score = x;
            } else if (nq) {  // parity mode: the reference's arithmetic, softmax numerator over Exp(1) noise
                x = __fdiv_rn(x, rk.temperature);
                score = __fdiv_rn(expf(__fsub_rn(x, mx)), q[e]);
            } else {          // counter-based noise: the same draw in the log domain (Gumbel-max); identical arithmetic in the
                score = tail_score_gumbel(x, inv_t, q[e]);  // head GEMM's fused tail epilogue (gemm.hip)
            }
            argmax_update(best, best_i, score, i4 * 4 + e);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(best_i, o, 64);
        argmax_update(best, best_i, ov, oi);
    }
    if (lane == 0) { red_v[wave] = best; red_i[wave] = best_i; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) argmax_update(best, best_i, red_v[w], red_i[w]);
        if (best_i == 0x7fffffff) best_i = 0;  // all-NaN row
        int64_t tok = best_i;
        if (rk.active) {  // an idle slot of a request stream keeps what its rows held
            if (a.sampled_out) a.sampled_out[row] = tok;
            tok = renoise_token(a, rk, row, tok);
            if (a.pin_keep) tok = pin_token<REQ>(a, row, tok);  // (kernel-uniform: null = the unpinned tail)
            a.tokens_out[row] = tok;
        }
    }
}

// Second half of the FUSED tail: the head GEMM's epilogue (gemm.hip, TAIL instantiations) left, per row and column tile, the best
// (score, label) of that tile; pick the row's winner (first index wins ties -> identical to the one-kernel tail under any
// reduction order), renoise, store the token.  One wave per row: lane t reads tile t (coalesced), xor-shuffle argmax.
template <bool REQ>
__global__ __launch_bounds__(256) void tail_finalize_kernel(TailArgs a, const float* __restrict__ part_score, const int* __restrict__ part_idx,
                                                            int tiles_n) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.rows) return;
    float best = -INFINITY;
    int best_i = 0x7fffffff;
    const float* ps = part_score + row * tiles_n;
    const int* pi = part_idx + row * tiles_n;
    for (int t = lane; t < tiles_n; t += 64) argmax_update(best, best_i, ps[t], pi[t]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(best_i, o, 64);
        argmax_update(best, best_i, ov, oi);
    }
    if (lane == 0) {
        const RowKey rk = tail_row_key<REQ>(a, row);
        if (best_i == 0x7fffffff) best_i = 0;
        int64_t tok = best_i;
        if (rk.active) {
            if (a.sampled_out) a.sampled_out[row] = tok;
            tok = renoise_token(a, rk, row, tok);
            if (a.pin_keep) tok = pin_token<REQ>(a, row, tok);  // (kernel-uniform: null = the unpinned tail)
            a.tokens_out[row] = tok;
        }
    }
}

// request form: the tables must be there, the rows whole samples, the draw categorical from Philox; fills the division
static int tail_req_prepare(TailArgs& a) {
    const ReqTables& q = a.rq;
    if (!q.seeds || !q.temperature || a.rows <= 0 || a.rows > 0x7fffffff || a.rows % q.rows_per_sample || a.mode != 0 || a.noise_q || a.mask_u) {
        paella_set_error("request tail: needs seed and temperature tables, rows a multiple of rows_per_sample (%d), categorical mode and in-kernel noise", q.rows_per_sample);
        return PAELLA_ERR_ARG;
    }
    a.rq.rps_div = fast_div_of((unsigned)q.rows_per_sample);
    return PAELLA_OK;
}
#define RET_REQ(r) do { const int _rc = tail_req_prepare(r); if (_rc != PAELLA_OK) return _rc; } while (0)

// the pin tables of either form, checked here only (launchers and argument-block runners): both row tables or neither, categorical mode and in-kernel noise; pin_on belongs to the request form
int tail_pin_check(const char* who, const TailArgs& a) {
    if (!a.pin_keep && !a.pin_tokens && !a.pin_on) return PAELLA_OK;
    if (!a.pin_keep != !a.pin_tokens) { paella_set_error("%s: pin_keep and pin_tokens must be given together (one pin table without the other)", who); return PAELLA_ERR_ARG; }
    if (a.pin_on && (!a.pin_keep || a.rq.rows_per_sample <= 0)) { paella_set_error("%s: pin_on without the pin_keep / pin_tokens row tables, or outside the request form", who); return PAELLA_ERR_ARG; }
    if (a.mode != 0 || a.noise_q || a.mask_u) { paella_set_error("%s: the pin needs categorical mode and in-kernel noise (it is not offered in argmax mode)", who); return PAELLA_ERR_ARG; }
    return PAELLA_OK;
}
#define RET_PIN(a) do { const int _rc = tail_pin_check("sampling tail", a); if (_rc != PAELLA_OK) return _rc; } while (0)

int launch_tail_finalize(const TailArgs& a, const float* part_score, const int* part_idx, int tiles_n, hipStream_t st) {
    if (a.rows <= 0) return PAELLA_OK;
    RET_PIN(a);
    if (a.rq.rows_per_sample > 0) {
        TailArgs r = a;
        RET_REQ(r);
        hipLaunchKernelGGL(tail_finalize_kernel<true>, dim3((unsigned)((a.rows + 3) / 4)), dim3(256), 0, st, r, part_score, part_idx, tiles_n);
    } else hipLaunchKernelGGL(tail_finalize_kernel<false>, dim3((unsigned)((a.rows + 3) / 4)), dim3(256), 0, st, a, part_score, part_idx, tiles_n);
    LAUNCH_CHECK_RET();
    return PAELLA_OK;
}

int launch_sample_tail(const TailArgs& a, hipStream_t st) {
    if (a.rows <= 0) return PAELLA_OK;
    if (a.L & 3) { paella_set_error("sample_tail: num_labels %% 4 != 0"); return PAELLA_ERR_ARG; }
    if (a.rows > 0x7fffffff) { paella_set_error("sample_tail: too many rows"); return PAELLA_ERR_ARG; }
    RET_PIN(a);
    if (a.rq.rows_per_sample > 0) {
        TailArgs r = a;
        RET_REQ(r);
        hipLaunchKernelGGL(sample_tail_kernel<true>, dim3((unsigned)a.rows), dim3(256), 0, st, r);
    } else hipLaunchKernelGGL(sample_tail_kernel<false>, dim3((unsigned)a.rows), dim3(256), 0, st, a);
    LAUNCH_CHECK_RET();
    return PAELLA_OK;
}

// ---------------------------------------------------------------------------
// Truncated sampling (common.h: TailFilter): top-k, nucleus (top-p) and typical filtering of a row before the categorical draw.  A threshold filter needs whole-row
// statistics, so this is the one-kernel tail on MATERIALISED logits with the row's z = fp32(mix * inv_t) held in LDS (L * 4 bytes, written once), one 256-thread
// workgroup per row.  Every threshold -- the k-th largest z, the nucleus value v*, the typical distance d*, the min_tokens value -- comes from filter_threshold:
// bitwise bisection over an order-preserving 32-bit key, one workgroup reduction per bit, weight = count or exp(z - m).  Every reduction runs in one fixed order
// (per thread sequential over i = tid, tid + 256, ...; xor-shuffles inside the wave; one LDS hop across the 4 waves) and a label outside the tested set adds +0:
// rounding is monotone, so the sum is monotone in the set, the bisection is well defined and the kept set is bit-reproducible.  No atomics.
// The draw itself is the plain tail's: the same Philox words, the same scores, the same first-index arg-max -- over the kept labels only.
// ---------------------------------------------------------------------------
// smaller key = larger z (-0 == +0); z is never NaN here
__device__ __forceinline__ uint32_t filter_key_desc(float z) {
    const uint32_t b = __float_as_uint(z == 0.f ? 0.f : z);
    return (b & 0x80000000u) ? b : ~(b | 0x80000000u);
}
__device__ __forceinline__ float filter_key_desc_value(uint32_t key) {
    return __uint_as_float((key & 0x80000000u) ? key : (~key & 0x7fffffffu));
}
// typical filtering: d = |-log p - H| = |c - (z - m)| with c = sum (z - m) e / sum e (the log sum cancels); d >= 0, so its bit pattern is its key
__device__ __forceinline__ uint32_t filter_key_typ(float z, float m, float c) { return __float_as_uint(fabsf(c - (z - m))); }

struct FilterSums { float s, e; };
// sum of (v, w) over the workgroup in the fixed order; red: [2][4][2] floats, `phase` alternates so one barrier per reduction is enough
__device__ __forceinline__ FilterSums filter_reduce(float v, float w, float* red, int& phase) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { v += __shfl_xor(v, o, 64); w += __shfl_xor(w, o, 64); }
    float* r = red + phase * 8;
    if ((threadIdx.x & 63) == 0) { r[(threadIdx.x >> 6) * 2] = v; r[(threadIdx.x >> 6) * 2 + 1] = w; }
    __syncthreads();
    phase ^= 1;
    return FilterSums{(r[0] + r[2]) + (r[4] + r[6]), (r[1] + r[3]) + (r[5] + r[7])};
}
// The smallest tau such that the weight of {i in A : key_i <= tau} reaches target; 0xffffffff (= all of A) when even A does not reach it.
// A = {i : filter_key_desc(z_i) <= tau_a}; TYP: key = the typical distance, else the descending-z key; MASS: weight = exp(z - m), else 1.  Workgroup-uniform result.
template <bool TYP, bool MASS>
__device__ uint32_t filter_threshold(const float* zs, int L, uint32_t tau_a, float m, float c, float target, float* red, int& phase) {
    uint32_t prefix = 0;
    for (int bit = 32; bit >= 0; --bit) {
        const uint32_t t = bit == 32 ? 0xffffffffu : (prefix | ((1u << bit) - 1u));
        float acc = 0.f;
        for (int i = threadIdx.x; i < L; i += 256) {
            const float z = zs[i];
            const uint32_t ka = filter_key_desc(z);
            const uint32_t key = TYP ? filter_key_typ(z, m, c) : ka;
            const float w = MASS ? __expf(z - m) : 1.f;
            acc += (ka <= tau_a && key <= t) ? w : 0.f;
        }
        const bool reached = filter_reduce(acc, 0.f, red, phase).s >= target;
        if (bit == 32) { if (!reached) return 0xffffffffu; }
        else if (!reached) prefix |= 1u << bit;
    }
    return prefix;
}

// The kernel's body, shared by its two forms.  STATS (common.h: TailStats): the row's sums are formed whatever the filter says -- with every filter off too -- and
// the storing lane writes log p(token) and the entropy from them; the draw is the same draw.  zs [L] dynamic LDS, red [16], red_v / red_i [4] static LDS of the kernel.
template <bool REQ, bool STATS>
__device__ __forceinline__ void sample_tail_filter_body(const TailArgs& a, const TailFilter& f, const TailStats& st_out, float* zs, float* red, float* red_v, int* red_i) {
    const int64_t row = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int L = a.L, L4 = L >> 2;
    const float* lc = a.logits_c + row * L;
    const float* lu = a.logits_u ? a.logits_u + row * L : nullptr;
    const bool has_u = lu != nullptr;
    const RowKey rk = tail_row_key<REQ>(a, row);
    if (!rk.active) return;  // an idle slot of a request stream stores nothing (workgroup-uniform)
    const float inv_t = tail_inv_temperature(rk.temperature);

    // the row's filter, read once per workgroup
    int top_k = f.top_k, min_tokens = f.min_tokens;
    float top_p = f.top_p, typical = f.typical_mass;
    if constexpr (REQ) {
        if (!STATS || f.filter_k) {  // (the statistics form runs without the filter tables as well: every request off)
            const unsigned b = fast_div((unsigned)row, a.rq.rps_div);
            top_k = f.filter_k[2 * b]; min_tokens = f.filter_k[2 * b + 1];
            top_p = f.filter_mass[2 * b]; typical = f.filter_mass[2 * b + 1];
        }
    }
    const bool k_on = top_k >= 1 && top_k < L;
    const bool p_on = top_p > 0.f && top_p < 1.f;
    const bool t_on = !p_on && typical > 0.f && typical < 1.f;
    const bool hook = f.keep_out != nullptr;

    bool use = false, typ_b = false;  // the kept set: key_desc <= tau_a && (typ_b ? key_typ : key_desc) <= tau_b
    uint32_t tau_a = 0xffffffffu, tau_b = 0xffffffffu;
    float m = 0.f, c = 0.f, sum = 0.f;
    if (k_on || p_on || t_on || hook || STATS) {  // (workgroup-uniform: a row with every filter off runs the plain arg-max loop below and never touches zs)
        float mx = -INFINITY, bad = 0.f;
        for (int i4 = tid; i4 < L4; i4 += 256) {
            const f32x4 cc = *reinterpret_cast<const f32x4*>(lc + i4 * 4);
            const f32x4 uu = has_u ? *reinterpret_cast<const f32x4*>(lu + i4 * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
            f32x4 z;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                z[e] = mix_logit(cc[e], uu[e], rk.cfg, rk.omc, has_u) * inv_t;
                mx = fmaxf(mx, z[e]);
                if (z[e] != z[e]) bad = 1.f;
            }
            *reinterpret_cast<f32x4*>(zs + i4 * 4) = z;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { mx = fmaxf(mx, __shfl_xor(mx, o, 64)); bad = fmaxf(bad, __shfl_xor(bad, o, 64)); }
        if (lane == 0) { red[wave * 2] = mx; red[wave * 2 + 1] = bad; }
        __syncthreads();  // (also: zs is complete)
        mx = fmaxf(fmaxf(red[0], red[2]), fmaxf(red[4], red[6]));
        bad = fmaxf(fmaxf(red[1], red[3]), fmaxf(red[5], red[7]));
        int phase = 1;  // the first reduction below writes red[8..15]; red[0..7] is rewritten only after the barrier that follows these reads
        if (bad == 0.f && fabsf(mx) < INFINITY) {  // a NaN, or no finite maximum: the plain tail
            use = true;
            m = mx;
            if (k_on) tau_a = filter_threshold<false, false>(zs, L, 0xffffffffu, m, 0.f, (float)top_k, red, phase);
            if (p_on || t_on || hook || STATS) {
                float s = 0.f, e = 0.f;
                for (int i = tid; i < L; i += 256) {
                    const float z = zs[i];
                    const float w = filter_key_desc(z) <= tau_a ? __expf(z - m) : 0.f;
                    s += w;
                    e += w > 0.f ? (z - m) * w : 0.f;  // a label of probability 0 adds 0 to the entropy
                }
                const FilterSums st = filter_reduce(s, e, red, phase);
                sum = st.s;
                c = __fdiv_rn(st.e, st.s);
                if (p_on) tau_b = filter_threshold<false, true>(zs, L, tau_a, m, c, top_p * sum, red, phase);
                else if (t_on) { typ_b = true; tau_b = filter_threshold<true, true>(zs, L, tau_a, m, c, typical * sum, red, phase); }
                if ((p_on || t_on) && min_tokens > 1 && tau_b != 0xffffffffu) {
                    const float n = (float)(min_tokens < L + 1 ? min_tokens : L + 1);
                    const uint32_t tn = typ_b ? filter_threshold<true, false>(zs, L, tau_a, m, c, n, red, phase)
                                              : filter_threshold<false, false>(zs, L, tau_a, m, c, n, red, phase);
                    if (tn > tau_b) tau_b = tn;
                }
            }
        }
    }
    if (hook) {  // test hook: the selection only
        for (int i = tid; i < L; i += 256) {
            const float z = zs[i];
            f.keep_out[row * L + i] = (!use || (filter_key_desc(z) <= tau_a && (typ_b ? filter_key_typ(z, m, c) : filter_key_desc(z)) <= tau_b)) ? 1 : 0;
        }
        if (tid == 0 && f.rec_out) {
            const float nan = __uint_as_float(0x7fc00000u);
            const float ls = use ? logf(sum) : nan;
            const uint32_t tb = (p_on || t_on) ? tau_b : tau_a;
            const bool thr = use && (k_on || p_on || t_on) && tb != 0xffffffffu;
            f.rec_out[row * 4] = use ? m : nan;
            f.rec_out[row * 4 + 1] = ls;
            f.rec_out[row * 4 + 2] = ls - c;
            f.rec_out[row * 4 + 3] = !thr ? nan : typ_b ? __uint_as_float(tb) : filter_key_desc_value(tb);
        }
        return;
    }

    // the plain tail's draw (sample_tail_kernel, counter-based mode), over the kept labels
    float best = -INFINITY;
    int best_i = 0x7fffffff;
    for (int i4 = tid; i4 < L4; i4 += 256) {
        const f32x4 cc = *reinterpret_cast<const f32x4*>(lc + i4 * 4);
        const f32x4 uu = has_u ? *reinterpret_cast<const f32x4*>(lu + i4 * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
        f32x4 z = f32x4{0.f, 0.f, 0.f, 0.f};
        if (use) z = *reinterpret_cast<const f32x4*>(zs + i4 * 4);
        uint32_t rb[4];
        philox4x32(rk.seed, (uint64_t)rk.ctr_row * L4 + i4, rk.step, rb);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool kept = !use || (filter_key_desc(z[e]) <= tau_a && (typ_b ? filter_key_typ(z[e], m, c) : filter_key_desc(z[e])) <= tau_b);
            const float score = tail_score_gumbel(mix_logit(cc[e], uu[e], rk.cfg, rk.omc, has_u), inv_t, log_exp1(rb[e]));
            if (kept) argmax_update(best, best_i, score, i4 * 4 + e);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(best_i, o, 64);
        argmax_update(best, best_i, ov, oi);
    }
    if (lane == 0) { red_v[wave] = best; red_i[wave] = best_i; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) argmax_update(best, best_i, red_v[w], red_i[w]);
        if (best_i == 0x7fffffff) best_i = 0;  // all-NaN row
        int64_t tok = best_i;
        if constexpr (STATS) {  // log p(token) = (z_t - m) - log S and H = log S - E / S from the sums above, in their fixed order; the drawn label is always in A
            const float ls = logf(sum);
            if (st_out.logprob_out) st_out.logprob_out[row] = use ? (zs[best_i] - m) - ls : -INFINITY;
            if (st_out.entropy_out) st_out.entropy_out[row] = use ? ls - c : __uint_as_float(0x7fc00000u);
        }
        if (a.sampled_out) a.sampled_out[row] = tok;
        tok = renoise_token(a, rk, row, tok);
        if (a.pin_keep) tok = pin_token<REQ>(a, row, tok);
        a.tokens_out[row] = tok;
    }
}

template <bool REQ>
__global__ __launch_bounds__(256) void sample_tail_filter_kernel(TailArgs a, TailFilter f) {
    extern __shared__ float zs[];  // [L]
    __shared__ float red[16];
    __shared__ float red_v[4];
    __shared__ int red_i[4];
    sample_tail_filter_body<REQ, false>(a, f, TailStats{}, zs, red, red_v, red_i);
}
// the statistics form: the same body, two more stores in the storing lane
template <bool REQ>
__global__ __launch_bounds__(256) void sample_tail_stats_kernel(TailArgs a, TailFilter f, TailStats s) {
    extern __shared__ float zs[];  // [L]
    __shared__ float red[16];
    __shared__ float red_v[4];
    __shared__ int red_i[4];
    sample_tail_filter_body<REQ, true>(a, f, s, zs, red, red_v, red_i);
}

// the filter's own argument rules; everything here is host arithmetic, checked before anything is enqueued
static int tail_filter_check(const TailArgs& a, const TailFilter& f) {
    if (a.L > kTailFilterMaxLabels) {
        paella_set_error("sampling tail: the filter holds a row in LDS, num_labels (%d) is limited to %d", a.L, kTailFilterMaxLabels);
        return PAELLA_ERR_ARG;
    }
    if (a.mode != 0 || a.noise_q || a.mask_u) { paella_set_error("sampling tail: the filter needs categorical mode and in-kernel noise"); return PAELLA_ERR_ARG; }
    if (!f.filter_k != !f.filter_mass) { paella_set_error("sampling tail: filter_k and filter_mass must be given together"); return PAELLA_ERR_ARG; }
    if (f.filter_k && a.rq.rows_per_sample <= 0) { paella_set_error("sampling tail: the filter tables need the request form"); return PAELLA_ERR_ARG; }
    if (a.rq.rows_per_sample <= 0) {
        if (!(f.top_p > 0.f && f.top_p <= 1.f)) { paella_set_error("sampling tail: top_p must be in (0, 1] (1 = off)"); return PAELLA_ERR_ARG; }
        if (!(f.typical_mass > 0.f && f.typical_mass <= 1.f)) { paella_set_error("sampling tail: typical_mass must be in (0, 1] (1 = off)"); return PAELLA_ERR_ARG; }
        if (f.top_p < 1.f && f.typical_mass < 1.f) { paella_set_error("sampling tail: top_p and typical_mass are mutually exclusive (one mass filter at most)"); return PAELLA_ERR_ARG; }
        if (f.min_tokens < 1) { paella_set_error("sampling tail: min_tokens must be >= 1"); return PAELLA_ERR_ARG; }
    }
    return PAELLA_OK;
}

int launch_sample_tail_filter(const TailArgs& a, const TailFilter& f, hipStream_t st) {
    if (a.rows <= 0) return PAELLA_OK;
    if (a.L <= 0 || (a.L & 3)) { paella_set_error("sample_tail: num_labels %% 4 != 0"); return PAELLA_ERR_ARG; }
    if (a.rows > 0x7fffffff) { paella_set_error("sample_tail: too many rows"); return PAELLA_ERR_ARG; }
    const int rc = tail_filter_check(a, f);
    if (rc != PAELLA_OK) return rc;
    RET_PIN(a);
    const size_t lds = (size_t)a.L * sizeof(float);
    if (a.rq.rows_per_sample > 0) {
        if (!f.filter_k) return launch_sample_tail(a, st);  // no tables: the request form of the plain tail, the same launch
        TailArgs r = a;
        RET_REQ(r);
        if (lds > 48 * 1024) HIP_CHECK_RET(hipFuncSetAttribute(reinterpret_cast<const void*>(&sample_tail_filter_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(sample_tail_filter_kernel<true>, dim3((unsigned)a.rows), dim3(256), lds, st, r, f);
    } else {
        if (lds > 48 * 1024) HIP_CHECK_RET(hipFuncSetAttribute(reinterpret_cast<const void*>(&sample_tail_filter_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(sample_tail_filter_kernel<false>, dim3((unsigned)a.rows), dim3(256), lds, st, a, f);
    }
    LAUNCH_CHECK_RET();
    return PAELLA_OK;
}

// the statistics form of the filtered tail: the filter launcher's rules; in the request form the filter tables are optional (none = every request off)
int launch_sample_tail_stats(const TailArgs& a, const TailFilter& f, const TailStats& s, hipStream_t st) {
    if (a.rows <= 0) return PAELLA_OK;
    if (a.L <= 0 || (a.L & 3)) { paella_set_error("sample_tail: num_labels %% 4 != 0"); return PAELLA_ERR_ARG; }
    if (a.rows > 0x7fffffff) { paella_set_error("sample_tail: too many rows"); return PAELLA_ERR_ARG; }
    const int rc = tail_filter_check(a, f);
    if (rc != PAELLA_OK) return rc;
    RET_PIN(a);
    const size_t lds = (size_t)a.L * sizeof(float);
    if (a.rq.rows_per_sample > 0) {
        TailArgs r = a;
        RET_REQ(r);
        if (lds > 48 * 1024) HIP_CHECK_RET(hipFuncSetAttribute(reinterpret_cast<const void*>(&sample_tail_stats_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(sample_tail_stats_kernel<true>, dim3((unsigned)a.rows), dim3(256), lds, st, r, f, s);
    } else {
        if (lds > 48 * 1024) HIP_CHECK_RET(hipFuncSetAttribute(reinterpret_cast<const void*>(&sample_tail_stats_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(sample_tail_stats_kernel<false>, dim3((unsigned)a.rows), dim3(256), lds, st, a, f, s);
    }
    LAUNCH_CHECK_RET();
    return PAELLA_OK;
}

// ---------------------------------------------------------------------------
// Renoise stage (common.h: RenoiseArgs): per SAMPLE, which positions go back to init_noise after the draw.  One 256-thread workgroup per sample; policy 0 is
// renoise_token's independent coin per position, policy 1 renoises exactly n = rint(t_next * free positions) positions, the least confident first.  The sample's
// 32-bit keys live in LDS (HW * 4 bytes, written once); the n-th smallest (key, index) pair comes from two bitwise bisections with INTEGER counts -- 32 steps over
// the key for the threshold tau, then over the index among key == tau -- one workgroup reduction each, in filter_threshold's manner.  No atomics, no scratch, no
// per-thread arrays; plain loads and stores.  Everything a workgroup branches on (active, policy, n) is uniform over it.
// ---------------------------------------------------------------------------
// ascending order-preserving key of an fp32 score: smaller key = less confident; -0 == +0, NaN -> 0 (the least confident).  No score maps to 0xffffffff
__device__ __forceinline__ uint32_t renoise_key(float s) {
    if (s != s) return 0u;
    const uint32_t b = __float_as_uint(s == 0.f ? 0.f : s);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
static const uint32_t kRenoiseExcluded = 0xffffffffu;  // a position the pin owns: never counted, never selected
// sum of v over the workgroup; red: [2][4] ints, `phase` alternates so one barrier per reduction is enough
__device__ __forceinline__ int renoise_count(int v, int* red, int& phase) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    int* r = red + phase * 4;
    if ((threadIdx.x & 63) == 0) r[threadIdx.x >> 6] = v;
    __syncthreads();
    phase ^= 1;
    return (r[0] + r[1]) + (r[2] + r[3]);
}

template <bool REQ>
__global__ __launch_bounds__(256) void renoise_select_kernel(TailArgs a, RenoiseArgs r) {
    extern __shared__ uint32_t keys[];  // [HW]
    __shared__ int red[8];
    const unsigned b = blockIdx.x;
    const int tid = threadIdx.x, HW = r.rows_per_sample;
    const int64_t row0 = (int64_t)b * HW;
    // what the sample draws with: renoise_token's key, counter and step words (tail_row_key without the categorical draw's tables)
    uint64_t seed, step;
    int64_t ctr0;
    float t_next, g;
    int policy;
    bool pin = a.pin_keep != nullptr;
    if constexpr (REQ) {
        if (a.rq.active[b] == 0) return;  // an idle slot keeps what its rows held
        seed = a.rq.seeds[b]; ctr0 = 0; step = (uint64_t)a.rq.step[b]; t_next = a.rq.t_next[b];
        policy = r.policy_tab ? r.policy_tab[b] : 0;
        g = r.noise_tab ? r.noise_tab[b] : 0.f;
        if (pin && a.pin_on && a.pin_on[b] == 0) pin = false;
    } else {
        seed = a.seed + (a.seed_ptr ? *a.seed_ptr : 0ull); ctr0 = row0 + tail_row_offset(a); step = a.offset; t_next = a.t_next;
        policy = r.policy; g = r.confidence_noise;
    }
    seed ^= 0x5bd1e9955bd1e995ull;

    if (policy != 1) {  // random: renoise_token's coin, then the pin
        for (int p = tid; p < HW; p += 256) {
            const int64_t row = row0 + p;
            uint32_t rb[4];
            philox4x32(seed, (uint64_t)(ctr0 + p), step, rb);
            int64_t tok = u01_half_open(rb[0]) <= t_next ? a.init_noise[row] : r.drawn[row];
            if (pin && a.pin_keep[row] == 0) tok = a.pin_tokens[row];
            if (r.scores_out) r.scores_out[row] = r.logprob ? r.logprob[row] : 0.f;
            a.tokens_out[row] = tok;
        }
        return;
    }

    // confidence: the keys of the free positions, and how many there are
    const float gt = g * t_next;
    int mine = 0;
    for (int p = tid; p < HW; p += 256) {
        const int64_t row = row0 + p;
        float score = r.logprob[row];
        const bool pinned = pin && a.pin_keep[row] == 0;
        if (g != 0.f && !pinned) {
            uint32_t rb[4];
            philox4x32(seed, (uint64_t)(ctr0 + p), step, rb);
            score = __builtin_fmaf(-gt, log_exp1(rb[1]), score);
        }
        if (r.scores_out) r.scores_out[row] = score;
        keys[p] = pinned ? kRenoiseExcluded : renoise_key(score);
        mine += pinned ? 0 : 1;
    }
    int phase = 0;
    const int n_free = renoise_count(mine, red, phase);  // (the barrier inside also completes `keys`)
    int n = __float2int_rn(t_next * (float)n_free);      // (a NaN threshold converts to 0)
    n = n < 0 ? 0 : (n > n_free ? n_free : n);

    uint32_t tau = 0u;
    int cut = -1;  // selected = key < tau || (key == tau && index <= cut)
    if (n > 0) {
        // the smallest tau with |{free : key <= tau}| >= n
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t t = tau | ((1u << bit) - 1u);
            int cnt = 0;
            for (int p = tid; p < HW; p += 256) { const uint32_t k = keys[p]; cnt += (k != kRenoiseExcluded && k <= t) ? 1 : 0; }
            if (renoise_count(cnt, red, phase) < n) tau |= 1u << bit;
        }
        // of the positions with key == tau the first `need` by index: the smallest cut with |{key == tau, index <= cut}| >= need
        int below = 0;
        for (int p = tid; p < HW; p += 256) below += keys[p] < tau ? 1 : 0;
        const int need = n - renoise_count(below, red, phase);
        int top = 0;
        while ((1 << top) < HW) ++top;
        cut = 0;
        for (int bit = top - 1; bit >= 0; --bit) {
            const int t = cut | ((1 << bit) - 1);
            int cnt = 0;
            for (int p = tid; p < HW; p += 256) cnt += (keys[p] == tau && p <= t) ? 1 : 0;
            if (renoise_count(cnt, red, phase) < need) cut |= 1 << bit;
        }
    }
    for (int p = tid; p < HW; p += 256) {
        const int64_t row = row0 + p;
        const uint32_t k = keys[p];
        int64_t tok;
        if (k == kRenoiseExcluded) tok = a.pin_tokens[row];
        else tok = (k < tau || (k == tau && p <= cut)) ? a.init_noise[row] : r.drawn[row];
        a.tokens_out[row] = tok;
    }
}

int launch_renoise_select(const TailArgs& a, const RenoiseArgs& r, hipStream_t st) {
    const bool req = a.rq.rows_per_sample > 0;
    if (!r.drawn || !a.init_noise || !a.tokens_out) { paella_set_error("renoise_select: null argument (drawn / init_noise / tokens_out)"); return PAELLA_ERR_ARG; }
    if (r.rows_per_sample < 1 || r.rows_per_sample > kTailFilterMaxLabels) {
        paella_set_error("renoise_select: a sample's keys live in LDS, rows_per_sample (%d) must be 1 ... %d", r.rows_per_sample, kTailFilterMaxLabels);
        return PAELLA_ERR_ARG;
    }
    if (a.rows < 0 || a.rows % r.rows_per_sample || a.rows / r.rows_per_sample > 0x7fffffff) {
        paella_set_error("renoise_select: rows (%lld) must be a multiple of rows_per_sample (%d): the selection is per sample", (long long)a.rows, r.rows_per_sample);
        return PAELLA_ERR_ARG;
    }
    if (!a.pin_keep != !a.pin_tokens) { paella_set_error("renoise_select: pin_keep and pin_tokens must be given together (one pin table without the other)"); return PAELLA_ERR_ARG; }
    if (a.pin_on && !a.pin_keep) { paella_set_error("renoise_select: pin_on without the pin_keep / pin_tokens row tables"); return PAELLA_ERR_ARG; }
    if (req) {
        if (!a.rq.seeds || !a.rq.step || !a.rq.t_next || !a.rq.active) { paella_set_error("renoise_select_stream: null argument (the seeds, step, t_next and active tables are required)"); return PAELLA_ERR_ARG; }
        if (r.policy_tab && !r.logprob) { paella_set_error("renoise_select_stream: a policy table (policy 1 = confidence) needs logprob"); return PAELLA_ERR_ARG; }
    } else {
        if (a.row_offset < 0) { paella_set_error("renoise_select: row_offset must be >= 0"); return PAELLA_ERR_ARG; }
        if (r.policy != 0 && r.policy != 1) { paella_set_error("renoise_select: policy must be 0 (random) or 1 (confidence), got %d", r.policy); return PAELLA_ERR_ARG; }
        if (!(r.confidence_noise >= 0.f) || !(r.confidence_noise < INFINITY)) { paella_set_error("renoise_select: confidence_noise must be finite and >= 0"); return PAELLA_ERR_ARG; }
        if (r.policy == 1 && !r.logprob) { paella_set_error("renoise_select: policy 1 (confidence) needs logprob"); return PAELLA_ERR_ARG; }
    }
    if (a.rows == 0) return PAELLA_OK;
    const size_t lds = (size_t)r.rows_per_sample * sizeof(uint32_t);
    const dim3 grid((unsigned)(a.rows / r.rows_per_sample));
    if (req) {
        if (lds > 48 * 1024) HIP_CHECK_RET(hipFuncSetAttribute(reinterpret_cast<const void*>(&renoise_select_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(renoise_select_kernel<true>, grid, dim3(256), lds, st, a, r);
    } else {
        if (lds > 48 * 1024) HIP_CHECK_RET(hipFuncSetAttribute(reinterpret_cast<const void*>(&renoise_select_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(renoise_select_kernel<false>, grid, dim3(256), lds, st, a, r);
    }
    LAUNCH_CHECK_RET();
    return PAELLA_OK;
}

// ---------------------------------------------------------------------------
// The argument block of a sampling tail (include/paella_hip.h: paella_tail_args): tail_block_convert is the one place where a block's rules are checked and where it becomes
// TailArgs / TailFilter / TailStats; every paella_sample_tail* entry point (end of this file) and every fused step of model.hip fills a block, names itself and goes through it.
// need (internal.h: kNeed*): what a fixed-form entry point's NAME promises on top of what its block holds; a block alone takes its form from what is present.  fused: the tail
// of a fused step (the head GEMM holds the logits and the guidance mix; the caller fills a.rows / a.L).  *kind: 0 launch_sample_tail, 1 ..._filter, 2 ..._stats
// ---------------------------------------------------------------------------
int tail_block_convert(const char* who, const paella_tail_args& t, int need, bool fused, TailArgs& a, TailFilter& f, TailStats& s, int* kind) {
    const bool tables = t.seeds || t.temperature_tab || t.cfg_pairs || t.step || t.t_next_tab || t.active;
    if (t.rows_per_sample < 0 || (t.rows_per_sample == 0 && (tables || (need & (kNeedRequest | kNeedStream))))) {
        paella_set_error("%s: rows_per_sample must be > 0 (the request tables need the request form)", who);
        return PAELLA_ERR_ARG;
    }
    const bool req = t.rows_per_sample > 0, strm = t.step || t.t_next_tab || t.active || (need & kNeedStream);
    if ((!fused && !t.logits_c) || !t.tokens_out || (req && (!t.seeds || !t.temperature_tab))) {
        paella_set_error("%s: null argument (%stokens_out%s)", who, fused ? "" : "logits_c / ", req ? " / seeds / temperature" : "");
        return PAELLA_ERR_ARG;
    }
    if (strm && (!t.step || !t.t_next_tab || !t.active || !t.init_noise)) {
        paella_set_error("%s: null argument (the step, t_next and active tables and init_noise, the renoise source of every slot, are required)", who);
        return PAELLA_ERR_ARG;
    }
    if (!req && t.mode == 0 && !(t.temperature > 0.f)) { paella_set_error("%s: temperature must be > 0 in categorical mode (use mode=1 for argmax)", who); return PAELLA_ERR_ARG; }
    if (!req && t.row_offset < 0) { paella_set_error("%s: row_offset must be >= 0", who); return PAELLA_ERR_ARG; }
    a = TailArgs{};
    a.logits_c = fused ? nullptr : t.logits_c; a.rows = t.rows; a.L = t.L;
    a.noise_q = fused ? nullptr : t.noise_q; a.mask_u = fused ? nullptr : t.mask_u;
    a.cfg = 1.f; a.one_minus_cfg = 0.f; a.temperature = 1.f;
    a.offset = strm ? 0 : t.offset; a.t_next = strm ? -1.f : t.t_next;
    a.init_noise = t.init_noise; a.tokens_out = t.tokens_out; a.sampled_out = fused ? nullptr : t.sampled_out;
    a.pin_keep = t.pin_keep; a.pin_tokens = t.pin_tokens; a.pin_on = t.pin_on;
    if (req) {
        if (!fused) { a.logits_u = t.cfg_pairs ? t.logits_u : nullptr; a.rq.cfg_pairs = t.cfg_pairs; }  // (fused: the pairs ride through the head, none left for the tail)
        a.rq.seeds = t.seeds; a.rq.temperature = t.temperature_tab; a.rq.rows_per_sample = t.rows_per_sample;
        a.rq.step = t.step; a.rq.t_next = t.t_next_tab; a.rq.active = t.active;
    } else {
        if (!fused) { a.logits_u = t.logits_u; a.cfg = t.cfg; a.one_minus_cfg = t.one_minus_cfg; }
        a.temperature = t.temperature; a.mode = t.mode; a.seed = t.seed; a.seed_ptr = t.seed_ptr; a.row_offset = t.row_offset; a.row_offset_ptr = t.row_offset_ptr;
    }
    RET_IF(tail_pin_check(who, a));
    f = TailFilter{}; s = TailStats{};
    const bool stats = t.logprob_out || t.entropy_out;
    bool filter = t.filter_k || t.filter_mass;
    if (!req && ((need & kNeedFilter) || t.top_k != 0 || t.top_p != 0.f || t.typical_mass != 0.f || t.min_tokens != 0)) {
        filter = true;
        f.top_k = t.top_k; f.top_p = t.top_p; f.typical_mass = t.typical_mass; f.min_tokens = t.min_tokens;
    }
    if ((filter || stats) && fused) { paella_set_error("%s: the filter and the statistics need materialised logits (a logits forward + paella_sample_tail_args)", who); return PAELLA_ERR_ARG; }
    if ((filter || stats) && a.mode != 0) { paella_set_error("%s: the filter and the statistics are not offered in argmax mode", who); return PAELLA_ERR_ARG; }
    if (!t.filter_k != !t.filter_mass) { paella_set_error("%s: filter_k and filter_mass must be given together (one filter table without the other)", who); return PAELLA_ERR_ARG; }
    f.filter_k = t.filter_k; f.filter_mass = t.filter_mass;
    s.logprob_out = t.logprob_out; s.entropy_out = t.entropy_out;
    *kind = stats ? 2 : filter ? 1 : 0;
    return PAELLA_OK;
}

static int renoise_select_scalar(const int64_t* drawn, const float* logprob, const int64_t* init_noise, int64_t rows, int rows_per_sample, uint64_t seed,
                                 const uint64_t* seed_ptr, uint64_t offset, int64_t row_offset, const int64_t* row_offset_ptr, float t_next, int policy,
                                 float confidence_noise, const int64_t* pin_keep, const int64_t* pin_tokens, int64_t* tokens_out, float* scores_out, void* stream) {
    TailArgs a = {};
    a.rows = rows; a.seed = seed; a.seed_ptr = seed_ptr; a.offset = offset; a.row_offset = row_offset; a.row_offset_ptr = row_offset_ptr;
    a.init_noise = init_noise; a.t_next = t_next; a.tokens_out = tokens_out; a.pin_keep = pin_keep; a.pin_tokens = pin_tokens;
    RenoiseArgs r;
    r.drawn = drawn; r.logprob = logprob; r.rows_per_sample = rows_per_sample; r.policy = policy; r.confidence_noise = confidence_noise; r.scores_out = scores_out;
    return launch_renoise_select(a, r, (hipStream_t)stream);
}
static int renoise_select_stream(const int64_t* drawn, const float* logprob, const int64_t* init_noise, int64_t rows, int rows_per_sample, const uint64_t* seeds,
                                 const int* step, const float* t_next, const int* active, const int* policy, const float* confidence_noise, const int64_t* pin_keep,
                                 const int64_t* pin_tokens, const int* pin_on, int64_t* tokens_out, float* scores_out, void* stream) {
    TailArgs a = {};
    a.rows = rows; a.init_noise = init_noise; a.t_next = -1.f; a.tokens_out = tokens_out; a.pin_keep = pin_keep; a.pin_tokens = pin_tokens; a.pin_on = pin_on;
    a.rq.seeds = seeds; a.rq.step = step; a.rq.t_next = t_next; a.rq.active = active; a.rq.rows_per_sample = rows_per_sample > 0 ? rows_per_sample : 1;
    RenoiseArgs r;
    r.drawn = drawn; r.logprob = logprob; r.rows_per_sample = rows_per_sample; r.policy_tab = policy; r.noise_tab = confidence_noise; r.scores_out = scores_out;
    return launch_renoise_select(a, r, (hipStream_t)stream);
}
extern "C" int paella_renoise_select(const int64_t* drawn, const float* logprob, const int64_t* init_noise, int64_t rows, int rows_per_sample, uint64_t seed,
                                     const uint64_t* seed_ptr, uint64_t offset, int64_t row_offset, const int64_t* row_offset_ptr, float t_next, int policy,
                                     float confidence_noise, const int64_t* pin_keep, const int64_t* pin_tokens, int64_t* tokens_out, void* stream) {
    return renoise_select_scalar(drawn, logprob, init_noise, rows, rows_per_sample, seed, seed_ptr, offset, row_offset, row_offset_ptr, t_next, policy, confidence_noise,
                                 pin_keep, pin_tokens, tokens_out, nullptr, stream);
}
extern "C" int paella_renoise_select_stream(const int64_t* drawn, const float* logprob, const int64_t* init_noise, int64_t rows, int rows_per_sample,
                                            const uint64_t* seeds, const int* step, const float* t_next, const int* active, const int* policy,
                                            const float* confidence_noise, const int64_t* pin_keep, const int64_t* pin_tokens, const int* pin_on, int64_t* tokens_out,
                                            void* stream) {
    return renoise_select_stream(drawn, logprob, init_noise, rows, rows_per_sample, seeds, step, t_next, active, policy, confidence_noise, pin_keep, pin_tokens, pin_on,
                                 tokens_out, nullptr, stream);
}
// test hook (test_hooks.h): the renoise stage with its fp32 scores written out -- scores_out [rows] = what the kernel ranked (policy-0 slots: logprob, 0 without one).
// seeds == NULL: the scalar form (seed, offset, row_offset, t_next, policy, confidence_noise by value); otherwise the stream form's tables.
extern "C" int paella_test_renoise_scores(const int64_t* drawn, const float* logprob, const int64_t* init_noise, int64_t rows, int rows_per_sample, uint64_t seed,
                                          uint64_t offset, int64_t row_offset, float t_next, int policy, float confidence_noise, const uint64_t* seeds, const int* step,
                                          const float* t_next_tab, const int* active, const int* policy_tab, const float* noise_tab, const int64_t* pin_keep,
                                          const int64_t* pin_tokens, const int* pin_on, int64_t* tokens_out, float* scores_out, void* stream) {
    if (!scores_out) { paella_set_error("renoise_scores: scores_out is required"); return PAELLA_ERR_ARG; }
    if (seeds)
        return renoise_select_stream(drawn, logprob, init_noise, rows, rows_per_sample, seeds, step, t_next_tab, active, policy_tab, noise_tab, pin_keep, pin_tokens, pin_on,
                                     tokens_out, scores_out, stream);
    return renoise_select_scalar(drawn, logprob, init_noise, rows, rows_per_sample, seed, nullptr, offset, row_offset, nullptr, t_next, policy, confidence_noise, pin_keep,
                                 pin_tokens, tokens_out, scores_out, stream);
}

// ---------------------------------------------------------------------------
// One tick of a request stream (continuous batching; paella_amd.RequestStream): every slot b of the fixed-shape batch runs its own PROGRAM, one row per step,
//   program [B, max_steps, 5] fp32: row j = (r_j, temperature_j, cfg_j, 1 - cfg_j, t_next_j)       cursor pos[b], length len[b]
// and this launch turns the cursors into the flat per-slot tables the forward's timestep kernel and the stream form of the tail read at this tick, then advances
// the cursors of the running slots.  A slot whose cursor reached its length is idle: finite placeholder values, active 0 (the tail stores nothing for it).
// Editing stream: an optional policy per slot (0 never, 1 every step, 2 the request's final step only) becomes this tick's flag pin_on[b] the pinned tail reads;
// with a null policy table the kernel stores exactly what it stores without one.
// One thread per slot, plain loads and stores; a slot is touched by its own thread only.  Graph-capturable: everything is device state.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void request_step_kernel(const float* __restrict__ program, int max_steps, int* __restrict__ pos, const int* __restrict__ len, int B,
                                                           float* __restrict__ r, float* __restrict__ temperature, float* __restrict__ pairs,
                                                           float* __restrict__ t_next, int* __restrict__ step, int* __restrict__ active,
                                                           const int* __restrict__ pin_policy, int* __restrict__ pin_on) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const int p = pos[b];
    const int n = len[b];
    const bool on = p >= 0 && p < n && p < max_steps;  // (the last two conditions keep a corrupt cursor or length inside the program)
    float v[5] = {0.f, 1.f, 1.f, 0.f, -1.f};
    if (on) {
        const float* row = program + ((size_t)b * max_steps + p) * 5;
#pragma unroll
        for (int e = 0; e < 5; ++e) v[e] = row[e];
    }
    r[b] = v[0];
    temperature[b] = v[1];
    if (pairs) { pairs[2 * b] = v[2]; pairs[2 * b + 1] = v[3]; }
    t_next[b] = v[4];
    step[b] = p;
    active[b] = on ? 1 : 0;
    if (pin_policy) {
        const int pol = pin_policy[b];
        pin_on[b] = (on && (pol == 1 || (pol == 2 && p + 1 == n))) ? 1 : 0;
    }
    if (on) pos[b] = p + 1;
}
int launch_request_step(const float* program, int max_steps, int* pos, const int* len, int B, float* r, float* temperature, float* pairs, float* t_next,
                        int* step, int* active, const int* pin_policy, int* pin_on, hipStream_t st) {
    if (!program || !pos || !len || !r || !temperature || !t_next || !step || !active || B <= 0 || max_steps <= 0) {
        paella_set_error("request_step: null table, B <= 0 or max_steps <= 0");
        return PAELLA_ERR_ARG;
    }
    if (!pin_policy != !pin_on) { paella_set_error("request_step: pin_policy and pin_on must be given together"); return PAELLA_ERR_ARG; }
    hipLaunchKernelGGL(request_step_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, st, program, max_steps, pos, len, B, r, temperature, pairs, t_next, step, active,
                       pin_policy, pin_on);
    LAUNCH_CHECK_RET();
    return PAELLA_OK;
}

// ---------------------------------------------------------------------------
// Start tokens of the counter-based noise mode: the reference draws randint(0, num_labels, (B, H, W)) from torch's global generator
// (src/utils.py:37), a stream that cannot be sharded.  Here token i of the GLOBAL grid is a function of (seed, i) alone, so a batch
// shard draws exactly the start tokens the unsharded call gives its rows, at O(shard) cost, and -- seed and row offset being optional
// device-resident words -- from inside a captured graph.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void start_tokens_kernel(uint64_t seed, const uint64_t* __restrict__ seed_ptr, int64_t row_offset,
                                                           const int64_t* __restrict__ row_offset_ptr, int num_labels, int64_t n,
                                                           int64_t* __restrict__ out) {
    const uint64_t s = (seed + (seed_ptr ? *seed_ptr : 0ull)) ^ 0x9e3779b97f4a7c15ull;
    const int64_t off = row_offset + (row_offset_ptr ? *row_offset_ptr : 0);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        uint32_t rb[4];
        philox4x32(s, (uint64_t)(i + off), ~0ull, rb);
        out[i] = (int64_t)((((uint64_t)rb[0] << 32) | rb[1]) % (uint64_t)num_labels);
    }
}
int launch_start_tokens(uint64_t seed, const uint64_t* seed_ptr, int64_t row_offset, const int64_t* row_offset_ptr, int num_labels, int64_t n,
                        int64_t* out, hipStream_t st) {
    if (n <= 0) return PAELLA_OK;
    if (!out || num_labels <= 0 || row_offset < 0) { paella_set_error("start_tokens: bad arguments"); return PAELLA_ERR_ARG; }
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(start_tokens_kernel, dim3((unsigned)blocks), dim3(256), 0, st, seed, seed_ptr, row_offset, row_offset_ptr, num_labels, n, out);
    LAUNCH_CHECK_RET();
    return PAELLA_OK;
}

// request batch: sample b draws the start tokens of seeds[b] sampled alone (counter = the position inside the sample)
__global__ __launch_bounds__(256) void start_tokens_req_kernel(const uint64_t* __restrict__ seeds, FastDiv rps_div, int rows_per_sample, int num_labels, int64_t n,
                                                               int64_t* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const unsigned b = fast_div((unsigned)i, rps_div);
        uint32_t rb[4];
        philox4x32(seeds[b] ^ 0x9e3779b97f4a7c15ull, (uint64_t)(i - (int64_t)b * rows_per_sample), ~0ull, rb);
        out[i] = (int64_t)((((uint64_t)rb[0] << 32) | rb[1]) % (uint64_t)num_labels);
    }
}
int launch_start_tokens_req(const uint64_t* seeds, int B, int rows_per_sample, int num_labels, int64_t* out, hipStream_t st) {
    const int64_t n = (int64_t)B * rows_per_sample;
    if (!seeds || !out || B <= 0 || rows_per_sample <= 0 || num_labels <= 0 || n > 0x7fffffff) { paella_set_error("start_tokens_req: bad arguments"); return PAELLA_ERR_ARG; }
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(start_tokens_req_kernel, dim3((unsigned)blocks), dim3(256), 0, st, seeds, fast_div_of((unsigned)rows_per_sample), rows_per_sample, num_labels, n, out);
    LAUNCH_CHECK_RET();
    return PAELLA_OK;
}

// ---------------------------------------------------------------------------
// add_noise: mask = (U[0,1) <= t[b]).long(); x*(1-mask) + random_x*mask   (int64 arithmetic as written)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void add_noise_kernel(const int64_t* __restrict__ x, const float* __restrict__ t,
                                                        const int64_t* __restrict__ mask_in, const int64_t* __restrict__ random_x,
                                                        const float* __restrict__ rand_u, uint64_t seed, uint64_t offset,
                                                        int num_labels, int64_t total, int64_t per_sample,
                                                        int64_t* __restrict__ x_out, int64_t* __restrict__ mask_out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        uint32_t rb[4] = {0, 0, 0, 0};
        if ((!mask_in && !rand_u) || !random_x) philox4x32(seed, (uint64_t)i, offset, rb);
        int64_t m;
        if (mask_in) m = mask_in[i];
        else {
            const float u = rand_u ? rand_u[i] : u01_half_open(rb[0]);
            m = (u <= t[i / per_sample]) ? 1 : 0;
        }
        const int64_t rx = random_x ? random_x[i] : (int64_t)((((uint64_t)rb[1] << 32) | rb[2]) % (uint64_t)num_labels);
        x_out[i] = x[i] * (1 - m) + rx * m;
        if (mask_out) mask_out[i] = m;
    }
}

int launch_add_noise(const int64_t* x, const float* t, const int64_t* mask_in, const int64_t* random_x,
                     const float* rand_u, uint64_t seed, uint64_t offset, int num_labels, int B, int64_t per_sample,
                     int64_t* x_out, int64_t* mask_out, hipStream_t st) {
    const int64_t total = (int64_t)B * per_sample;
    if (total <= 0) return PAELLA_OK;
    int64_t blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(add_noise_kernel, dim3((unsigned)blocks), dim3(256), 0, st, x, t, mask_in, random_x, rand_u, seed,
                       offset, num_labels, total, per_sample, x_out, mask_out);
    LAUNCH_CHECK_RET();
    return PAELLA_OK;
}

// ---------------------------------------------------------------------------
// Token select: out[i] = keep(i) ? a[i] : (b ? b[i] : fill), keep(i) = (mask == null || mask[i] != 0) && (flag == null || *flag == 1.0f).
// Two users, both integer elementwise work on the [B, H, W] grid that used to go through ATen: the inpainting wrapper re-imposes the known tokens
// (`out * mask + tokens * (1 - mask)`, paella_amd/editing.py -- an extension of the recipe src/modules.py:277-283 + src_distributed/utils.py:97-109) and the
// batch-sharded sampler replaces a receiver's tokens by -1 when the conditioning broadcast carried a zero validity flag (paella_amd/dist.py).  `flag` is a
// DEVICE word, so neither needs a host round trip and both can be captured in a HIP graph.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void select_tokens_kernel(const int64_t* __restrict__ a, const int64_t* __restrict__ b, const int64_t* __restrict__ mask,
                                                            const float* __restrict__ flag, int64_t fill, int64_t n, int64_t* __restrict__ out) {
    const bool ok = flag ? (*flag == 1.0f) : true;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const bool keep = ok && (mask ? mask[i] != 0 : true);
        out[i] = keep ? a[i] : (b ? b[i] : fill);
    }
}
int launch_select_tokens(const int64_t* a, const int64_t* b, const int64_t* mask, const float* flag, int64_t fill, int64_t n, int64_t* out, hipStream_t st) {
    if (n <= 0) return PAELLA_OK;
    if (!a || !out) { paella_set_error("select_tokens: null argument"); return PAELLA_ERR_ARG; }
    int64_t blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(select_tokens_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a, b, mask, flag, fill, n, out);
    LAUNCH_CHECK_RET();
    return PAELLA_OK;
}

// ---------------------------------------------------------------------------
// test hook (test_hooks.h): the scores the counter-based tail maximises, written out -- score[row][i] = mix(l_c, l_u)[i] / T - log q_i
// with exactly the kernels' arithmetic and Philox counters.  Lets a test classify a differing token by the decision margin
// (top-1 minus top-2 score) instead of bounding a mismatch count.
// ---------------------------------------------------------------------------
template <bool REQ>
__global__ __launch_bounds__(256) void tail_scores_kernel(TailArgs a, float* __restrict__ scores) {
    const int64_t row = blockIdx.x;
    const int L = a.L, L4 = L >> 2;
    const float* lc = a.logits_c + row * L;
    const float* lu = a.logits_u ? a.logits_u + row * L : nullptr;
    const bool has_u = lu != nullptr;
    const RowKey rk = tail_row_key<REQ>(a, row);
    for (int i4 = threadIdx.x; i4 < L4; i4 += 256) {
        const f32x4 c = *reinterpret_cast<const f32x4*>(lc + i4 * 4);
        const f32x4 u = has_u ? *reinterpret_cast<const f32x4*>(lu + i4 * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
        uint32_t rb[4];
        philox4x32(rk.seed, (uint64_t)rk.ctr_row * L4 + i4, rk.step, rb);
        f32x4 s;
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] = tail_score_gumbel(mix_logit(c[e], u[e], rk.cfg, rk.omc, has_u), tail_inv_temperature(rk.temperature), log_exp1(rb[e]));
        *reinterpret_cast<f32x4*>(scores + row * L + i4 * 4) = s;
    }
}
extern "C" int paella_test_tail_scores(const float* logits_c, const float* logits_u, int64_t rows, int L, float cfg, float one_minus_cfg,
                                       float temperature, uint64_t seed, uint64_t offset, int64_t row_offset, float* scores_out, void* stream) {
    if (!logits_c || !scores_out || (L & 3) || rows <= 0 || rows > 0x7fffffff || !(temperature > 0.f)) { paella_set_error("tail_scores: bad arguments"); return PAELLA_ERR_ARG; }
    TailArgs a = {};
    a.logits_c = logits_c; a.logits_u = logits_u; a.rows = rows; a.L = L; a.cfg = cfg; a.one_minus_cfg = one_minus_cfg; a.temperature = temperature;
    a.seed = seed; a.offset = offset; a.row_offset = row_offset;
    hipLaunchKernelGGL(tail_scores_kernel<false>, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, a, scores_out);
    LAUNCH_CHECK_RET();
    return PAELLA_OK;
}
extern "C" int paella_test_tail_scores_req(const float* logits_c, const float* logits_u, int64_t rows, int L, const float* cfg_pairs, const float* temperature,
                                           const uint64_t* seeds, int rows_per_sample, uint64_t offset, float* scores_out, void* stream) {
    if (!logits_c || !scores_out || (L & 3) || rows_per_sample <= 0) { paella_set_error("tail_scores_req: bad arguments"); return PAELLA_ERR_ARG; }
    TailArgs a = {};
    a.logits_c = logits_c; a.logits_u = logits_u; a.rows = rows; a.L = L; a.offset = offset;
    a.rq.seeds = seeds; a.rq.temperature = temperature; a.rq.cfg_pairs = cfg_pairs; a.rq.rows_per_sample = rows_per_sample;
    RET_REQ(a);
    hipLaunchKernelGGL(tail_scores_kernel<true>, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, a, scores_out);
    LAUNCH_CHECK_RET();
    return PAELLA_OK;
}

// test hook (test_hooks.h): the selection of the truncated-sampling tail alone -- keep_out uint8 [rows, L] = the kept set of every row, rec_out fp32 [rows, 4] =
// (m, log sum exp(z - m), H, threshold) (NaN where the row has none: a NaN / non-finite row, no filter on, an unreachable target).  Scalar form
// (rows_per_sample == 0: cfg pair, temperature and the four filter values by value) or request form (cfg_pairs / temps / seeds / the two filter tables per request,
// as paella_sample_tail_req takes them; the seeds are read but nothing is drawn).
extern "C" int paella_test_tail_filter_keep(const float* logits_c, const float* logits_u, int64_t rows, int L, float cfg, float one_minus_cfg, float temperature,
                                            int top_k, float top_p, float typical_mass, int min_tokens, const float* cfg_pairs, const float* temps,
                                            const uint64_t* seeds, int rows_per_sample, const int* filter_k, const float* filter_mass, unsigned char* keep_out, float* rec_out,
                                            void* stream) {
    if (!logits_c || !keep_out || rows <= 0 || rows > 0x7fffffff || rows_per_sample < 0) { paella_set_error("tail_filter_keep: bad arguments"); return PAELLA_ERR_ARG; }
    TailArgs a = {};
    a.logits_c = logits_c; a.logits_u = logits_u; a.rows = rows; a.L = L; a.cfg = cfg; a.one_minus_cfg = one_minus_cfg; a.temperature = temperature;
    TailFilter f;
    f.keep_out = keep_out; f.rec_out = rec_out;
    if (rows_per_sample > 0) {
        if (!temps || !seeds || !filter_k || !filter_mass) { paella_set_error("tail_filter_keep: the request form needs the temperature, seed and the two filter tables"); return PAELLA_ERR_ARG; }
        a.logits_u = cfg_pairs ? logits_u : nullptr; a.cfg = 1.f; a.one_minus_cfg = 0.f; a.temperature = 1.f;
        a.rq.seeds = seeds; a.rq.temperature = temps; a.rq.cfg_pairs = cfg_pairs; a.rq.rows_per_sample = rows_per_sample;
        f.filter_k = filter_k; f.filter_mass = filter_mass;
    } else {
        if (!(temperature > 0.f)) { paella_set_error("tail_filter_keep: temperature must be > 0"); return PAELLA_ERR_ARG; }
        f.top_k = top_k; f.top_p = top_p; f.typical_mass = typical_mass; f.min_tokens = min_tokens;
    }
    return launch_sample_tail_filter(a, f, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------
// measurement hook: a chain of n dependent, nearly empty kernels on `stream` (launch-boundary floor of this box)
// ---------------------------------------------------------------------------
__global__ void chain_kernel(float* p, int bytes4) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < bytes4) p[i] += 1.0f;
}
extern "C" int paella_test_launch_chain(float* buf, int n_elems, int blocks, int n_launches, void* stream) {
    for (int i = 0; i < n_launches; ++i) hipLaunchKernelGGL(chain_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, buf, n_elems);
    LAUNCH_CHECK_RET();
    return PAELLA_OK;
}

// ---- C entry points of the sampling tails (include/paella_hip.h): the argument block, and the fixed forms over it
static int run_tail_block(const char* who, const paella_tail_args& t, int need, void* stream) {
    TailArgs a; TailFilter f; TailStats s;
    int kind = 0;
    RET_IF(tail_block_convert(who, t, need, false, a, f, s, &kind));
    if (kind == 2) return launch_sample_tail_stats(a, f, s, (hipStream_t)stream);
    if (kind == 1) return launch_sample_tail_filter(a, f, (hipStream_t)stream);
    return launch_sample_tail(a, (hipStream_t)stream);
}

extern "C" int paella_sample_tail_args(const paella_tail_args* args, size_t args_bytes, void* stream) {
    if (args_bytes != sizeof(paella_tail_args)) { paella_set_error("sample_tail_args: args_bytes %zu is not this library's sizeof(paella_tail_args) = %zu", args_bytes, sizeof(paella_tail_args)); return PAELLA_ERR_ARG; }
    if (!args) { paella_set_error("sample_tail_args: null argument"); return PAELLA_ERR_ARG; }
    return run_tail_block("sample_tail_args", *args, 0, stream);
}

// ---- the fixed-form entry points: each fills a block (internal.h: tail_block_scalar / tail_block_stream), names itself and runs it; one that extends another IS that
// one when what it adds is absent, and then reports under the other's name
extern "C" int paella_sample_tail_ex(const float* logits_c, const float* logits_u, int64_t rows, int L, float cfg, float one_minus_cfg,
                                     float temperature, int mode, const float* noise_q, uint64_t seed, const uint64_t* seed_ptr,
                                     uint64_t offset, int64_t row_offset, const int64_t* row_offset_ptr, const int64_t* init_noise, const float* mask_u,
                                     float t_next, int64_t* tokens_out, int64_t* sampled_out, void* stream) {
    paella_tail_args t = tail_block_scalar(logits_c, logits_u, rows, L, cfg, one_minus_cfg, temperature, mode, seed, seed_ptr, offset, row_offset, row_offset_ptr,
                                           init_noise, t_next, nullptr, nullptr, tokens_out, sampled_out);
    t.noise_q = noise_q; t.mask_u = mask_u;
    return run_tail_block("sample_tail_ex", t, 0, stream);
}
extern "C" int paella_sample_tail(const float* logits_c, const float* logits_u, int64_t rows, int L, float cfg, float one_minus_cfg,
                                  float temperature, int mode, const float* noise_q, uint64_t seed, uint64_t offset,
                                  const int64_t* init_noise, const float* mask_u, float t_next, int64_t* tokens_out,
                                  int64_t* sampled_out, void* stream) {
    return paella_sample_tail_ex(logits_c, logits_u, rows, L, cfg, one_minus_cfg, temperature, mode, noise_q, seed, nullptr, offset, 0, nullptr,
                                 init_noise, mask_u, t_next, tokens_out, sampled_out, stream);
}
// paella_sample_tail_ex in the counter-based noise mode with the optional pin: tokens_out[row] = pin_keep[row] == 0 ? pin_tokens[row] : the renoised draw
extern "C" int paella_sample_tail_pin(const float* logits_c, const float* logits_u, int64_t rows, int L, float cfg, float one_minus_cfg, float temperature, int mode,
                                      uint64_t seed, const uint64_t* seed_ptr, uint64_t offset, int64_t row_offset, const int64_t* row_offset_ptr,
                                      const int64_t* init_noise, float t_next, const int64_t* pin_keep, const int64_t* pin_tokens, int64_t* tokens_out,
                                      int64_t* sampled_out, void* stream) {
    return run_tail_block("sample_tail_pin", tail_block_scalar(logits_c, logits_u, rows, L, cfg, one_minus_cfg, temperature, mode, seed, seed_ptr, offset, row_offset,
                                                               row_offset_ptr, init_noise, t_next, pin_keep, pin_tokens, tokens_out, sampled_out), 0, stream);
}
// paella_sample_tail_pin with a truncation filter (common.h: TailFilter; top_k <= 0 or >= L, top_p = 1, typical_mass = 1 are "off"): categorical mode only
extern "C" int paella_sample_tail_filter(const float* logits_c, const float* logits_u, int64_t rows, int L, float cfg, float one_minus_cfg, float temperature, int mode,
                                         uint64_t seed, const uint64_t* seed_ptr, uint64_t offset, int64_t row_offset, const int64_t* row_offset_ptr,
                                         const int64_t* init_noise, float t_next, const int64_t* pin_keep, const int64_t* pin_tokens, int top_k, float top_p,
                                         float typical_mass, int min_tokens, int64_t* tokens_out, int64_t* sampled_out, void* stream) {
    return paella_sample_tail_stats(logits_c, logits_u, rows, L, cfg, one_minus_cfg, temperature, mode, seed, seed_ptr, offset, row_offset, row_offset_ptr, init_noise,
                                    t_next, pin_keep, pin_tokens, top_k, top_p, typical_mass, min_tokens, tokens_out, sampled_out, nullptr, nullptr, stream);
}
// paella_sample_tail_filter plus the two statistics outputs; both NULL = paella_sample_tail_filter, the same launch
extern "C" int paella_sample_tail_stats(const float* logits_c, const float* logits_u, int64_t rows, int L, float cfg, float one_minus_cfg, float temperature, int mode,
                                        uint64_t seed, const uint64_t* seed_ptr, uint64_t offset, int64_t row_offset, const int64_t* row_offset_ptr,
                                        const int64_t* init_noise, float t_next, const int64_t* pin_keep, const int64_t* pin_tokens, int top_k, float top_p,
                                        float typical_mass, int min_tokens, int64_t* tokens_out, int64_t* sampled_out, float* logprob_out, float* entropy_out,
                                        void* stream) {
    paella_tail_args t = tail_block_scalar(logits_c, logits_u, rows, L, cfg, one_minus_cfg, temperature, mode, seed, seed_ptr, offset, row_offset, row_offset_ptr,
                                           init_noise, t_next, pin_keep, pin_tokens, tokens_out, sampled_out);
    t.top_k = top_k; t.top_p = top_p; t.typical_mass = typical_mass; t.min_tokens = min_tokens; t.logprob_out = logprob_out; t.entropy_out = entropy_out;
    return run_tail_block(logprob_out || entropy_out ? "sample_tail_stats" : "sample_tail_filter", t, kNeedFilter, stream);
}

// Request batch (ABI 6) and request stream (ABI 7): the per-sample device tables (common.h: ReqTables)
extern "C" int paella_sample_tail_req(const float* logits_c, const float* logits_u, int64_t rows, int L, const float* cfg_pairs, const float* temperature,
                                      const uint64_t* seeds, int rows_per_sample, uint64_t offset, const int64_t* init_noise, float t_next,
                                      int64_t* tokens_out, int64_t* sampled_out, void* stream) {
    paella_tail_args t = tail_block_stream(logits_c, logits_u, rows, L, cfg_pairs, temperature, seeds, rows_per_sample, nullptr, nullptr, nullptr, init_noise, nullptr,
                                           nullptr, nullptr, tokens_out, sampled_out);
    t.offset = offset; t.t_next = t_next;
    return run_tail_block("sample_tail_req", t, kNeedRequest, stream);
}
// paella_sample_tail_stream_filter (the per-request filter tables, common.h: TailFilter) plus the two statistics outputs, the most general member of the family.
// Both outputs NULL = that entry point; both filter tables NULL as well = paella_sample_tail_stream(_pin), whose name then answers
extern "C" int paella_sample_tail_stream_stats(const float* logits_c, const float* logits_u, int64_t rows, int L, const float* cfg_pairs, const float* temperature,
                                               const uint64_t* seeds, int rows_per_sample, const int* step, const float* t_next, const int* active,
                                               const int64_t* init_noise, const int64_t* pin_keep, const int64_t* pin_tokens, const int* pin_on,
                                               const int* filter_k, const float* filter_mass, int64_t* tokens_out, int64_t* sampled_out, float* logprob_out,
                                               float* entropy_out, void* stream) {
    paella_tail_args t = tail_block_stream(logits_c, logits_u, rows, L, cfg_pairs, temperature, seeds, rows_per_sample, step, t_next, active, init_noise, pin_keep,
                                           pin_tokens, pin_on, tokens_out, sampled_out);
    t.filter_k = filter_k; t.filter_mass = filter_mass; t.logprob_out = logprob_out; t.entropy_out = entropy_out;
    const char* who = logprob_out || entropy_out ? "sample_tail_stream_stats" : filter_k || filter_mass ? "sample_tail_stream_filter" : "sample_tail_stream";
    return run_tail_block(who, t, kNeedStream, stream);
}
extern "C" int paella_sample_tail_stream_filter(const float* logits_c, const float* logits_u, int64_t rows, int L, const float* cfg_pairs, const float* temperature,
                                                const uint64_t* seeds, int rows_per_sample, const int* step, const float* t_next, const int* active,
                                                const int64_t* init_noise, const int64_t* pin_keep, const int64_t* pin_tokens, const int* pin_on,
                                                const int* filter_k, const float* filter_mass, int64_t* tokens_out, int64_t* sampled_out, void* stream) {
    return paella_sample_tail_stream_stats(logits_c, logits_u, rows, L, cfg_pairs, temperature, seeds, rows_per_sample, step, t_next, active, init_noise, pin_keep,
                                           pin_tokens, pin_on, filter_k, filter_mass, tokens_out, sampled_out, nullptr, nullptr, stream);
}
extern "C" int paella_sample_tail_stream_pin(const float* logits_c, const float* logits_u, int64_t rows, int L, const float* cfg_pairs, const float* temperature,
                                             const uint64_t* seeds, int rows_per_sample, const int* step, const float* t_next, const int* active,
                                             const int64_t* init_noise, const int64_t* pin_keep, const int64_t* pin_tokens, const int* pin_on,
                                             int64_t* tokens_out, int64_t* sampled_out, void* stream) {
    return paella_sample_tail_stream_stats(logits_c, logits_u, rows, L, cfg_pairs, temperature, seeds, rows_per_sample, step, t_next, active, init_noise, pin_keep,
                                           pin_tokens, pin_on, nullptr, nullptr, tokens_out, sampled_out, nullptr, nullptr, stream);
}
extern "C" int paella_sample_tail_stream(const float* logits_c, const float* logits_u, int64_t rows, int L, const float* cfg_pairs, const float* temperature,
                                         const uint64_t* seeds, int rows_per_sample, const int* step, const float* t_next, const int* active,
                                         const int64_t* init_noise, int64_t* tokens_out, int64_t* sampled_out, void* stream) {
    return paella_sample_tail_stream_pin(logits_c, logits_u, rows, L, cfg_pairs, temperature, seeds, rows_per_sample, step, t_next, active, init_noise, nullptr, nullptr,
                                         nullptr, tokens_out, sampled_out, stream);
}
