// Training optimizer step: the global gradient norm, clip_grad_norm_'s coefficient and the AdamW update of every parameter tensor as THREE launches over a
// device-readable table of tensors (include/paella_hip.h "Training optimizer step").  fp32 tensors; the sums and the per-tensor scalars in fp64.
//
//   (1) adamw_sumsq_kernel    per chunk of kChunk consecutive elements of ONE tensor: sum of g^2, each element widened to fp64 before it is squared; a lane adds
//                             its elements in ascending order, then the wave by an xor butterfly, then the four waves through LDS in wave order -> part[chunk]
//   (2) adamw_finalize_kernel ONE workgroup: lane t adds part[t], part[t + kFinThreads], ... ascending, then a fixed tree over the lanes; norm, finite, coef; with
//                             `steps`: step += 1 and the two bias corrections of every tensor that has a gradient, in fp64
//   (3) adamw_update_kernel   per chunk: g' = g coef (the one product formed in fp64), decay, m, v, p -- reads p, g, m, v once and writes p, m, v once; returns at
//                             once when the norm is not finite
//
// A chunk finds its tensor by binary search over chunk_begin (the address is workgroup-uniform: scalar loads); there is no per-chunk list.  (1) and (3) are
// grid-stride loops over the chunks under a capped grid: a chunk's values depend on the chunk alone, part[] is indexed by the chunk, so neither the grid nor the
// scheduling reaches a bit.  No atomics.  Every chunk writes its partial (0 for a tensor without a gradient): the workspace needs no initialisation.
// Whatever the table says, an element outside [0, n) of a row is neither read nor written: a chunk whose offset falls outside is skipped.
#include "train_common.h"

namespace {

using namespace train;

constexpr int kThreads = 256;
constexpr int kChunk = PAELLA_ADAMW_CHUNK;
constexpr int kVecs = kChunk / (kThreads * 4);  // 16-byte vectors per thread and full chunk: all of them in flight at once
constexpr int kMaxGrid = 2048;                  // ~8 workgroups per CU; the chunks beyond are grid-strided
constexpr int kFinThreads = 1024;
static_assert(kChunk % 1024 == 0 && kVecs >= 1, "a chunk is a whole number of 16-byte vectors per thread");

struct Header {
    double coef;  // applied in fp64: g' = (float)((double)g coef) is ONE rounding, and no rounding of coef itself -- a relative error every element would share
    int finite;
};

struct Layout {
    size_t scal_off, part_off, bytes;  // the header at 0
};

Layout make_layout(int n_tensors, int64_t n_chunks) {
    Layout l;
    l.scal_off = 256;
    l.part_off = l.scal_off + align256((size_t)n_tensors * 2 * sizeof(double));
    l.bytes = l.part_off + align256((size_t)n_chunks * sizeof(double));
    return l;
}

__device__ __forceinline__ f32x4 ldq(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void stq(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ bool dev_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the last row whose chunk_begin is <= c (rows without chunks share the chunk_begin of the row behind them and are never the last)
__device__ __forceinline__ int find_row(const paella_adamw_tensor* __restrict__ rows, int n_tensors, int64_t c) {
    int lo = 0, hi = n_tensors;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (rows[mid].chunk_begin <= c) lo = mid;
        else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ double sq(float x) {
    const double d = (double)x;
    return d * d;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(kThreads) void adamw_sumsq_kernel(const paella_adamw_tensor* __restrict__ rows, int n_tensors, int64_t n_chunks,
                                                               double* __restrict__ part) {
    __shared__ double red[kThreads / 64];
    const int tid = threadIdx.x;
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int r = find_row(rows, n_tensors, c);
        const float* g = rows[r].g;
        const int64_t n = rows[r].n, off = (c - rows[r].chunk_begin) * kChunk;
        double s = 0.0;
        if (g && off >= 0 && off < n) {  // uniform
            const int len = (int)(n - off < kChunk ? n - off : kChunk);
            const float* gp = g + off;
            if (dev_aligned16(g)) {  // off is a multiple of the chunk: the chunk is aligned as its tensor is
                const int nv = len >> 2;
                if (len == kChunk) {
                    f32x4 x[kVecs];
#pragma unroll
                    for (int k = 0; k < kVecs; ++k) x[k] = ldq(gp + 4 * (tid + k * kThreads));
#pragma unroll
                    for (int k = 0; k < kVecs; ++k) s += sq(x[k][0]) + sq(x[k][1]) + sq(x[k][2]) + sq(x[k][3]);
                } else {
                    for (int i = tid; i < nv; i += kThreads) {
                        const f32x4 x = ldq(gp + 4 * i);
                        s += sq(x[0]) + sq(x[1]) + sq(x[2]) + sq(x[3]);
                    }
                    if (nv * 4 + tid < len) s += sq(gp[nv * 4 + tid]);  // at most three elements
                }
            } else {
                for (int i = tid; i < len; i += kThreads) s += sq(gp[i]);
            }
        }
        s = wave_sum(s);
        if ((tid & 63) == 0) red[tid >> 6] = s;
        __syncthreads();
        if (tid == 0) part[c] = ((red[0] + red[1]) + red[2]) + red[3];
        __syncthreads();  // red is written again in the next round
    }
}

// `steps` NULL: the norm alone (paella_adamw_grad_norm)
__global__ __launch_bounds__(kFinThreads) void adamw_finalize_kernel(const paella_adamw_tensor* __restrict__ rows, int n_tensors, int64_t n_chunks,
                                                                     const double* __restrict__ part, float max_norm, float* __restrict__ steps,
                                                                     float* __restrict__ norm_out, Header* __restrict__ hdr, double* __restrict__ scal) {
    __shared__ double red[kFinThreads];
    const int tid = threadIdx.x;
    double s = 0.0;
#pragma unroll 8  // eight loads in flight; the additions keep their order
    for (int64_t c = tid; c < n_chunks; c += kFinThreads) s += part[c];
    red[tid] = s;
    __syncthreads();
    for (int o = kFinThreads / 2; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
    double total = red[0];
    // the plan, where the host could not read it: chunk_begin ascends from 0 within n_chunks and no n is negative
    int bad = 0;
    for (int t = tid; t < n_tensors; t += kFinThreads) {
        const int64_t b = rows[t].chunk_begin, e = t + 1 < n_tensors ? rows[t + 1].chunk_begin : n_chunks;
        bad |= (t == 0 && b != 0) || e < b || rows[t].n < 0;
    }
    if (__syncthreads_or(bad)) total = __builtin_nan("");
    const bool finite = isfinite(total);
    if (tid == 0) {
        const double norm = sqrt(total);
        norm_out[0] = (float)norm;
        hdr->finite = finite ? 1 : 0;
        const double k = max_norm > 0.f ? (double)max_norm / (norm + 1e-6) : 1.0;
        hdr->coef = k < 1.0 ? k : 1.0;
    }
    if (!steps || !finite) return;
    for (int t = tid; t < n_tensors; t += kFinThreads) {
        if (!rows[t].g) continue;
        const float st = steps[t] + 1.0f;
        steps[t] = st;
        scal[2 * t] = rows[t].lr / (1.0 - pow(rows[t].beta1, (double)st));
        scal[2 * t + 1] = 1.0 / sqrt(1.0 - pow(rows[t].beta2, (double)st));
    }
}

struct Hyper {
    double coef;
    float decay, omb1, b2, omb2, step_size, rs, eps;
};

// torch's single-tensor AdamW: mul_(1 - lr wd); lerp_(g, 1 - beta1); mul_(beta2).addcmul_(g, g, 1 - beta2); addcdiv_(m, sqrt(v) / sqrt(bc2) + eps, -step_size)
__device__ __forceinline__ void adamw_element(float& p, float g, float& m, float& v, const Hyper& h) {
    g = (float)((double)g * h.coef);  // coef == 1: g itself
    p *= h.decay;
    m += (g - m) * h.omb1;
    v = v * h.b2 + h.omb2 * g * g;
    p -= h.step_size * m / (sqrtf(v) * h.rs + h.eps);
}

__device__ __forceinline__ void adamw_vector(f32x4& p, const f32x4& g, f32x4& m, f32x4& v, const Hyper& h) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float pj = p[j], mj = m[j], vj = v[j];
        adamw_element(pj, g[j], mj, vj, h);
        p[j] = pj;
        m[j] = mj;
        v[j] = vj;
    }
}

__global__ __launch_bounds__(kThreads) void adamw_update_kernel(const paella_adamw_tensor* __restrict__ rows, int n_tensors, int64_t n_chunks,
                                                                const Header* __restrict__ hdr, const double* __restrict__ scal) {
    if (!hdr->finite) return;
    const int tid = threadIdx.x;
    const double coef = hdr->coef;
    for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const int r = find_row(rows, n_tensors, c);
        const paella_adamw_tensor row = rows[r];
        const int64_t off = (c - row.chunk_begin) * kChunk;
        if (!row.g || off < 0 || off >= row.n) continue;  // uniform
        const int len = (int)(row.n - off < kChunk ? row.n - off : kChunk);
        Hyper h;
        h.coef = coef;
        h.decay = (float)(1.0 - row.lr * row.weight_decay);
        h.omb1 = (float)(1.0 - row.beta1);
        h.b2 = (float)row.beta2;
        h.omb2 = (float)(1.0 - row.beta2);
        h.step_size = (float)scal[2 * r];
        h.rs = (float)scal[2 * r + 1];
        h.eps = (float)row.eps;
        float* __restrict__ pp = row.p + off;
        const float* __restrict__ gp = row.g + off;
        float* __restrict__ mp = row.m + off;
        float* __restrict__ vp = row.v + off;
        if (dev_aligned16(row.p) && dev_aligned16(row.g) && dev_aligned16(row.m) && dev_aligned16(row.v)) {
            if (len == kChunk) {
                f32x4 p[kVecs], g[kVecs], m[kVecs], v[kVecs];
#pragma unroll
                for (int k = 0; k < kVecs; ++k) {
                    const int i = 4 * (tid + k * kThreads);
                    p[k] = ldq(pp + i);
                    g[k] = ldq(gp + i);
                    m[k] = ldq(mp + i);
                    v[k] = ldq(vp + i);
                }
#pragma unroll
                for (int k = 0; k < kVecs; ++k) {
                    const int i = 4 * (tid + k * kThreads);
                    adamw_vector(p[k], g[k], m[k], v[k], h);
                    stq(pp + i, p[k]);
                    stq(mp + i, m[k]);
                    stq(vp + i, v[k]);
                }
            } else {
                const int nv = len >> 2;
                for (int i = tid; i < nv; i += kThreads) {
                    f32x4 p = ldq(pp + 4 * i), m = ldq(mp + 4 * i), v = ldq(vp + 4 * i);
                    adamw_vector(p, ldq(gp + 4 * i), m, v, h);
                    stq(pp + 4 * i, p);
                    stq(mp + 4 * i, m);
                    stq(vp + 4 * i, v);
                }
                const int i = nv * 4 + tid;  // at most three elements
                if (i < len) adamw_element(pp[i], gp[i], mp[i], vp[i], h);
            }
        } else {
            for (int i = tid; i < len; i += kThreads) adamw_element(pp[i], gp[i], mp[i], vp[i], h);
        }
    }
}

// A table in pinned host memory is read here, before anything is enqueued; one in device memory is checked by the finalize launch
int check_plan(const char* who, const paella_adamw_tensor* rows, int n_tensors, int64_t n_chunks) {
    if (n_tensors == 0) return PAELLA_OK;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, rows) != hipSuccess) {
        (void)hipGetLastError();  // not a pointer the runtime knows: nothing to read here
        return PAELLA_OK;
    }
    if (at.type != hipMemoryTypeHost || !at.hostPointer) return PAELLA_OK;
    const paella_adamw_tensor* h = (const paella_adamw_tensor*)at.hostPointer;
    for (int t = 0; t < n_tensors; ++t) {
        const int64_t b = h[t].chunk_begin, e = t + 1 < n_tensors ? h[t + 1].chunk_begin : n_chunks;
        if ((t == 0 && b != 0) || e < b) {
            paella_set_error("%s: chunk_begin must ascend from 0 within n_chunks = %lld (row %d: %lld, then %lld)", who, (long long)n_chunks, t, (long long)b, (long long)e);
            return PAELLA_ERR_ARG;
        }
        if (h[t].n < 0) {
            paella_set_error("%s: row %d has n = %lld", who, t, (long long)h[t].n);
            return PAELLA_ERR_ARG;
        }
    }
    return PAELLA_OK;
}

int run(const char* who, const paella_adamw_tensor* rows, int n_tensors, int64_t n_chunks, float max_norm, float* steps, bool update, float* norm_out, void* ws,
        size_t ws_bytes, void* stream) {
    if (n_tensors < 0 || n_chunks < 0 || (n_tensors == 0 && n_chunks != 0)) {
        paella_set_error("%s: n_tensors = %d, n_chunks = %lld (both >= 0, and no chunk without a tensor)", who, n_tensors, (long long)n_chunks);
        return PAELLA_ERR_ARG;
    }
    int rc = update ? check_required(who, (rows || !n_tensors) && steps && norm_out, "rows, steps and norm_out")
                    : check_required(who, (rows || !n_tensors) && norm_out, "rows and norm_out");
    if (rc != PAELLA_OK) return rc;
    if (max_norm != max_norm) {
        paella_set_error("%s: max_norm is NaN", who);
        return PAELLA_ERR_ARG;
    }
    const Layout l = make_layout(n_tensors, n_chunks);
    rc = check_workspace(who, ws, ws_bytes, l.bytes, "paella_adamw_workspace_bytes asks for");
    if (rc == PAELLA_OK) rc = check_plan(who, rows, n_tensors, n_chunks);
    if (rc != PAELLA_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    Header* hdr = (Header*)ws;
    double* scal = (double*)((char*)ws + l.scal_off);
    double* part = (double*)((char*)ws + l.part_off);
    const unsigned grid = (unsigned)(n_chunks < kMaxGrid ? n_chunks : kMaxGrid);
    if (grid) {
        hipLaunchKernelGGL(adamw_sumsq_kernel, dim3(grid), dim3(kThreads), 0, st, rows, n_tensors, n_chunks, part);
        LAUNCH_CHECK_RET();
    }
    hipLaunchKernelGGL(adamw_finalize_kernel, dim3(1), dim3(kFinThreads), 0, st, rows, n_tensors, n_chunks, (const double*)part, max_norm, update ? steps : nullptr,
                       norm_out, hdr, scal);
    LAUNCH_CHECK_RET();
    if (update && grid) {
        hipLaunchKernelGGL(adamw_update_kernel, dim3(grid), dim3(kThreads), 0, st, rows, n_tensors, n_chunks, (const Header*)hdr, (const double*)scal);
        LAUNCH_CHECK_RET();
    }
    return PAELLA_OK;
}

}  // namespace

extern "C" int paella_adamw_chunk_elems(void) { return kChunk; }

extern "C" size_t paella_adamw_workspace_bytes(int n_tensors, int64_t n_chunks) {
    if (n_tensors < 0 || n_chunks < 0) return 0;
    return make_layout(n_tensors, n_chunks).bytes;
}

extern "C" int paella_adamw_grad_norm(const paella_adamw_tensor* rows, int n_tensors, int64_t n_chunks, float* norm_out, void* ws, size_t ws_bytes, void* stream) {
    return run("adamw_grad_norm", rows, n_tensors, n_chunks, 0.f, nullptr, false, norm_out, ws, ws_bytes, stream);
}

extern "C" int paella_adamw_step(const paella_adamw_tensor* rows, int n_tensors, int64_t n_chunks, float max_norm, float* steps, float* norm_out, void* ws,
                                 size_t ws_bytes, void* stream) {
    return run("adamw_step", rows, n_tensors, n_chunks, max_norm, steps, true, norm_out, ws, ws_bytes, stream);
}
