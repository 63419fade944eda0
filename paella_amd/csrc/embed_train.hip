// Training token stem: token embedding -> LayerNorm(c_in, no affine) -> PixelUnshuffle(patch) -> NHWC rows, the top of the train-mode network, as ONE op in both
// directions.  tokens int64 [B, H, W]; table fp32 [num_labels, c_in] (in_mapper.0.weight as it is); rows fp32 [B, H/p, W/p, c_in p^2] with
// rows[b, oy, ox, c p^2 + dy p + dx] = LN(table[clamp(tokens[b, oy p + dy, ox p + dx])])[c] -- the A operand of the 1x1 convolution as a linear.
//
//   forward : the eval engine's launch itself (elementwise.hip: launch_embed_ln_unshuffle), so the train rows are the engine's bits; nothing is kept
//   backward: dtable[l] = LNbwd(table[l], G[l]),  G[l] = sum over the positions n with clamp(tokens[n]) = l of the de-interleaved row of d_rows at n.  The
//             LayerNorm backward is linear in the arriving gradient for a fixed row, so the gathered gradients are summed per LABEL first and the LayerNorm
//             backward runs once per label: there is no [N, c_in] intermediate and the statistics are recomputed from the table row, as the forward forms them.
//
// Launch.  ONE, no workspace.  A workgroup owns a block of `labels_per_block(c_in)` consecutive labels with their sums in LDS, carried in fp64.  It scans ALL N tokens
// in ascending order, kTokenBlock at a time (the token array is 128-512 KiB and stays in L2): kRounds ballots per wave mark the tokens of its labels, the marks are
// compacted IN ASCENDING POSITION ORDER into an LDS list (row offset, local label), and thread c adds channel c of every listed row to its label's sum in list
// order -- a run of one label stays in a register, which changes no addition.  Then one wave per owned label: a label that never occurred is written as exact
// zeros (whatever its table row holds), the others get rstd ((G - mean G) - xhat mean(G xhat)), statistics and all in fp64, rounded once at the store.
// No atomics of any kind: the bits of dtable are a function of (tokens, table, d_rows, shape) alone -- every sum is one thread's, in ascending position order.
// The grid is ceil(num_labels / labels per block): it depends on the shape only.  KNOWN WEAK SPOT: the additions of one label are one workgroup's, serially; when
// most tokens share a label that workgroup does most of the op's N row additions (the time stays bounded by N row adds, the result is the same sum).
#include "train_common.h"
#include "test_hooks.h"

namespace {

using namespace train;

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kRounds = 4;                          // ballots per scan step
constexpr int kTokenBlock = kRounds * kThreads;     // tokens per scan step
constexpr int kAccDoubles = 4096;                   // 32 KiB of label sums per workgroup
constexpr int kMaxLabelsPerBlock = 256;
constexpr int kMaxC = 1024, kMaxLabels = 65536;
constexpr int kInFlight = 8;                        // gathered loads a thread keeps in flight

// c_in <= 1024 gives at least 4 labels; c_in = 256 (the shipped width) 16
int labels_per_block(int c_in) { return kAccDoubles / c_in < kMaxLabelsPerBlock ? kAccDoubles / c_in : kMaxLabelsPerBlock; }

bool shape_ok(int B, int H, int W, int c_in, int patch, int num_labels) {
    if (patch < 1 || patch > 2 || B < 1 || H < 1 || W < 1 || (H % patch) || (W % patch)) return false;
    if ((int64_t)B * (H / patch) * (W / patch) > 0x7fffffffll) return false;
    return c_in >= 4 && !(c_in & 3) && c_in <= kMaxC && num_labels >= 1 && num_labels <= kMaxLabels;
}

__device__ __forceinline__ f32x4 ldq(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void stq(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// P = patch.  N = B H W tokens; the element offset of token n's gradient row in d_rows is off(n) + c P^2 for channel c
template <int P>
__global__ __launch_bounds__(kThreads) void embed_ln_train_bwd_kernel(const int64_t* __restrict__ tokens, const float* __restrict__ table,
                                                                      const float* __restrict__ d_rows, float* __restrict__ dtable, int64_t N, int H, int W, int c_in,
                                                                      int num_labels, int lpb, float eps) {
    __shared__ double acc[kAccDoubles];         // [lpb][c_in]
    __shared__ long long m_off[kTokenBlock];    // the matches of one scan step, ascending position
    __shared__ int m_lab[kTokenBlock];
    __shared__ int wcount[kRounds * kWaves];
    __shared__ int seen[kMaxLabelsPerBlock];
    constexpr int PP = P * P;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l0 = blockIdx.x * lpb;
    for (int i = tid; i < lpb * c_in; i += kThreads) acc[i] = 0.0;
    for (int i = tid; i < lpb; i += kThreads) seen[i] = 0;
    __syncthreads();

    for (int64_t t0 = 0; t0 < N; t0 += kTokenBlock) {
        int lab[kRounds];
        unsigned long long bal[kRounds];
#pragma unroll
        for (int j = 0; j < kRounds; ++j) {
            const int64_t n = t0 + j * kThreads + tid;
            int local = -1;
            if (n < N) {
                int64_t tok = tokens[n];
                tok = tok < 0 ? 0 : (tok >= num_labels ? num_labels - 1 : tok);  // the forward's clamp
                const int d = (int)tok - l0;
                local = (unsigned)d < (unsigned)lpb ? d : -1;
            }
            lab[j] = local;
            bal[j] = __ballot(local >= 0);
            if (lane == 0) wcount[j * kWaves + wave] = __popcll(bal[j]);
        }
        __syncthreads();
        int total = 0, base[kRounds] = {};  // base[j]: the matches in front of this wave's in round j
#pragma unroll
        for (int i = 0; i < kRounds * kWaves; ++i) {
            if ((i & (kWaves - 1)) == wave) base[i / kWaves] = total;
            total += wcount[i];
        }
#pragma unroll
        for (int j = 0; j < kRounds; ++j) {
            if (lab[j] < 0) continue;
            const int64_t n = t0 + j * kThreads + tid;
            int64_t off;
            if (P == 1) {
                off = n * c_in;
            } else {
                const int64_t r = n / W, b = r / H;  // (b H + y), b
                const int x = (int)(n - r * W), y = (int)(r - b * H);
                const int64_t opos = (b * (H / P) + y / P) * (W / P) + x / P;
                off = opos * ((int64_t)c_in * PP) + (y % P) * P + (x % P);
            }
            const int idx = base[j] + __popcll(bal[j] & ((1ull << lane) - 1ull));  // < kTokenBlock: one entry per token of the step at most
            m_off[idx] = off;
            m_lab[idx] = lab[j];
            seen[lab[j]] = 1;
        }
        __syncthreads();
        // (no barrier at the end of the step: a wave that runs ahead rewrites wcount, which every wave has read before the barrier above, and reaches m_off /
        // m_lab only behind the next step's first barrier; acc[.][c] is thread c's alone)
        if (total == 0) continue;
        for (int c = tid; c < c_in; c += kThreads) {
            const float* g = d_rows + c * PP;
            int cur = -1;
            double a = 0.0;
            int m = 0;
            for (; m + kInFlight <= total; m += kInFlight) {
                float v[kInFlight];
#pragma unroll
                for (int u = 0; u < kInFlight; ++u) v[u] = g[m_off[m + u]];
#pragma unroll
                for (int u = 0; u < kInFlight; ++u) {
                    const int l = m_lab[m + u];
                    if (l != cur) {
                        if (cur >= 0) acc[cur * c_in + c] = a;
                        cur = l;
                        a = acc[l * c_in + c];
                    }
                    a += (double)v[u];
                }
            }
            for (; m < total; ++m) {
                const int l = m_lab[m];
                if (l != cur) {
                    if (cur >= 0) acc[cur * c_in + c] = a;
                    cur = l;
                    a = acc[l * c_in + c];
                }
                a += (double)g[m_off[m]];
            }
            acc[cur * c_in + c] = a;  // total > 0: cur is a label
        }
    }
    __syncthreads();

    // the LayerNorm backward, one wave per owned label; the statistics two-pass over the table row, as the forward forms them
    const int nl = min(lpb, num_labels - l0);
    const int C4 = c_in >> 2;
    for (int i = wave; i < nl; i += kWaves) {
        float* out = dtable + (int64_t)(l0 + i) * c_in;
        if (!seen[i]) {
            for (int c4 = lane; c4 < C4; c4 += 64) stq(out + c4 * 4, f32x4{0.f, 0.f, 0.f, 0.f});
            continue;
        }
        // in fp64 throughout and rounded once at the store: a label is visited once, so the width costs nothing next to the scan
        const float* row = table + (int64_t)(l0 + i) * c_in;
        const double* gs = acc + i * c_in;
        double s = 0.0;
        for (int c4 = lane; c4 < C4; c4 += 64) {
            const f32x4 v = ldq(row + c4 * 4);
            s += ((double)v[0] + (double)v[1]) + ((double)v[2] + (double)v[3]);
        }
        const double mean = wave_sum(s) / (double)c_in;
        double q = 0.0;
        for (int c4 = lane; c4 < C4; c4 += 64) {
            const f32x4 v = ldq(row + c4 * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) q += ((double)v[e] - mean) * ((double)v[e] - mean);
        }
        const double rstd = 1.0 / sqrt(wave_sum(q) / (double)c_in + (double)eps);
        double s1 = 0.0, s2 = 0.0;
        for (int c4 = lane; c4 < C4; c4 += 64) {
            const f32x4 v = ldq(row + c4 * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double gv = gs[c4 * 4 + e];
                s1 += gv;
                s2 += gv * (((double)v[e] - mean) * rstd);
            }
        }
        const double c1 = wave_sum(s1) / (double)c_in, c2 = wave_sum(s2) / (double)c_in;
        for (int c4 = lane; c4 < C4; c4 += 64) {
            const f32x4 v = ldq(row + c4 * 4);
            f32x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (float)(((gs[c4 * 4 + e] - c1) - (((double)v[e] - mean) * rstd) * c2) * rstd);
            stq(out + c4 * 4, o);
        }
    }
}

int check_call(const char* who, int B, int H, int W, int c_in, int patch, int num_labels, float eps) {
    if (!shape_ok(B, H, W, c_in, patch, num_labels)) {
        paella_set_error("%s: unsupported shape B=%d H=%d W=%d c_in=%d patch=%d num_labels=%d (patch 1 or 2 dividing H and W, B (H / patch) (W / patch) <= 2^31 - 1; "
                         "c_in a multiple of 4 in 4...1024; num_labels in 1...65536)", who, B, H, W, c_in, patch, num_labels);
        return PAELLA_ERR_ARG;
    }
    if (!(eps > 0.f) || !(eps < 1e30f)) {  // false for NaN as well
        paella_set_error("%s: eps must be positive and finite (got %g)", who, (double)eps);
        return PAELLA_ERR_ARG;
    }
    return PAELLA_OK;
}

}  // namespace

// the op keeps nothing in its workspace today; a supported shape is sized 256 so that 0 keeps saying "unsupported" and the entry points check what they are given
extern "C" size_t paella_embed_ln_train_workspace_bytes(int B, int H, int W, int c_in, int patch, int num_labels) {
    return shape_ok(B, H, W, c_in, patch, num_labels) ? 256 : 0;
}

extern "C" int paella_embed_ln_train_forward(const int64_t* tokens, const float* table, int B, int H, int W, int c_in, int patch, int num_labels, float eps,
                                             float* rows_out, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "embed_ln_train_forward";
    int rc = check_call(who, B, H, W, c_in, patch, num_labels, eps);
    if (rc == PAELLA_OK) rc = check_required(who, tokens && table && rows_out, "tokens, table and rows_out");
    if (rc == PAELLA_OK) rc = check_tensors_aligned16(who, tokens, table, rows_out);
    if (rc == PAELLA_OK) rc = check_workspace(who, ws, ws_bytes, 256, "paella_embed_ln_train_workspace_bytes asks for");
    if (rc != PAELLA_OK) return rc;
    return launch_embed_ln_unshuffle(tokens, table, rows_out, B, H, W, c_in, patch, num_labels, eps, (hipStream_t)stream);
}

// test hook (test_hooks.h): the engine's stem launch with nothing around it
extern "C" int paella_test_embed_ln_unshuffle(const int64_t* tokens, const float* table, float* out, int B, int H, int W, int c_in, int patch, int num_labels, float eps,
                                              void* stream) {
    if (!tokens || !table || !out || B < 1 || H < 1 || W < 1 || num_labels < 1 || !all_aligned16(tokens, table, out)) {
        paella_set_error("test_embed_ln_unshuffle: tokens, table and out are required, 16-byte aligned, with positive sizes");
        return PAELLA_ERR_ARG;
    }
    return launch_embed_ln_unshuffle(tokens, table, out, B, H, W, c_in, patch, num_labels, eps, (hipStream_t)stream);
}

extern "C" int paella_embed_ln_train_backward(const int64_t* tokens, const float* table, const float* d_rows, int B, int H, int W, int c_in, int patch, int num_labels,
                                              float eps, float* dtable_out, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "embed_ln_train_backward";
    int rc = check_call(who, B, H, W, c_in, patch, num_labels, eps);
    if (rc == PAELLA_OK) rc = check_required(who, tokens && table && d_rows && dtable_out, "tokens, table, d_rows and dtable_out");
    if (rc == PAELLA_OK) rc = check_tensors_aligned16(who, tokens, table, d_rows, dtable_out);
    if (rc == PAELLA_OK) rc = check_workspace(who, ws, ws_bytes, 256, "paella_embed_ln_train_workspace_bytes asks for");
    if (rc != PAELLA_OK) return rc;
    const int lpb = labels_per_block(c_in);
    const int64_t N = (int64_t)B * H * W;
    const dim3 grid((unsigned)((num_labels + lpb - 1) / lpb)), block(kThreads);
    hipStream_t st = (hipStream_t)stream;
    if (patch == 2) hipLaunchKernelGGL((embed_ln_train_bwd_kernel<2>), grid, block, 0, st, tokens, table, d_rows, dtable_out, N, H, W, c_in, num_labels, lpb, eps);
    else hipLaunchKernelGGL((embed_ln_train_bwd_kernel<1>), grid, block, 0, st, tokens, table, d_rows, dtable_out, N, H, W, c_in, num_labels, lpb, eps);
    LAUNCH_CHECK_RET();
    return PAELLA_OK;
}
