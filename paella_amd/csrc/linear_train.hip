// Training linear on the bf16 matrix cores: y = x W^T + b with x [M, K], W [N, K], dy [M, N] -- forward, dgrad and wgrad as NT products of bf16 operands with fp32
// accumulation (the OPT-IN training GEMM precision, outside the fp32 parity contract; Paella.set_training_gemm("bf16")).  Every tensor the caller sees stays fp32:
// only the operands of the three GEMMs are rounded, here, into the workspace.
//
//   forward : y  [M, N] = x16  [M, K] . w16  [N, K]^T + bias        reduction K
//   dgrad   : dx [M, K] = dy16 [M, N] . w16T [K, N]^T               reduction N
//   wgrad   : dW [N, K] = dy16T[N, M] . x16T [K, M]^T               reduction M
//   db      : column sums of the UNROUNDED dy
//
// All three are NT products once each operand exists as bf16 with its reduction axis contiguous, so they run on gemm.hip's bf16 kernels through launch_gemm
// (GemmArgs::A16 / W16, the bias in the epilogue).  The device code of this file is the PACK family that makes those operands: one pass over an fp32 [rows, cols]
// tensor that reads it exactly once and writes any subset of (row-major bf16, transposed bf16, fp32 column sums), compile-time flags, absent outputs compiled out.
//
// The pack.  A workgroup of 256 threads walks the 64 x 64 tiles of one column tile down a STRIP of row tiles.  Thread (q, c4) -- q = 0..15 a quad of rows, c4 = 0..15
// a 16-byte column vector -- loads rows 4q..4q+3 at columns 4c4..4c4+3 (four 16-byte loads; the 16 lanes of a quarter wave are 8 column vectors x 2 row quads, so every
// row segment a load instruction touches is a whole 128-byte line).  Rounding is __builtin_convertvector to __bf16 (round to nearest even, as elementwise.hip), the
// bits of torch's .bfloat16().
//   row-major  : four 8-byte stores per thread, 64 contiguous bytes per 8 lanes.
//   transposed : for each of its four columns a thread rounds the COLUMN of four rows into one 8-byte word (no register shuffles: the conversion packs two arbitrary
//                registers) and writes it to the LDS tile T[c][q]; then every lane reads 16 bytes = rows 8m..8m+7 of one column c and stores them along the source's
//                row axis, 8 lanes a whole 128-byte line of the transposed tensor.
//   LDS layout : T is [64 columns][16 words of 8 bytes], 128 bytes per column, NO padding; word q of column c sits at word index q ^ (2 ((c >> 2) & 7)) of its row.
//                Write (ds_write_b64: 16 contiguous lanes per LDS cycle group, bank = dword address mod 32): a group is q bit 0 x c4 bits 0..2 at a fixed column offset k,
//                its word indices mod 16 are (q & 1) | ((q >> 1 ^ c4 & 7) << 1): 16 distinct words = 32 distinct banks.  Read (ds_read_b128: groups {0-3, 12-15, 20-27}, ...,
//                bank = dword address mod 64): lane u reads column 8 wave + (u >> 3) (+ 32 in the second pass), 16-byte slot (u & 7) ^ ((c >> 2) & 7); the four columns of
//                a group share c >> 2, even columns cover the slots {0-3} ^ h and {4-7} ^ h of the lower 128 bytes of the bank row, odd ones those of the upper: 16 distinct
//                slots = 64 distinct banks.  Two tiles of LDS (16 KiB) alternate, so a tile costs ONE barrier.
//   column sums: a thread carries the sums of its four columns in fp64 over its rows of every tile of the strip (rows ascending), the 16 row quads of a column are
//                added in ascending q through LDS, and the strip's sum is ONE partial per (strip, column) -- fp64 in the workspace, or the fp32 result itself when the
//                tensor is one strip.  A finalize launch adds the partials in ASCENDING strip order and rounds once.  No float atomics: the strips are a function of
//                the row count alone (train::plan_strips over row tiles), hence so are the bits.
// Without column sums a strip is one tile (the most workgroups); with them at least kSumMinTiles tiles.
//
// Split-K.  launch_gemm wants a region whose ticket header is zero and leaves it zero; a training op's workspace is fresh plain bytes, so each entry point zeroes the
// kGemmTicketBytes header of its region on the stream before its first GEMM and hands the region to every GEMM of the call (the heuristic may then split the long
// reduction of a wgrad with few output tiles).  Nothing else of the workspace is initialised.
#include "train_common.h"
#include "internal.h"

namespace {

using namespace train;

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));

constexpr int kThreads = 256;
constexpr int kTile = 64;
constexpr int kSumMinTiles = 4;     // row tiles per strip at least when column sums are wanted: 256 rows
constexpr int kSumMaxStrips = 256;  // bounds the finalize loop
constexpr int kMaxDim = 65535 * 64;  // rows / cols of a pack, M / N / K of a linear: 65535 tiles, the largest y extent of a grid (the pack puts column tiles there)
constexpr size_t kSlabBudget = (size_t)64 << 20;                   // slab space behind the ticket header: 256 persistent workgroups of 256 x 128 tiles
constexpr size_t kSplitBytes = kGemmTicketBytes + kSlabBudget;     // the split-K region at the START of a linear's workspace

enum { WANT_DX = 1, WANT_DW = 2, WANT_DB = 4 };

bool dim_ok(int64_t v) { return v >= kTile && v <= kMaxDim && (v & (kTile - 1)) == 0; }

Strips pack_strips(int rows, bool colsum) {
    const int tiles = rows / kTile;
    return colsum ? plan_strips(tiles, kSumMinTiles, kSumMaxStrips) : Strips{1, tiles};
}

size_t pack_partial_bytes(int rows, int cols, bool colsum) {
    if (!colsum) return 0;
    const Strips s = pack_strips(rows, true);
    return s.count > 1 ? align256((size_t)s.count * cols * sizeof(double)) : 0;
}

// One pass over src [rows, cols] fp32 (both multiples of 64): blockIdx.x = strip of row tiles, blockIdx.y = column tile.
//   ROW: out_row [rows, cols] bf16.   TR: out_tr [cols, rows] bf16.   SUM: part [strips, cols] fp64 (gridDim.x > 1) or colsum [cols] fp32 (one strip).
template <bool ROW, bool TR, bool SUM>
__global__ __launch_bounds__(kThreads) void pack_bf16_kernel(const float* __restrict__ src, int rows, int cols, int tiles_per_strip, unsigned short* __restrict__ out_row,
                                                             unsigned short* __restrict__ out_tr, double* __restrict__ part, float* __restrict__ colsum) {
    __shared__ __attribute__((aligned(16))) unsigned long long lds_t[TR ? 2 * kTile * 16 : 1];
    __shared__ double lds_sum[SUM ? 16 * kTile : 1];
    const int t = threadIdx.x;
    // lane bits: 0 = q bit 0, 1..3 = c4 bits 0..2, 4 = c4 bit 3, 5 = q bit 1; the wave = q bits 2..3
    const int c4 = (t >> 1) & 15;
    const int q = (t & 1) | ((t >> 4) & 2) | ((t >> 6) << 2);
    const int tiles = rows / kTile;
    const int tile0 = blockIdx.x * tiles_per_strip;
    const int tile1 = min(tiles, tile0 + tiles_per_strip);
    const size_t col = (size_t)blockIdx.y * kTile + 4 * c4;
    double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
    for (int tile = tile0, it = 0; tile < tile1; ++tile, ++it) {
        const size_t row = (size_t)tile * kTile + 4 * q;
        const float* p = src + row * cols + col;
        const f32x4 x0 = *reinterpret_cast<const f32x4*>(p);
        const f32x4 x1 = *reinterpret_cast<const f32x4*>(p + (size_t)cols);
        const f32x4 x2 = *reinterpret_cast<const f32x4*>(p + 2 * (size_t)cols);
        const f32x4 x3 = *reinterpret_cast<const f32x4*>(p + 3 * (size_t)cols);
        if (ROW) {
            unsigned short* o = out_row + row * cols + col;
            *reinterpret_cast<bf16x4*>(o) = __builtin_convertvector(x0, bf16x4);
            *reinterpret_cast<bf16x4*>(o + (size_t)cols) = __builtin_convertvector(x1, bf16x4);
            *reinterpret_cast<bf16x4*>(o + 2 * (size_t)cols) = __builtin_convertvector(x2, bf16x4);
            *reinterpret_cast<bf16x4*>(o + 3 * (size_t)cols) = __builtin_convertvector(x3, bf16x4);
        }
        if (SUM) {  // rows ascending
            acc0 += (double)x0[0]; acc1 += (double)x0[1]; acc2 += (double)x0[2]; acc3 += (double)x0[3];
            acc0 += (double)x1[0]; acc1 += (double)x1[1]; acc2 += (double)x1[2]; acc3 += (double)x1[3];
            acc0 += (double)x2[0]; acc1 += (double)x2[1]; acc2 += (double)x2[2]; acc3 += (double)x2[3];
            acc0 += (double)x3[0]; acc1 += (double)x3[1]; acc2 += (double)x3[2]; acc3 += (double)x3[3];
        }
        if (TR) {
            unsigned long long* T = lds_t + (it & 1) * (kTile * 16);
            const int w = q ^ (2 * (c4 & 7));  // (c >> 2) & 7 of the columns 4 c4 + k
#pragma unroll
            for (int k = 0; k < 4; ++k)
                *reinterpret_cast<bf16x4*>(T + (4 * c4 + k) * 16 + w) = __builtin_convertvector(f32x4{x0[k], x1[k], x2[k], x3[k]}, bf16x4);
            __syncthreads();  // the only barrier of a tile: the other buffer is rewritten one tile later, behind the next barrier
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int c = 32 * j + (t >> 3);
                const int m = t & 7;
                const u16x8 v = *reinterpret_cast<const u16x8*>(T + c * 16 + 2 * (m ^ ((c >> 2) & 7)));
                *reinterpret_cast<u16x8*>(out_tr + ((size_t)blockIdx.y * kTile + c) * rows + (size_t)tile * kTile + 8 * m) = v;
            }
        }
    }
    if (SUM) {
        lds_sum[q * kTile + 4 * c4 + 0] = acc0;
        lds_sum[q * kTile + 4 * c4 + 1] = acc1;
        lds_sum[q * kTile + 4 * c4 + 2] = acc2;
        lds_sum[q * kTile + 4 * c4 + 3] = acc3;
        __syncthreads();
        if (t < kTile) {
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < 16; ++i) s += lds_sum[i * kTile + t];  // row quads ascending
            const size_t c = (size_t)blockIdx.y * kTile + t;
            if (gridDim.x > 1) part[(size_t)blockIdx.x * cols + c] = s;
            else colsum[c] = (float)s;
        }
    }
}

// colsum [cols] = the strips' partials in ascending strip order, rounded once; one thread per column
__global__ __launch_bounds__(kThreads) void pack_colsum_finalize_kernel(const double* __restrict__ part, int strips, int cols, float* __restrict__ colsum) {
    const int c = blockIdx.x * kThreads + threadIdx.x;
    if (c >= cols) return;
    double s = 0.0;
#pragma unroll 8  // the loads of eight strips in flight; the additions keep their order
    for (int st = 0; st < strips; ++st) s += part[(size_t)st * cols + c];
    colsum[c] = (float)s;
}

template <bool ROW, bool TR, bool SUM>
void launch_pack_variant(const float* src, int rows, int cols, const Strips& s, unsigned short* out_row, unsigned short* out_tr, double* part, float* colsum,
                         hipStream_t st) {
    hipLaunchKernelGGL((pack_bf16_kernel<ROW, TR, SUM>), dim3((unsigned)s.count, (unsigned)(cols / kTile)), dim3(kThreads), 0, st, src, rows, cols, s.rows, out_row,
                       out_tr, part, colsum);
}

// the launches of one pack; `part` holds pack_partial_bytes(rows, cols, colsum != NULL) bytes.  The caller has checked shapes and alignment.
int launch_pack(const float* src, int rows, int cols, unsigned short* out_row, unsigned short* out_tr, float* colsum, void* part, hipStream_t st) {
    const Strips s = pack_strips(rows, colsum != nullptr);
    double* pd = (double*)part;
    const int which = (out_row ? 1 : 0) | (out_tr ? 2 : 0) | (colsum ? 4 : 0);
    switch (which) {
        case 1: launch_pack_variant<true, false, false>(src, rows, cols, s, out_row, out_tr, pd, colsum, st); break;
        case 2: launch_pack_variant<false, true, false>(src, rows, cols, s, out_row, out_tr, pd, colsum, st); break;
        case 3: launch_pack_variant<true, true, false>(src, rows, cols, s, out_row, out_tr, pd, colsum, st); break;
        case 4: launch_pack_variant<false, false, true>(src, rows, cols, s, out_row, out_tr, pd, colsum, st); break;
        case 5: launch_pack_variant<true, false, true>(src, rows, cols, s, out_row, out_tr, pd, colsum, st); break;
        case 6: launch_pack_variant<false, true, true>(src, rows, cols, s, out_row, out_tr, pd, colsum, st); break;
        case 7: launch_pack_variant<true, true, true>(src, rows, cols, s, out_row, out_tr, pd, colsum, st); break;
        default: return PAELLA_OK;
    }
    LAUNCH_CHECK_RET();
    if (colsum && s.count > 1) {
        hipLaunchKernelGGL(pack_colsum_finalize_kernel, dim3((unsigned)((cols + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, (const double*)pd, s.count, cols, colsum);
        LAUNCH_CHECK_RET();
    }
    return PAELLA_OK;
}

int check_linear_shape(const char* who, int M, int N, int K) {
    // all three reductions (K forward, N dgrad, M wgrad) must pass gemm_bf16_ok, and the pack moves whole 64 x 64 tiles
    if (dim_ok(M) && dim_ok(N) && dim_ok(K) && gemm_bf16_ok(K, K, K) && gemm_bf16_ok(N, N, N) && gemm_bf16_ok(M, M, M)) return PAELLA_OK;
    paella_set_error("%s: unsupported shape M=%d N=%d K=%d (M, N and K must be positive multiples of 64 up to 65535 x 64)", who, M, N, K);
    return PAELLA_ERR_ARG;
}

// workspace of a linear: the split-K region first, then the bf16 operands in the order they are packed, then the partials of db
struct Plan {
    size_t a_off, b_off, c_off, d_off, part_off, bytes;  // forward: a = x16, b = w16; backward: a = dy16, b = dy16T, c = x16T, d = w16T
};

Plan make_plan(int M, int N, int K, bool backward, int wants) {
    Plan p = {};
    size_t off = align256(kSplitBytes);
    auto take = [&](bool on, size_t elems) {
        const size_t o = off;
        if (on) off += align256(elems * sizeof(unsigned short));
        return o;
    };
    const size_t MN = (size_t)M * N, MK = (size_t)M * K, NK = (size_t)N * K;
    if (!backward) {
        p.a_off = take(true, MK);
        p.b_off = take(true, NK);
    } else {
        p.a_off = take(wants & WANT_DX, MN);
        p.b_off = take(wants & WANT_DW, MN);
        p.c_off = take(wants & WANT_DW, MK);
        p.d_off = take(wants & WANT_DX, NK);
        p.part_off = off;
        off += pack_partial_bytes(M, N, (wants & WANT_DB) != 0);
    }
    p.bytes = off;
    return p;
}

GemmArgs bf16_gemm(const unsigned short* A16, int lda, const unsigned short* W16, int ldw, float* C, int M, int N, int K) {
    GemmArgs g = gemm_args(nullptr, lda, nullptr, ldw, C, N, M, N, K);
    g.A16 = A16;
    g.W16 = W16;
    return g;
}

}  // namespace

extern "C" size_t paella_linear_train_workspace_bytes(int M, int N, int K, int direction, int wants) {
    if (!dim_ok(M) || !dim_ok(N) || !dim_ok(K) || (direction != 0 && direction != 1) || (wants & ~7)) return 0;
    return make_plan(M, N, K, direction == 1, wants).bytes;
}

extern "C" int paella_pack_bf16(const float* src, int rows, int cols, unsigned short* out_rowmajor, unsigned short* out_transposed, float* colsum, void* ws,
                                size_t ws_bytes, void* stream) {
    const char* who = "pack_bf16";
    if (!dim_ok(rows) || !dim_ok(cols)) {
        paella_set_error("%s: unsupported shape rows=%d cols=%d (both must be positive multiples of 64 up to 65535 x 64)", who, rows, cols);
        return PAELLA_ERR_ARG;
    }
    if (!src || !(out_rowmajor || out_transposed || colsum)) {
        paella_set_error("%s: src is required, and at least one of out_rowmajor, out_transposed and colsum", who);
        return PAELLA_ERR_ARG;
    }
    int rc = check_tensors_aligned16(who, src, out_rowmajor, out_transposed, colsum);
    if (rc != PAELLA_OK) return rc;
    const size_t need = pack_partial_bytes(rows, cols, colsum != nullptr);
    if (need) {
        rc = check_workspace(who, ws, ws_bytes, need, "the column sums of this shape ask for");
        if (rc != PAELLA_OK) return rc;
    }
    return launch_pack(src, rows, cols, out_rowmajor, out_transposed, colsum, ws, (hipStream_t)stream);
}

extern "C" int paella_linear_train_forward(const float* x, const float* w, const float* bias, float* y, int M, int N, int K, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "linear_train_forward";
    int rc = check_linear_shape(who, M, N, K);
    if (rc == PAELLA_OK) rc = check_required(who, x && w && y, "x, w and y");
    if (rc == PAELLA_OK) rc = check_tensors_aligned16(who, x, w, bias, y);
    if (rc != PAELLA_OK) return rc;
    const Plan pl = make_plan(M, N, K, false, 0);
    rc = check_workspace(who, ws, ws_bytes, pl.bytes, "paella_linear_train_workspace_bytes asks for");
    if (rc != PAELLA_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)ws;
    unsigned short* x16 = (unsigned short*)(base + pl.a_off);
    unsigned short* w16 = (unsigned short*)(base + pl.b_off);
    RET_IF(launch_pack(x, M, K, x16, nullptr, nullptr, nullptr, st));
    RET_IF(launch_pack(w, N, K, w16, nullptr, nullptr, nullptr, st));
    HIP_CHECK_RET(hipMemsetAsync(ws, 0, kGemmTicketBytes, st));
    GemmArgs g = bf16_gemm(x16, K, w16, K, y, M, N, K);
    g.ep.bias = bias;
    return launch_gemm(g, ws, kSplitBytes, st);
}

extern "C" int paella_linear_train_backward(const float* x, const float* w, const float* dy, float* dx, float* dw, float* db, int M, int N, int K, void* ws,
                                            size_t ws_bytes, void* stream) {
    const char* who = "linear_train_backward";
    int rc = check_linear_shape(who, M, N, K);
    if (rc != PAELLA_OK) return rc;
    if (!dy || (dx && !w) || (dw && !x)) {
        paella_set_error("%s: dy is required, and w for dx_out, x for dw_out", who);
        return PAELLA_ERR_ARG;
    }
    rc = check_tensors_aligned16(who, x, w, dy, dx, dw, db);
    if (rc != PAELLA_OK) return rc;
    const int wants = (dx ? WANT_DX : 0) | (dw ? WANT_DW : 0) | (db ? WANT_DB : 0);
    const Plan pl = make_plan(M, N, K, true, wants);
    rc = check_workspace(who, ws, ws_bytes, pl.bytes, "paella_linear_train_workspace_bytes asks for");
    if (rc != PAELLA_OK) return rc;
    if (!wants) return PAELLA_OK;
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)ws;
    unsigned short* dy16 = dx ? (unsigned short*)(base + pl.a_off) : nullptr;
    unsigned short* dy16t = dw ? (unsigned short*)(base + pl.b_off) : nullptr;
    unsigned short* x16t = dw ? (unsigned short*)(base + pl.c_off) : nullptr;
    unsigned short* w16t = dx ? (unsigned short*)(base + pl.d_off) : nullptr;
    RET_IF(launch_pack(dy, M, N, dy16, dy16t, db, base + pl.part_off, st));
    if (dw) RET_IF(launch_pack(x, M, K, nullptr, x16t, nullptr, nullptr, st));
    if (dx) RET_IF(launch_pack(w, N, K, nullptr, w16t, nullptr, nullptr, st));
    if (!dx && !dw) return PAELLA_OK;
    HIP_CHECK_RET(hipMemsetAsync(ws, 0, kGemmTicketBytes, st));
    if (dx) RET_IF(launch_gemm(bf16_gemm(dy16, N, w16t, N, dx, M, K, N), ws, kSplitBytes, st));
    if (dw) RET_IF(launch_gemm(bf16_gemm(dy16t, M, x16t, M, dw, N, K, M), ws, kSplitBytes, st));
    return PAELLA_OK;
}
