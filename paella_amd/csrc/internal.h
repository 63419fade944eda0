// Host-side helpers shared by model.hip (UNet) and vqmodel.hip (VQGAN).
#pragma once
#include "common.h"
#include "../../include/paella_hip.h"
#include <vector>

#define RET_IF(expr)                      \
    do {                                  \
        int _rc = (expr);                 \
        if (_rc != PAELLA_OK) return _rc; \
    } while (0)

// library-owned device tensor (repacked weight)
struct DevBuf {
    float* p = nullptr;
    size_t n = 0;
    bool loaded = false;
};
int devbuf_alloc(DevBuf& b, size_t n);
struct DevBuf16 {  // bf16 shadow copy of a weight (opt-in fast mode)
    unsigned short* p = nullptr;
    size_t n = 0;
};

// bump allocator over a caller-owned workspace; base == nullptr -> size query only
struct Arena {
    char* base;
    size_t cap, off;
    bool ok;
    Arena(void* b, size_t c) : base((char*)b), cap(c), off(0), ok(true) {}
    float* take(size_t nfloats) {
        const size_t bytes = (nfloats * sizeof(float) + 255) & ~(size_t)255;
        const size_t o = off;
        off += bytes;
        if (base && off > cap) ok = false;
        return base ? (float*)(base + o) : nullptr;
    }
};

static const size_t kSplitKBudget = (size_t)96 << 20;  // bytes of the split-K region (ticket header + slabs) at the START of every workspace

enum Repack {
    RP_COPY,      // as is
    RP_DW,        // depthwise [C, J, 3, 3] -> [J, 3, 3, C]
    RP_CONV_K2,   // conv [co, ci, kh, kw] -> [co, kh, kw, ci]
    RP_CONVT_K2,  // transposed conv [ci, co, kh, kw] -> [kh, kw, co, ci]
    RP_TILE4,     // bias [c] -> [4][c]
    RP_CLF_W, RP_CLF_B, RP_TS_W, RP_TS_B  // handled by the UNet loader
};
int repack_into(Repack kind, const float* src, const std::vector<int64_t>& shape, DevBuf& dst, hipStream_t st);

// One state-dict tensor of a model: what the loader expects under its key, and the SLOTS of everything made from it.  The models keep these in a std::map by key
// (node addresses never move), the plans bind `Weight*` members to them, and a launch reads slot.p when it is enqueued -- so a reload that reallocates, or a
// shadow that first appears at a later set_precision(1), needs no re-bind.  A slot nobody filled is a null pointer.
struct Weight {
    Repack kind;
    std::vector<int64_t> shape;  // expected reference shape
    int aux = 0;                 // RP_TS_*: offset into the concatenated timestep mapper
    DevBuf w;                    // repacked fp32 tensor
    DevBuf16 w16;                // its bf16 shadow (make_shadows; read only in precision mode 1)
    DevBuf wsum, wsum16;         // LayerNorm-consuming weights: row sums of w (finalize) / of the rounded w (make_shadows)
};
int weight_make_shadow(Weight& t, hipStream_t st);  // refreshes t.w16 from t.w as loaded now
void weight_free(Weight& t);

// Argument blocks (include/paella_hip.h: paella_tail_args / paella_step_args; tail.hip, model.hip).  What a fixed-form entry point's NAME promises on top of what
// its block holds (a block alone takes its form from what is present): the request form, its stream tables, the scalar filter values, a guidance pair table.
enum { kNeedRequest = 1, kNeedStream = 2, kNeedFilter = 4, kNeedPairs = 8 };
int tail_pin_check(const char* who, const TailArgs& a);
int tail_block_convert(const char* who, const paella_tail_args& t, int need, bool fused, TailArgs& a, TailFilter& f, TailStats& s, int* kind);
// the two fillers of a tail block, from the parameter lists of the scalar and of the request / stream entry points (absent tables null)
static inline paella_tail_args tail_block_scalar(const float* logits_c, const float* logits_u, int64_t rows, int L, float cfg, float one_minus_cfg, float temperature, int mode,
                                                 uint64_t seed, const uint64_t* seed_ptr, uint64_t offset, int64_t row_offset, const int64_t* row_offset_ptr,
                                                 const int64_t* init_noise, float t_next, const int64_t* pin_keep, const int64_t* pin_tokens, int64_t* tokens_out,
                                                 int64_t* sampled_out) {
    paella_tail_args t = {};
    t.logits_c = logits_c; t.logits_u = logits_u; t.rows = rows; t.L = L; t.cfg = cfg; t.one_minus_cfg = one_minus_cfg; t.temperature = temperature; t.mode = mode;
    t.seed = seed; t.seed_ptr = seed_ptr; t.offset = offset; t.row_offset = row_offset; t.row_offset_ptr = row_offset_ptr; t.init_noise = init_noise; t.t_next = t_next;
    t.pin_keep = pin_keep; t.pin_tokens = pin_tokens; t.tokens_out = tokens_out; t.sampled_out = sampled_out;
    return t;
}
static inline paella_tail_args tail_block_stream(const float* logits_c, const float* logits_u, int64_t rows, int L, const float* cfg_pairs, const float* temperature,
                                                 const uint64_t* seeds, int rows_per_sample, const int* step, const float* t_next, const int* active, const int64_t* init_noise,
                                                 const int64_t* pin_keep, const int64_t* pin_tokens, const int* pin_on, int64_t* tokens_out, int64_t* sampled_out) {
    paella_tail_args t = {};
    t.logits_c = logits_c; t.logits_u = logits_u; t.rows = rows; t.L = L; t.cfg_pairs = cfg_pairs; t.temperature_tab = temperature; t.seeds = seeds;
    t.rows_per_sample = rows_per_sample; t.step = step; t.t_next_tab = t_next; t.active = active; t.init_noise = init_noise;
    t.pin_keep = pin_keep; t.pin_tokens = pin_tokens; t.pin_on = pin_on; t.tokens_out = tokens_out; t.sampled_out = sampled_out;
    return t;
}

static inline GemmArgs gemm_args(const float* A, int lda, const float* Wt, int ldw, float* C, int ldc, int M, int N, int K) {
    GemmArgs g;
    g.A = A; g.lda = lda; g.W = Wt; g.ldw = ldw; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K;
    g.a_scale = nullptr; g.a_shift = nullptr; g.a_rows_per_sample = 1; g.a_rps_div.mul = 0; g.a_rps_div.shr = 0; g.a_rps_div.pass = 0xffffffffu; g.grn_gx = nullptr; g.grn_gamma = nullptr; g.grn_part = nullptr; g.grn_np = 0; g.force_ring_cfg = 0; g.ln_stats = nullptr; g.ln_nblk = 0; g.ln_eps = 1e-6f; g.ln_wsum = nullptr; g.ln_row = nullptr; g.ln_fold_ratio = 4.0f; g.ln_guard_count = nullptr;
    g.ep = make_epilogue();
    g.ft.temperature = 1.f; g.ft.mode = 0; g.ft.seed = 0; g.ft.seed_ptr = nullptr; g.ft.offset = 0; g.ft.row_offset = 0; g.ft.row_offset_ptr = nullptr;
    g.ft.part_score = nullptr; g.ft.part_idx = nullptr;
    g.cv.enabled = 0;
    g.A16 = nullptr; g.W16 = nullptr;
    return g;
}
