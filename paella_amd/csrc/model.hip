// Denoising-UNet execution plan and C ABI (include/paella_hip.h) for gfx950.
//
// The whole forward (reference src/modules.py:263-275 Paella.forward, :234-261 _down_encode/_up_decode) is
// enqueued by ONE call from the host: the block list is walked natively, every op is a HIP kernel from
// gemm.hip / elementwise.hip / attention.hip, activations stay NHWC in a caller-owned workspace arena, and
// nothing synchronises the host.  Weights are repacked once at load (paella_unet_load_tensor).
#include "internal.h"
#include "test_hooks.h"
#include "../../include/paella_hip.h"

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

// ---------------------------------------------------------------------------
// error string
// ---------------------------------------------------------------------------
static thread_local char g_err[2048] = "";
void paella_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* paella_last_error(void) { return g_err; }
extern "C" int paella_abi_version(void) { return PAELLA_ABI_VERSION; }

// ---------------------------------------------------------------------------
// library-owned device tensors
// ---------------------------------------------------------------------------
int devbuf_alloc(DevBuf& b, size_t n) {
    if (b.p && b.n == n) return PAELLA_OK;
    if (b.p) { (void)hipFree(b.p); b.p = nullptr; }
    b.n = n;
    HIP_CHECK_RET(hipMalloc((void**)&b.p, (n ? n : 1) * sizeof(float)));
    return PAELLA_OK;
}

// ---------------------------------------------------------------------------
// plan
//
// A state-dict key is written ONCE, in build_plan: the add_spec call that declares the tensor (key, repack kind, expected shape) returns its Weight (internal.h),
// and the same statement binds it to the member of the Block / paella_unet that the launches read.  paella_unet_load_tensor, the "never loaded" check of
// paella_unet_finalize and paella_unet_destroy are the only code that goes through the names; everything else follows the bound pointers.  What is derived from a
// weight (bf16 shadow, row sums) lives in slots of the same Weight, listed once at the end of build_plan (shadowed / ln_weights).
// ---------------------------------------------------------------------------
enum BlockType { BT_RES, BT_TS, BT_ATTN, BT_FF, BT_DOWN, BT_UP };

struct Block {
    BlockType type;
    int level = 0;
    int c = 0;
    bool has_skip = false;
    int ts_offset = -1;        // BT_TS: offset of [a|b] in the ts vector
    bool ts_standalone = true; // BT_TS: false when fused into the previous block's GEMM epilogue
    int fused_ts = -1;         // BT_RES/BT_FF: ts offset fused into GEMM2, or -1
    int attn_index = -1;
    bool emit_rowstat = false;   // producer: this block's last GEMM also writes per-row (sum, centred M2) partials of x
    bool ln_from_stats = false;  // consumer (ATTN / UP): LayerNorm folded into the GEMM's A-operand load from those partials
    int c_from = 0, c_to = 0;  // samplers
    // the tensors this block type reads
    Weight *dw_w = nullptr, *dw_b = nullptr;                                                                  // BT_RES: depthwise conv
    Weight *w1 = nullptr, *b1 = nullptr, *gamma = nullptr, *beta = nullptr, *w2 = nullptr, *b2 = nullptr;       // BT_RES / BT_FF: MLP with GlobalResponseNorm
    Weight *in_w = nullptr, *in_b = nullptr, *out_w = nullptr, *out_b = nullptr, *kv_w = nullptr, *kv_b = nullptr;  // BT_ATTN
    Weight *conv_w = nullptr, *conv_b = nullptr;                                                              // BT_DOWN / BT_UP
};

struct LnWeight { Weight* t; int N, K; };  // a weight whose GEMM consumes LayerNorm-from-statistics, with (N, K) of the repacked matrix

struct paella_unet {
    paella_unet_config cfg;
    std::vector<Block> down, up;  // execution order, samplers included
    std::map<std::string, Weight> t;  // every state-dict tensor by key; the members below and the Blocks point into it
    Weight *byt5_w, *byt5_b, *clip_w, *clip_b, *clip_image_w, *clip_image_b;
    Weight *in_mapper, *embedding_w, *embedding_b, *clf_w, *clf_b, *out_mapper;
    std::vector<Weight*> shadowed;     // the weights a bf16 GEMM of the forward reads (execution order)
    std::vector<LnWeight> ln_weights;  // the LayerNorm-consuming ones: row sums for the LayerNorm folded into the GEMM epilogue
    DevBuf ts_w, ts_b, freqs;
    // conditioning K|V of EVERY AttnBlock as one GEMM: kv_w [kv_total, c_cond] = rows of in_proj_weight[c:3c] . kv_mapper.1.weight per block
    // (composed at finalize), kv_b = in_proj_weight[c:3c] . kv_mapper.1.bias + in_proj_bias[c:3c]; kv_col[i] = first column of block i
    DevBuf kv_w, kv_b;
    // OPT-IN bf16 fast mode, PER MODEL (paella_unet_set_precision; outside the fp32 parity contract): bf16 shadow copies of the GEMM weights (made at finalize /
    // when the mode is switched on) and the row sums of the ROUNDED LayerNorm-consuming weights
    int precision = 0;                   // 0 = exact fp32 (default), 1 = bf16 operands
    std::vector<int> kv_col;
    int kv_total = 0;
    int ts_total = 0;
    int n_attn = 0;
    std::vector<int> attn_c;      // channel width per attention block (execution order)
    bool finalized = false;
    bool freqs_set = false;
    bool clf_from_stats = false;
    int c_max = 0;
};

// bf16 shadow of a weight, or null (fp32 mode / no shadow for this tensor)
static const unsigned short* W16(const paella_unet* m, const Weight* t) { return m->precision == 1 ? t->w16.p : nullptr; }

static Weight* add_spec(paella_unet* m, const std::string& key, Repack kind, std::vector<int64_t> shape, int aux = 0) {
    Weight& t = m->t[key];
    t.kind = kind; t.shape = std::move(shape); t.aux = aux;
    return &t;
}

static int build_plan(paella_unet* m) {
    const paella_unet_config& c = m->cfg;
    if (c.n_levels < 1 || c.n_levels > PAELLA_MAX_LEVELS) { paella_set_error("n_levels out of range"); return PAELLA_ERR_ARG; }
    if (c.kernel_size != 3) { paella_set_error("kernel_size %d unsupported (3 only)", c.kernel_size); return PAELLA_ERR_ARG; }
    if (c.patch_size != 1 && c.patch_size != 2) { paella_set_error("patch_size %d unsupported (1 or 2)", c.patch_size); return PAELLA_ERR_ARG; }
    if ((c.c_in & 3) || (c.c_out & 3) || (c.num_labels & 3) || (c.c_cond & 3) || (c.clip_embd & 3) || (c.byt5_embd & 3)) {
        paella_set_error("c_in, c_out, num_labels, c_cond, clip_embd, byt5_embd must be multiples of 4");
        return PAELLA_ERR_ARG;
    }
    const int p2 = c.patch_size * c.patch_size;
    const int64_t cr = c.c_r, cc = c.c_cond;
    m->byt5_w = add_spec(m, "byt5_mapper.weight", RP_COPY, {cc, c.byt5_embd});
    m->byt5_b = add_spec(m, "byt5_mapper.bias", RP_COPY, {cc});
    m->clip_w = add_spec(m, "clip_mapper.weight", RP_COPY, {cc * c.clip_seq_len, c.clip_embd});
    m->clip_b = add_spec(m, "clip_mapper.bias", RP_COPY, {cc * c.clip_seq_len});
    m->clip_image_w = add_spec(m, "clip_image_mapper.weight", RP_COPY, {cc * c.clip_seq_len, c.clip_embd});
    m->clip_image_b = add_spec(m, "clip_image_mapper.bias", RP_COPY, {cc * c.clip_seq_len});
    m->in_mapper = add_spec(m, "in_mapper.0.weight", RP_COPY, {c.num_labels, c.c_in});
    m->embedding_w = add_spec(m, "embedding.1.weight", RP_COPY, {c.c_hidden[0], (int64_t)c.c_in * p2, 1, 1});
    m->embedding_b = add_spec(m, "embedding.1.bias", RP_COPY, {c.c_hidden[0]});
    m->clf_w = add_spec(m, "clf.1.weight", RP_CLF_W, {(int64_t)c.c_out * p2, c.c_hidden[0], 1, 1});
    m->clf_b = add_spec(m, "clf.1.bias", RP_CLF_B, {(int64_t)c.c_out * p2});
    m->out_mapper = add_spec(m, "out_mapper.1.weight", RP_COPY, {c.num_labels, c.c_out, 1, 1});

    int ts_total = 0, n_attn = 0;
    auto add_block = [&](std::vector<Block>& seq, char type, int level, const std::string& prefix, bool skip) -> int {
        Block b;
        b.level = level; b.c = c.c_hidden[level];
        const int64_t ch = b.c;
        if (ch & 7) { paella_set_error("c_hidden[%d]=%d must be a multiple of 8", level, b.c); return PAELLA_ERR_ARG; }
        switch (type) {
            case 'C':
                b.type = BT_RES; b.has_skip = skip;
                b.dw_w = add_spec(m, prefix + ".depthwise.weight", RP_DW, {ch, skip ? 2 : 1, 3, 3});
                b.dw_b = add_spec(m, prefix + ".depthwise.bias", RP_COPY, {ch});
                /* fallthrough */
            case 'F':
                if (type == 'F') b.type = BT_FF;
                b.w1 = add_spec(m, prefix + ".channelwise.0.weight", RP_COPY, {4 * ch, ch});
                b.b1 = add_spec(m, prefix + ".channelwise.0.bias", RP_COPY, {4 * ch});
                b.gamma = add_spec(m, prefix + ".channelwise.2.gamma", RP_COPY, {1, 1, 1, 4 * ch});
                b.beta = add_spec(m, prefix + ".channelwise.2.beta", RP_COPY, {1, 1, 1, 4 * ch});
                b.w2 = add_spec(m, prefix + ".channelwise.4.weight", RP_COPY, {ch, 4 * ch});
                b.b2 = add_spec(m, prefix + ".channelwise.4.bias", RP_COPY, {ch});
                break;
            case 'T':
                b.type = BT_TS; b.ts_offset = ts_total;
                add_spec(m, prefix + ".mapper.weight", RP_TS_W, {2 * ch, cr}, ts_total);
                add_spec(m, prefix + ".mapper.bias", RP_TS_B, {2 * ch}, ts_total);
                ts_total += 2 * b.c;
                if (!seq.empty() && (seq.back().type == BT_RES || seq.back().type == BT_FF) && seq.back().level == level &&
                    seq.back().fused_ts < 0) {
                    seq.back().fused_ts = b.ts_offset;
                    b.ts_standalone = false;
                }
                break;
            case 'A': {
                b.type = BT_ATTN; b.attn_index = n_attn++;
                m->attn_c.push_back(b.c);
                const int nh = c.nhead[level];
                if (nh <= 0 || b.c % nh || (b.c / nh) % 16 || b.c / nh > 128) {
                    paella_set_error("level %d: c=%d nhead=%d -> head_dim must be a multiple of 16 and <= 128", level, b.c, nh);
                    return PAELLA_ERR_ARG;
                }
                b.in_w = add_spec(m, prefix + ".attention.attn.in_proj_weight", RP_COPY, {3 * ch, ch});
                b.in_b = add_spec(m, prefix + ".attention.attn.in_proj_bias", RP_COPY, {3 * ch});
                b.out_w = add_spec(m, prefix + ".attention.attn.out_proj.weight", RP_COPY, {ch, ch});
                b.out_b = add_spec(m, prefix + ".attention.attn.out_proj.bias", RP_COPY, {ch});
                b.kv_w = add_spec(m, prefix + ".kv_mapper.1.weight", RP_COPY, {ch, cc});
                b.kv_b = add_spec(m, prefix + ".kv_mapper.1.bias", RP_COPY, {ch});
                break;
            }
            default:
                paella_set_error("Block type %c not supported", type);
                return PAELLA_ERR_ARG;
        }
        seq.push_back(b);
        return PAELLA_OK;
    };

    char buf[128];
    // DOWN (reference src/modules.py:148-160)
    for (int i = 0; i < c.n_levels; ++i) {
        int j = 0;
        if (i > 0) {
            Block b;
            b.type = BT_DOWN; b.level = i; b.c = c.c_hidden[i]; b.c_from = c.c_hidden[i - 1]; b.c_to = c.c_hidden[i];
            snprintf(buf, sizeof buf, "down_blocks.%d.0.1", i);
            b.conv_w = add_spec(m, std::string(buf) + ".weight", RP_CONV_K2, {b.c_to, b.c_from, 2, 2});
            b.conv_b = add_spec(m, std::string(buf) + ".bias", RP_COPY, {b.c_to});
            m->down.push_back(b);
            j = 1;
        }
        for (int r = 0; r < c.blocks[i]; ++r)
            for (const char* t = c.level_config[i]; *t; ++t) {
                snprintf(buf, sizeof buf, "down_blocks.%d.%d", i, j++);
                RET_IF(add_block(m->down, *t, i, buf, false));
            }
    }
    // UP (reference src/modules.py:163-176)
    for (int u = 0; u < c.n_levels; ++u) {
        const int i = c.n_levels - 1 - u;
        int j = 0;
        for (int r = 0; r < c.blocks[i]; ++r) {
            int k = 0;
            for (const char* t = c.level_config[i]; *t; ++t, ++k) {
                snprintf(buf, sizeof buf, "up_blocks.%d.%d", u, j++);
                const bool skip = (i < c.n_levels - 1) && r == 0 && k == 0 && *t == 'C';
                RET_IF(add_block(m->up, *t, i, buf, skip));
            }
        }
        if (i > 0) {
            Block b;
            b.type = BT_UP; b.level = i; b.c = c.c_hidden[i]; b.c_from = c.c_hidden[i]; b.c_to = c.c_hidden[i - 1];
            snprintf(buf, sizeof buf, "up_blocks.%d.%d.1", u, j);
            b.conv_w = add_spec(m, std::string(buf) + ".weight", RP_CONVT_K2, {b.c_from, b.c_to, 2, 2});
            b.conv_b = add_spec(m, std::string(buf) + ".bias", RP_TILE4, {b.c_to});
            m->up.push_back(b);
        }
    }
    m->ts_total = ts_total;
    // LayerNorm-on-load planning: a consumer LN (AttnBlock, up-sampler, clf) whose input x was last written by a GEMM
    // epilogue (ResBlock / FeedForward GEMM2 incl. a fused TimestepBlock, or an AttnBlock's out-projection) gets its row
    // statistics from that epilogue and folds the normalisation into its own GEMM's operand load -- no LN launch.
    {
        std::vector<Block*> all;
        for (Block& b : m->down) all.push_back(&b);
        for (Block& b : m->up) all.push_back(&b);
        auto producer_of = [&](size_t idx) -> Block* {
            if (idx == 0) return nullptr;
            Block* p = all[idx - 1];
            if (p->type == BT_TS && !p->ts_standalone && idx >= 2) p = all[idx - 2];
            else if (p->type == BT_TS) return nullptr;
            if ((p->type == BT_RES || p->type == BT_FF || p->type == BT_ATTN) && (p->c % 16) == 0) return p;
            return nullptr;
        };
        for (size_t i = 0; i < all.size(); ++i) {
            Block* b = all[i];
            if (b->type != BT_ATTN && b->type != BT_UP) continue;
            Block* p = producer_of(i);
            if (p && p->level == b->level) { p->emit_rowstat = true; b->ln_from_stats = true; }
        }
        Block* p = producer_of(all.size());
        if (p && p->level == 0) { p->emit_rowstat = true; m->clf_from_stats = true; }
        // what is derived from the weights: the ones a bf16 GEMM reads get a bf16 shadow, the LayerNorm-folding ones their row sums (finalize, make_shadows)
        auto gemm_weight = [&](Weight* t, bool ln, int N, int K) {
            m->shadowed.push_back(t);
            if (ln) m->ln_weights.push_back({t, N, K});
        };
        for (const Block* b : all) switch (b->type) {
            case BT_RES: case BT_FF: gemm_weight(b->w1, false, 0, 0); gemm_weight(b->w2, false, 0, 0); break;
            case BT_ATTN: gemm_weight(b->in_w, b->ln_from_stats, 3 * b->c, b->c); gemm_weight(b->out_w, false, 0, 0); break;
            case BT_DOWN: gemm_weight(b->conv_w, false, 0, 0); break;
            case BT_UP: gemm_weight(b->conv_w, b->ln_from_stats, 4 * b->c_to, b->c_from); break;
            default: break;
        }
        gemm_weight(m->clf_w, m->clf_from_stats, c.c_out * p2, c.c_hidden[0]);
        gemm_weight(m->out_mapper, false, 0, 0);
    }
    m->n_attn = n_attn;
    m->c_max = 0;
    for (int i = 0; i < c.n_levels; ++i) m->c_max = c.c_hidden[i] > m->c_max ? c.c_hidden[i] : m->c_max;
    return PAELLA_OK;
}

extern "C" int paella_unet_create(const paella_unet_config* cfg, paella_unet** out) {
    if (!cfg || !out) { paella_set_error("null argument"); return PAELLA_ERR_ARG; }
    paella_unet* m = new paella_unet();
    m->cfg = *cfg;
    for (int i = 0; i < PAELLA_MAX_LEVELS; ++i) m->cfg.level_config[i][PAELLA_MAX_BLOCK_TYPES - 1] = 0;
    int rc = build_plan(m);
    if (rc != PAELLA_OK) { delete m; return rc; }
    if (m->ts_total > 0) {
        rc = devbuf_alloc(m->ts_w, (size_t)m->ts_total * cfg->c_r);
        if (rc == PAELLA_OK) rc = devbuf_alloc(m->ts_b, (size_t)m->ts_total);
        if (rc != PAELLA_OK) { delete m; return rc; }
    }
    *out = m;
    return PAELLA_OK;
}

extern "C" void paella_unet_destroy(paella_unet* m) {
    if (!m) return;
    for (auto& kv : m->t) weight_free(kv.second);
    if (m->kv_w.p) (void)hipFree(m->kv_w.p);
    if (m->kv_b.p) (void)hipFree(m->kv_b.p);
    if (m->ts_w.p) (void)hipFree(m->ts_w.p);
    if (m->ts_b.p) (void)hipFree(m->ts_b.p);
    if (m->freqs.p) (void)hipFree(m->freqs.p);
    delete m;
}

// shared by the UNet and VQGAN loaders
void weight_free(Weight& t) {
    if (t.w.p) (void)hipFree(t.w.p);
    if (t.w16.p) (void)hipFree(t.w16.p);
    if (t.wsum.p) (void)hipFree(t.wsum.p);
    if (t.wsum16.p) (void)hipFree(t.wsum16.p);
}
int weight_make_shadow(Weight& t, hipStream_t st) {
    DevBuf16& d = t.w16;
    if (d.p && d.n != t.w.n) { (void)hipFree(d.p); d.p = nullptr; }
    if (!d.p) HIP_CHECK_RET(hipMalloc((void**)&d.p, t.w.n * sizeof(unsigned short)));
    d.n = t.w.n;
    return launch_f32_to_bf16(t.w.p, d.p, d.n, st);
}
int repack_into(Repack kind, const float* src, const std::vector<int64_t>& shape, DevBuf& dst, hipStream_t st) {
    int64_t numel = 1;
    for (int64_t d : shape) numel *= d;
    switch (kind) {
        case RP_COPY:
            RET_IF(devbuf_alloc(dst, numel));
            HIP_CHECK_RET(hipMemcpyAsync(dst.p, src, numel * sizeof(float), hipMemcpyDeviceToDevice, st));
            break;
        case RP_DW: {  // [C, J, 3, 3] -> [J, 3, 3, C]
            RET_IF(devbuf_alloc(dst, numel));
            const int perm[4] = {1, 2, 3, 0};
            RET_IF(launch_permute(src, dst.p, shape.data(), perm, 4, st));
            break;
        }
        case RP_CONV_K2: {  // [co, ci, kh, kw] -> [co, kh, kw, ci]
            RET_IF(devbuf_alloc(dst, numel));
            const int perm[4] = {0, 2, 3, 1};
            RET_IF(launch_permute(src, dst.p, shape.data(), perm, 4, st));
            break;
        }
        case RP_CONVT_K2: {  // [ci, co, kh, kw] -> [kh, kw, co, ci]
            RET_IF(devbuf_alloc(dst, numel));
            const int perm[4] = {2, 3, 1, 0};
            RET_IF(launch_permute(src, dst.p, shape.data(), perm, 4, st));
            break;
        }
        case RP_TILE4:  // [c] -> [4][c]
            RET_IF(devbuf_alloc(dst, numel * 4));
            for (int r = 0; r < 4; ++r)
                HIP_CHECK_RET(hipMemcpyAsync(dst.p + r * numel, src, numel * sizeof(float), hipMemcpyDeviceToDevice, st));
            break;
        default:
            paella_set_error("internal: unexpected repack kind");
            return PAELLA_ERR_STATE;
    }
    dst.loaded = true;
    return PAELLA_OK;
}

extern "C" int paella_unet_load_tensor(paella_unet* m, const char* key, const float* dev_src, const int64_t* shape, int ndim,
                                       void* stream) {
    if (!m || !key || !dev_src) { paella_set_error("null argument"); return PAELLA_ERR_ARG; }
    hipStream_t st = (hipStream_t)stream;
    auto it = m->t.find(key);
    if (it == m->t.end()) { paella_set_error("unexpected state-dict key '%s'", key); return PAELLA_ERR_ARG; }
    const Weight& sp = it->second;
    if ((int)sp.shape.size() != ndim) { paella_set_error("%s: expected %d dims, got %d", key, (int)sp.shape.size(), ndim); return PAELLA_ERR_ARG; }
    int64_t numel = 1;
    for (int d = 0; d < ndim; ++d) {
        if (shape[d] != sp.shape[d]) { paella_set_error("%s: dim %d is %lld, expected %lld", key, d, (long long)shape[d], (long long)sp.shape[d]); return PAELLA_ERR_ARG; }
        numel *= shape[d];
    }
    const int p2 = m->cfg.patch_size * m->cfg.patch_size;
    DevBuf& dst = it->second.w;
    switch (sp.kind) {
        case RP_TS_W:
            HIP_CHECK_RET(hipMemcpyAsync(m->ts_w.p + (size_t)sp.aux * m->cfg.c_r, dev_src, numel * sizeof(float), hipMemcpyDeviceToDevice, st));
            dst.loaded = true;
            break;
        case RP_TS_B:
            HIP_CHECK_RET(hipMemcpyAsync(m->ts_b.p + sp.aux, dev_src, numel * sizeof(float), hipMemcpyDeviceToDevice, st));
            dst.loaded = true;
            break;
        case RP_CLF_W: {  // [c_out*p2, c0] rows (c, s) -> (s, c)
            RET_IF(devbuf_alloc(dst, numel));
            const int64_t sh[3] = {m->cfg.c_out, p2, m->cfg.c_hidden[0]};
            const int perm[3] = {1, 0, 2};
            RET_IF(launch_permute(dev_src, dst.p, sh, perm, 3, st));
            dst.loaded = true;
            break;
        }
        case RP_CLF_B: {
            RET_IF(devbuf_alloc(dst, numel));
            const int64_t sh[2] = {m->cfg.c_out, p2};
            const int perm[2] = {1, 0};
            RET_IF(launch_permute(dev_src, dst.p, sh, perm, 2, st));
            dst.loaded = true;
            break;
        }
        default:
            RET_IF(repack_into(sp.kind, dev_src, sp.shape, dst, st));
    }
    return PAELLA_OK;
}

extern "C" int paella_unet_set_timestep_freqs(paella_unet* m, const float* host_freqs, int n) {
    if (!m || !host_freqs) { paella_set_error("null argument"); return PAELLA_ERR_ARG; }
    if (n != m->cfg.c_r / 2) { paella_set_error("expected %d frequencies, got %d", m->cfg.c_r / 2, n); return PAELLA_ERR_ARG; }
    RET_IF(devbuf_alloc(m->freqs, n));
    HIP_CHECK_RET(hipMemcpy(m->freqs.p, host_freqs, n * sizeof(float), hipMemcpyHostToDevice));
    m->freqs_set = true;
    return PAELLA_OK;
}

// bf16 shadow copies of every weight a bf16 GEMM of the forward reads (+ row sums of the rounded LayerNorm-consuming ones), from the tensors as loaded now
static int make_shadows(paella_unet* m, hipStream_t st) {
    for (Weight* t : m->shadowed)
        if (t->w.p && !(t->w.n & 7)) RET_IF(weight_make_shadow(*t, st));
    for (const LnWeight& l : m->ln_weights) {
        if (!l.t->w16.p || (l.K & 7)) continue;
        RET_IF(devbuf_alloc(l.t->wsum16, (size_t)l.N));
        RET_IF(launch_rowsum_bf16(l.t->w16.p, l.t->wsum16.p, l.N, l.K, st));
    }
    HIP_CHECK_RET(hipStreamSynchronize(st));
    return PAELLA_OK;
}

// OPT-IN fast mode of THIS model (no process-wide state): mode 1 routes the forward's dense contractions whose K is a multiple of 64 through bf16-operand
// MFMA with fp32 accumulation -- bf16 shadow weights, bf16 activations between producer and consumer GEMMs (the 4c-wide MLP hidden tensor, the LayerNorm /
// attention outputs, a bf16 copy of the residual stream where a LayerNorm-folding GEMM reads it); the residual stream, statistics, attention, logits and the
// sampling tail stay fp32.  Workspaces must be sized (paella_unet_workspace_bytes) AFTER the switch.  Mode 0 (default) = the exact path, bit for bit.
extern "C" int paella_unet_set_precision(paella_unet* m, int mode, void* stream) {
    if (!m) { paella_set_error("null argument"); return PAELLA_ERR_ARG; }
    if (mode != 0 && mode != 1) { paella_set_error("precision mode must be 0 (fp32) or 1 (bf16 operands)"); return PAELLA_ERR_ARG; }
    m->precision = mode;
    if (mode == 1 && m->finalized) return make_shadows(m, (hipStream_t)stream);
    // mode 0: the bf16 shadows stay allocated until paella_unet_destroy: a HIP graph captured in the fast mode keeps raw pointers to them, so a
    // replay after the switch reads stale-but-live memory instead of freed memory (the Python GraphSampler refuses / recaptures such a graph anyway), and
    // nothing here synchronises, so the call is legal while another stream is capturing.  A later switch back to mode 1 refreshes them (make_shadows).
    return PAELLA_OK;
}
extern "C" int paella_unet_get_precision(const paella_unet* m) { return m ? m->precision : 0; }

extern "C" int paella_unet_finalize(paella_unet* m, void* stream) {
    if (!m) { paella_set_error("null argument"); return PAELLA_ERR_ARG; }
    for (auto& kv : m->t)
        if (!kv.second.w.loaded) { paella_set_error("tensor '%s' was never loaded", kv.first.c_str()); return PAELLA_ERR_STATE; }
    // Row sums of every weight whose GEMM consumes LayerNorm-from-statistics (the LayerNorm is folded into that GEMM's epilogue: gemm.hip, ln_row_stats):
    // wsum[n] = sum_k W[n][k], as one M = 1 GEMM over a vector of ones per weight.
    {
        hipStream_t st = (hipStream_t)stream;
        const std::vector<LnWeight>& todo = m->ln_weights;
        if (!todo.empty()) {
            int kmax = 0;
            for (const LnWeight& l : todo) kmax = l.K > kmax ? l.K : kmax;
            std::vector<float> ones_h((size_t)kmax, 1.0f);
            DevBuf ones;
            RET_IF(devbuf_alloc(ones, (size_t)kmax));
            HIP_CHECK_RET(hipMemcpyAsync(ones.p, ones_h.data(), (size_t)kmax * sizeof(float), hipMemcpyHostToDevice, st));
            int rc = PAELLA_OK;
            for (const LnWeight& l : todo) {
                rc = devbuf_alloc(l.t->wsum, (size_t)l.N);
                if (rc != PAELLA_OK) break;
                GemmArgs g = gemm_args(ones.p, l.K, l.t->w.p, l.K, l.t->wsum.p, l.N, 1, l.N, l.K);
                rc = launch_gemm_cfg(g, 5, 1, nullptr, 0, st);  // explicit fp32 tile, one tile per workgroup (no workspace needed)
                if (rc != PAELLA_OK) break;
            }
            if (hipStreamSynchronize(st) != hipSuccess && rc == PAELLA_OK) { paella_set_error("finalize: stream error while summing weight rows"); rc = PAELLA_ERR_HIP; }
            (void)hipFree(ones.p);
            if (rc != PAELLA_OK) return rc;
        }
    }
    // Compose the conditioning projections (reference src/modules.py:72-77: kv = kv_mapper(c_embed), then nn.MultiheadAttention's K / V in-projection
    // of those rows): K|V = (silu(c) . Wkv^T + bkv) . Win[c:3c]^T + bin[c:3c] = silu(c) . (Win[c:3c] . Wkv)^T + (Win[c:3c] . bkv + bin[c:3c]).
    // One [kv_total, c_cond] matrix for all AttnBlocks turns 2 x n_attn tiny GEMMs per sample() call (8 rows at batch 1: 48 launches, 0.57 ms per
    // image) into ONE weight-streaming launch; equal to the two-stage form up to fp32 rounding of the composed weights.
    if (m->n_attn > 0) {
        hipStream_t st = (hipStream_t)stream;
        const int cc = m->cfg.c_cond;
        m->kv_col.assign(m->n_attn, 0);
        int total = 0;
        for (int i = 0; i < m->n_attn; ++i) { m->kv_col[i] = total; total += 2 * m->attn_c[i]; }
        m->kv_total = total;
        RET_IF(devbuf_alloc(m->kv_w, (size_t)total * cc));
        RET_IF(devbuf_alloc(m->kv_b, (size_t)total));
        DevBuf wkv_t;
        RET_IF(devbuf_alloc(wkv_t, (size_t)cc * m->c_max));
        int rc = PAELLA_OK;  // (both launches below run one whole tile per workgroup: no split-K workspace, nothing to allocate per reload -- ADVICE r03)
        auto compose = [&](const Block& b) -> int {
            if (b.type != BT_ATTN) return PAELLA_OK;
            const int ch = b.c;
            const float* win = b.in_w->w.p + (size_t)ch * ch;  // rows c .. 3c
            const float* bin = b.in_b->w.p + ch;
            const int64_t shp[2] = {ch, cc};
            const int perm[2] = {1, 0};
            RET_IF(launch_permute(b.kv_w->w.p, wkv_t.p, shp, perm, 2, st));  // [ch, cc] -> [cc, ch]
            // kv_w rows [col, col + 2ch): C[2ch, cc] = Win[c:3c] [2ch, ch] . (Wkv^T [cc, ch])^T
            GemmArgs g = gemm_args(win, ch, wkv_t.p, ch, m->kv_w.p + (size_t)m->kv_col[b.attn_index] * cc, cc, 2 * ch, cc, ch);
            RET_IF(launch_gemm_cfg(g, 18, 1, nullptr, 0, st));  // (explicit fp32 tile: never the bf16 fast mode)
            // kv_b: C[1, 2ch] = bkv [1, ch] . Win[c:3c]^T + bin[c:3c]
            GemmArgs gb = gemm_args(b.kv_b->w.p, ch, win, ch, m->kv_b.p + m->kv_col[b.attn_index], 2 * ch, 1, 2 * ch, ch);
            gb.ep.bias = bin;
            RET_IF(launch_gemm_cfg(gb, 5, 1, nullptr, 0, st));
            return PAELLA_OK;
        };
        if (rc == PAELLA_OK) for (const Block& b : m->down) { rc = compose(b); if (rc != PAELLA_OK) break; }
        if (rc == PAELLA_OK) for (const Block& b : m->up) { rc = compose(b); if (rc != PAELLA_OK) break; }
        if (hipStreamSynchronize(st) != hipSuccess && rc == PAELLA_OK) { paella_set_error("finalize: stream error while composing the conditioning projections"); rc = PAELLA_ERR_HIP; }
        if (wkv_t.p) (void)hipFree(wkv_t.p);
        if (rc != PAELLA_OK) return rc;
    }
    if (!m->freqs_set) {
        const int half = m->cfg.c_r / 2;
        std::vector<float> f(half > 0 ? half : 1);
        const float e = logf(10000.0f) / (float)(half - 1);
        for (int k = 0; k < half; ++k) f[k] = expf((float)k * -e);
        RET_IF(paella_unet_set_timestep_freqs(m, f.data(), half));
    }
    m->finalized = true;
    if (m->precision == 1) RET_IF(make_shadows(m, (hipStream_t)stream));  // (a reload refreshes the shadows)
    return PAELLA_OK;
}

// ---------------------------------------------------------------------------
// conditioning cache layout: ONE row-major matrix [B*S, kv_total]; AttnBlock i (execution order) owns columns [kv_col[i], +2*c_i) = (K | V)
// (a block-major layout -- one contiguous [B*S, 2c] matrix per AttnBlock -- was tried in round 4: no effect on the attention launch, profiles/r04_attention_launch_ab.txt)
// ---------------------------------------------------------------------------
extern "C" size_t paella_unet_cond_bytes(const paella_unet* m, int B, int S) {
    if (!m) return 0;
    const size_t n = (size_t)B * S * (size_t)m->kv_total;
    return (n ? n : 64) * sizeof(float);
}

struct FwdBuffers {
    float* xl[PAELLA_MAX_LEVELS];
    float* xu[PAELLA_MAX_LEVELS];
    float *h, *g, *grn_scale, *grn_gx, *ts, *remb, *splitk, *rowstat;
    unsigned short *h16, *g16, *x16;  // bf16 fast mode: the A operands of the bf16 GEMMs (same roles as h, g; x16 = bf16 copy of the current residual stream for LayerNorm-folding consumers)
    // cond_prepare
    float *c_embed, *c_silu;
};

static int64_t level_rows(const paella_unet* m, int B, int H, int W, int l) {
    const int p = m->cfg.patch_size;
    return (int64_t)B * ((H / p) >> l) * ((W / p) >> l);
}

static void carve_forward(const paella_unet* m, Arena& a, int B, int H, int W, int S, FwdBuffers& f) {
    const paella_unet_config& c = m->cfg;
    const int p2 = c.patch_size * c.patch_size;
    f.splitk = a.take(kSplitKBudget / sizeof(float));  // FIRST: its ticket header sits at a fixed offset (paella_workspace_init)
    size_t hmax = (size_t)B * H * W * c.c_out;
    size_t gmax = (size_t)B * H * W * c.c_out;
    {   // the fused head + tail parks one (score, label) per row and column tile in f.g: [rows, tiles_n] x 2 with tiles of >= 64 labels
        const size_t part = (size_t)B * H * W * 2 * (((size_t)c.num_labels + 63) / 64);
        if (part > gmax) gmax = part;
    }
    const size_t emb = (size_t)level_rows(m, B, H, W, 0) * c.c_in * p2;
    if (emb > hmax) hmax = emb;
    for (int l = 0; l < c.n_levels; ++l) {
        const size_t n = (size_t)level_rows(m, B, H, W, l) * c.c_hidden[l];
        f.xl[l] = a.take(n);
        f.xu[l] = (l < c.n_levels - 1) ? a.take(n) : nullptr;
        if (n > hmax) hmax = n;
        if (4 * n > gmax) gmax = 4 * n;
    }
    f.h = a.take(hmax);
    f.g = a.take(gmax);
    f.grn_scale = a.take((size_t)B * 4 * m->c_max);
    {   // also holds the GEMM epilogue's per-16-row sum-of-squares partials: [rows/16, 4c] <= gmax/16
        const size_t a1 = (size_t)B * 4 * m->c_max, a2 = gmax / 16 + 64;
        f.grn_gx = a.take(a1 > a2 ? a1 : a2);
    }
    f.ts = a.take((size_t)B * (m->ts_total > 0 ? m->ts_total : 1));
    f.remb = a.take((size_t)B * c.c_r);
    f.rowstat = a.take(hmax / 8 + 64);  // [rows, C/16, 2]
    f.h16 = f.g16 = f.x16 = nullptr;
    if (m->precision == 1) {  // (after everything else: the fp32 layout does not move)
        f.h16 = reinterpret_cast<unsigned short*>(a.take(hmax / 2 + 64));
        f.g16 = reinterpret_cast<unsigned short*>(a.take(gmax / 2 + 64));
        f.x16 = reinterpret_cast<unsigned short*>(a.take(hmax / 2 + 64));
    }
    (void)S;
}

static void carve_cond(const paella_unet* m, Arena& a, int B, int S, FwdBuffers& f) {
    f.splitk = a.take(kSplitKBudget / sizeof(float));  // FIRST, as in carve_forward
    f.c_embed = a.take((size_t)B * S * m->cfg.c_cond);
    f.c_silu = a.take((size_t)B * S * m->cfg.c_cond);
}

extern "C" size_t paella_unet_workspace_bytes(const paella_unet* m, int B, int H, int W, int S) {
    if (!m) return 0;
    FwdBuffers f;
    Arena a(nullptr, 0);
    carve_forward(m, a, B, H, W, S, f);
    Arena c(nullptr, 0);
    carve_cond(m, c, B, S, f);
    return (a.off > c.off ? a.off : c.off) + 256;
}

// gen_c_embeddings (reference src/modules.py:223-232; list-valued clip_image utils/modules.py:229-235):
// seq = cat([byt5_mapper(byt5), clip_mapper(clip).view(B,-1,c_cond), clip_image_mapper(ci).view(...)...], dim=1); seq_norm
static int compute_c_embed(const paella_unet* m, const float* byt5, int S_byt5, const float* clip, const float* const* clip_image,
                           int n_clip_image, int B, int S, float* c_embed, float* splitk, hipStream_t st) {
    const paella_unet_config& c = m->cfg;
    const size_t skb = kSplitKBudget;
    const int cc = c.c_cond;
    if (S_byt5 > 0) {
        GemmArgs g = gemm_args(byt5, c.byt5_embd, m->byt5_w->w.p, c.byt5_embd, c_embed, cc, B * S_byt5, cc, c.byt5_embd);
        g.ep.bias = m->byt5_b->w.p;
        g.ep.remap_in = S_byt5; g.ep.remap_out = S; g.ep.remap_off = 0;
        RET_IF(launch_gemm(g, splitk, skb, st));
    }
    int row_off = S_byt5;
    if (clip) {
        GemmArgs g = gemm_args(clip, c.clip_embd, m->clip_w->w.p, c.clip_embd, c_embed + (size_t)row_off * cc, S * cc, B,
                               cc * c.clip_seq_len, c.clip_embd);
        g.ep.bias = m->clip_b->w.p;
        RET_IF(launch_gemm(g, splitk, skb, st));
        row_off += c.clip_seq_len;
    }
    for (int i = 0; i < n_clip_image; ++i) {
        if (!clip_image || !clip_image[i]) { paella_set_error("clip_image[%d] is null", i); return PAELLA_ERR_ARG; }
        GemmArgs g = gemm_args(clip_image[i], c.clip_embd, m->clip_image_w->w.p, c.clip_embd,
                               c_embed + (size_t)row_off * cc, S * cc, B, cc * c.clip_seq_len, c.clip_embd);
        g.ep.bias = m->clip_image_b->w.p;
        RET_IF(launch_gemm(g, splitk, skb, st));
        row_off += c.clip_seq_len;
    }
    RET_IF(launch_layernorm(c_embed, c_embed, (int64_t)B * S, cc, 1e-6f, 1.f, 0.f, 0, 0, 0, st));
    return PAELLA_OK;
}

extern "C" int paella_unet_c_embeddings(paella_unet* m, const float* byt5, int S_byt5, const float* clip,
                                        const float* const* clip_image, int n_clip_image, int B, float* c_embed_out, void* ws,
                                        size_t ws_bytes, void* stream) {
    if (!m || !m->finalized) { paella_set_error("model not finalized"); return PAELLA_ERR_STATE; }
    const int S = S_byt5 + (clip ? m->cfg.clip_seq_len : 0) + n_clip_image * m->cfg.clip_seq_len;
    if (B <= 0 || S <= 0 || !c_embed_out) { paella_set_error("bad conditioning shape"); return PAELLA_ERR_ARG; }
    if (ws_bytes < kSplitKBudget || !ws) { paella_set_error("workspace too small"); return PAELLA_ERR_WORKSPACE; }
    return compute_c_embed(m, byt5, S_byt5, clip, clip_image, n_clip_image, B, S, c_embed_out, (float*)ws, (hipStream_t)stream);
}

extern "C" int paella_unet_r_embedding(paella_unet* m, const float* r, int B, float max_positions, float* r_embed_out, void* stream) {
    if (!m || !m->finalized) { paella_set_error("model not finalized"); return PAELLA_ERR_STATE; }
    if (!r || !r_embed_out) { paella_set_error("null argument"); return PAELLA_ERR_ARG; }
    return launch_timestep(r, m->freqs.p, m->ts_w.p, m->ts_b.p, nullptr, B, m->cfg.c_r, 0, max_positions, r_embed_out, 1, (hipStream_t)stream);
}

// S_slot > 0: the slot form -- the B samples' S rows go to the front of slots slot0 .. slot0 + B - 1 (S_slot >= S rows each) of a larger cache through the
// epilogue's row remap; the GEMM itself is the plain call's, so the stored rows are the plain call's bit for bit and no other byte of the cache is written
static int cond_prepare_impl(paella_unet* m, const float* byt5, int S_byt5, const float* clip, const float* const* clip_image, int n_clip_image, int B,
                             int S_slot, int slot0, void* cond_out, size_t cond_bytes, int* cond_len, void* ws, size_t ws_bytes, void* stream) {
    if (!m || !m->finalized) { paella_set_error("model not finalized"); return PAELLA_ERR_STATE; }
    hipStream_t st = (hipStream_t)stream;
    const paella_unet_config& c = m->cfg;
    const int S = S_byt5 + (clip ? c.clip_seq_len : 0) + n_clip_image * c.clip_seq_len;
    if (B <= 0 || S_byt5 < 0 || n_clip_image < 0) { paella_set_error("bad conditioning shape"); return PAELLA_ERR_ARG; }
    const bool slots = S_slot > 0;
    if (slots && (slot0 < 0 || S > S_slot || !cond_len)) {
        paella_set_error("cond_prepare_slots: %d conditioning rows do not fit a slot of %d rows (or slot0 < 0 / cond_len is null)", S, S_slot);
        return PAELLA_ERR_ARG;
    }
    if (S <= 0 && (slots || m->n_attn > 0)) { paella_set_error("conditioning sequence is empty"); return PAELLA_ERR_ARG; }
    if (slots) HIP_CHECK_RET(hipMemsetD32Async((hipDeviceptr_t)(cond_len + slot0), S, (size_t)B, st));
    if (m->n_attn == 0) return PAELLA_OK;
    if (S_byt5 > 0 && !byt5) { paella_set_error("byt5 is null"); return PAELLA_ERR_ARG; }
    const size_t need = slots ? (size_t)(slot0 + B) * S_slot * (size_t)m->kv_total * sizeof(float) : paella_unet_cond_bytes(m, B, S);
    if (cond_bytes < need || !cond_out) { paella_set_error("cond buffer too small"); return PAELLA_ERR_WORKSPACE; }
    FwdBuffers f;
    Arena a(ws, ws_bytes);
    carve_cond(m, a, B, S, f);
    if (!a.ok || !ws) { paella_set_error("workspace too small (%zu needed)", a.off); return PAELLA_ERR_WORKSPACE; }
    const size_t skb = kSplitKBudget;

    const int cc = c.c_cond;
    RET_IF(compute_c_embed(m, byt5, S_byt5, clip, clip_image, n_clip_image, B, S, f.c_embed, f.splitk, st));
    RET_IF(launch_silu(f.c_embed, f.c_silu, (int64_t)B * S * cc, st));

    // every AttnBlock's kv = kv_mapper(c_embed) (src/modules.py:77) and K|V in-projection of those rows in ONE GEMM over the composed weights
    GemmArgs g = gemm_args(f.c_silu, cc, m->kv_w.p, cc, (float*)cond_out, m->kv_total, B * S, m->kv_total, cc);
    g.ep.bias = m->kv_b.p;
    if (slots) { g.ep.remap_in = S; g.ep.remap_out = S_slot; g.ep.remap_off = slot0 * S_slot; }
    RET_IF(launch_gemm(g, f.splitk, skb, st));
    return PAELLA_OK;
}

extern "C" int paella_unet_cond_prepare(paella_unet* m, const float* byt5, int S_byt5, const float* clip,
                                        const float* const* clip_image, int n_clip_image, int B, void* cond_out,
                                        size_t cond_bytes, void* ws, size_t ws_bytes, void* stream) {
    return cond_prepare_impl(m, byt5, S_byt5, clip, clip_image, n_clip_image, B, 0, 0, cond_out, cond_bytes, nullptr, ws, ws_bytes, stream);
}

extern "C" int paella_unet_cond_prepare_slots(paella_unet* m, const float* byt5, int S_byt5, const float* clip, const float* const* clip_image,
                                              int n_clip_image, int B, int S_slot, int slot0, void* cache, size_t cache_bytes, int* cond_len, void* ws,
                                              size_t ws_bytes, void* stream) {
    if (S_slot <= 0) { paella_set_error("cond_prepare_slots: S_slot must be > 0"); return PAELLA_ERR_ARG; }
    return cond_prepare_impl(m, byt5, S_byt5, clip, clip_image, n_clip_image, B, S_slot, slot0, cache, cache_bytes, cond_len, ws, ws_bytes, stream);
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------
struct FwdCtx {
    const paella_unet* m;
    const paella_step_args& s;  // the block of this forward: grid, conditioning cache and per-request tables are read from it where they are used
    hipStream_t st;
    FwdBuffers f;
    int B;  // samples in flight: s.n_unique over the shared prefix of a guided step, s.B after it
};

// The A operand of a GEMM g that consumes LayerNorm(x), x = `rows` rows of C channels of the residual stream, for the weight wt (w16 = its bf16 shadow where this
// site may use it, else null).  from_stats: no launch -- the LayerNorm is folded into g's operand load from the producer's row statistics (fp32 x, or its bf16 copy
// x16, with the matching row sums of the weight).  Otherwise one LayerNorm launch into h16 (bf16 GEMM) or h (g.A as the caller built it); s2d = 1 gathers the
// 2x2 space-to-depth rows of an h x w grid on the way (down-sampler).
static int ln_operand(FwdCtx& cx, GemmArgs& g, const Weight* wt, const unsigned short* w16, bool from_stats, const float* x, int64_t rows, int C, int s2d = 0,
                      int h = 0, int w = 0) {
    if (from_stats) {
        g.A = x; g.ln_stats = cx.f.rowstat; g.ln_nblk = C / 16; g.ln_eps = 1e-6f; g.ln_wsum = wt->wsum.p;
        if (w16) { g.A16 = cx.f.x16; g.W16 = w16; g.ln_wsum = wt->wsum16.p; }
        return PAELLA_OK;
    }
    if (!w16) return launch_layernorm(x, cx.f.h, rows, C, 1e-6f, 1.f, 0.f, s2d, h, w, cx.st);
    g.A16 = cx.f.h16; g.W16 = w16;
    return launch_layernorm16(x, nullptr, cx.f.h16, rows, C, 1e-6f, 1.f, 0.f, s2d, h, w, cx.st);
}

// GEMM2 of an MLP block, x += A . W2^T + b2, with everything its epilogue carries: the bf16 copy of x and the row statistics for a LayerNorm-folding consumer, the
// fused TimestepBlock.  The A-operand side (GRN prologue / bf16 operands) is the caller's.
static GemmArgs mlp_gemm2(FwdCtx& cx, const Block& b, const float* A, float* x, int64_t rows, int rps) {
    const int ch = b.c;
    GemmArgs g2 = gemm_args(A, 4 * ch, b.w2->w.p, 4 * ch, x, ch, (int)rows, ch, 4 * ch);
    g2.ep.bias = b.b2->w.p;
    g2.ep.residual = x; g2.ep.ldr = ch;
    if (cx.m->precision == 1 && b.emit_rowstat) g2.ep.c16 = cx.f.x16;  // (also where the block itself is not eligible for the bf16 GEMMs: the consumer may still be)
    if (b.emit_rowstat) g2.ep.rowstat_out = cx.f.rowstat;
    if (b.fused_ts >= 0) {
        g2.ep.ts = cx.f.ts + b.fused_ts; g2.ep.ts_stride = cx.m->ts_total; g2.ep.rows_per_sample = rps;
    }
    return g2;
}

// ResBlock / FeedForwardBlock (reference src/modules.py:43-62, 82-96); x is updated in place
static int run_mlp_block(FwdCtx& cx, const Block& b, float* x, const float* skip, int h, int w) {
    const paella_unet* m = cx.m;
    const int ch = b.c;
    const int64_t rows = (int64_t)cx.B * h * w;
    const int rps = h * w;
    const float *gamma = b.gamma->w.p, *beta = b.beta->w.p;
    const unsigned short* const w1_16 = W16(m, b.w1);
    const unsigned short* const w2_16 = W16(m, b.w2);
    // OPT-IN bf16 fast mode: depthwise conv + LayerNorm -> bf16 | GEMM1 (bf16 operands) -> GELU -> bf16 hidden + GRN statistics | GRN apply in place on the
    // bf16 hidden tensor | GEMM2 (bf16 operands) -> fp32 residual stream.  The 4c-wide hidden tensor never exists in fp32.
    const bool fast = w1_16 && w2_16 && (ch % 64) == 0 && (rps % 16) == 0;
    GemmArgs g1 = gemm_args(fast ? nullptr : cx.f.h, ch, b.w1->w.p, ch, fast ? nullptr : cx.f.g, 4 * ch, (int)rows, 4 * ch, ch);
    if (b.type == BT_RES) {
        RET_IF(launch_dwconv_ln(x, skip, b.dw_w->w.p, b.dw_b->w.p, fast ? nullptr : cx.f.h, cx.B, h, w, ch, 1e-6f, cx.st, fast ? cx.f.h16 : nullptr));
        if (fast) { g1.A16 = cx.f.h16; g1.W16 = w1_16; }
    } else {
        RET_IF(ln_operand(cx, g1, b.w1, fast ? w1_16 : nullptr, false, x, rows, ch));
    }
    g1.ep.bias = b.b1->w.p;
    g1.ep.act = ACT_GELU;
    if (fast) {
        g1.ep.c16 = cx.f.g16;
        g1.ep.sumsq_out = cx.f.grn_gx;
        RET_IF(launch_gemm(g1, cx.f.splitk, kSplitKBudget, cx.st));
        RET_IF(launch_grn_partials_apply16(cx.f.grn_gx, gamma, beta, cx.f.grn_scale, cx.f.g16, cx.B, rps, 4 * ch, cx.st));
        GemmArgs g2 = mlp_gemm2(cx, b, nullptr, x, rows, rps);
        g2.A16 = cx.f.g16; g2.W16 = w2_16;
        return launch_gemm(g2, cx.f.splitk, kSplitKBudget, cx.st);
    }
    const int fused_tile = (rps % 16 == 0 && m->precision == 0) ? gemm_grn_fused_tile((int)rows, 4 * ch, ch, rps, false) : 0;
    if (fused_tile) {
        // GlobalResponseNorm with NO launch of its own (batch-1 regime): GEMM1's tiles cover whole samples, so its epilogue finishes
        // Gx[b][k] = ||g[b, :, k]||_2 and leaves per-column-tile sums of Gx; GEMM2 derives mean_k Gx from those and applies
        // g * (1 + gamma * Gx / (mean + 1e-6)) + beta to its operand fragments (reference src/modules.py:36-40)
        const int np = (4 * ch / 32) * 2;  // (column tiles of 32) x (2 wave columns)
        g1.ep.grn_gx_out = cx.f.grn_scale; g1.ep.grn_part_out = cx.f.grn_gx; g1.ep.grn_rps = rps; g1.ep.grn_np = np;
        g1.force_ring_cfg = fused_tile;
        RET_IF(launch_gemm(g1, cx.f.splitk, kSplitKBudget, cx.st));
        GemmArgs g2 = mlp_gemm2(cx, b, cx.f.g, x, rows, rps);
        g2.grn_gx = cx.f.grn_scale; g2.grn_part = cx.f.grn_gx; g2.grn_np = np; g2.grn_gamma = gamma;
        g2.a_shift = beta;
        g2.a_rows_per_sample = rps;
        return launch_gemm(g2, cx.f.splitk, kSplitKBudget, cx.st);
    }
    if (rps % 16 == 0) {
        // GRN statistics ride on GEMM1's epilogue (per-16-row column sums of squares), then one tiny finalize launch
        g1.ep.sumsq_out = cx.f.grn_gx;
        RET_IF(launch_gemm(g1, cx.f.splitk, kSplitKBudget, cx.st));
        RET_IF(launch_grn_from_partials(cx.f.grn_gx, gamma, cx.f.grn_scale, cx.B, rps / 16, 4 * ch, cx.st));
    } else {
        RET_IF(launch_gemm(g1, cx.f.splitk, kSplitKBudget, cx.st));
        RET_IF(launch_grn_scale(cx.f.g, gamma, cx.f.grn_scale, cx.f.grn_gx, cx.B, rps, 4 * ch, cx.st));
    }
    GemmArgs g2 = mlp_gemm2(cx, b, cx.f.g, x, rows, rps);
    g2.a_scale = cx.f.grn_scale;
    g2.a_shift = beta;
    g2.a_rows_per_sample = rps;
    return launch_gemm(g2, cx.f.splitk, kSplitKBudget, cx.st);
}

// AttnBlock (reference src/modules.py:65-79)
static int run_attn_block(FwdCtx& cx, const Block& b, float* x, int h, int w) {
    const paella_unet* m = cx.m;
    const paella_step_args& s = cx.s;
    const int ch = b.c;
    const int64_t rows = (int64_t)cx.B * h * w;
    const int nh = m->cfg.nhead[b.level];
    const bool self = m->cfg.self_attn != 0;
    const int nq = self ? 3 * ch : ch;
    GemmArgs gq = gemm_args(cx.f.h, ch, b.in_w->w.p, ch, cx.f.g, nq, (int)rows, nq, ch);
    // opt-in bf16 fast mode: both projections on bf16 operands (bf16 copy of the residual stream / bf16 LayerNorm output in, bf16 attention output in); q, k, v and
    // the attention itself stay fp32
    const unsigned short* const wq16 = (ch % 64) == 0 ? W16(m, b.in_w) : nullptr;
    const unsigned short* const wo16 = (ch % 64) == 0 ? W16(m, b.out_w) : nullptr;
    RET_IF(ln_operand(cx, gq, b.in_w, wq16, b.ln_from_stats, x, rows, ch));
    gq.ep.bias = b.in_b->w.p;
    // bf16 fast mode at >= 256 queries: q / k / v leave the in-projection as bf16 only and the attention core runs on bf16 MFMA (attention_bf16_kernel)
    const bool attn16 = wq16 && wo16 && h * w >= 256 && (nq % 8) == 0 && ((ch / nh) % 16) == 0 && ch / nh >= 32;
    if (attn16) { gq.C = nullptr; gq.ep.c16 = cx.f.g16; }
    RET_IF(launch_gemm(gq, cx.f.splitk, kSplitKBudget, cx.st));
    const float* kv = (const float*)s.cond + m->kv_col[b.attn_index];
    AttnArgs a;
    a.q = cx.f.g; a.ldq = nq;
    a.k_self = self ? cx.f.g + ch : nullptr; a.v_self = self ? cx.f.g + 2 * ch : nullptr; a.ld_self = nq;
    a.k_cond = kv; a.v_cond = kv + ch; a.ld_cond = m->kv_total;
    a.out = cx.f.h; a.ldo = ch;
    a.B = cx.B; a.nhead = nh; a.D = ch / nh; a.Lq = h * w; a.Lself = self ? h * w : 0; a.Lcond = s.S;
    a.scale = 1.0f / sqrtf((float)(ch / nh));
    a.key_weights = s.attn_weights; a.n_kw = s.attn_weights ? s.n_attn_weights : 0;
    a.out16 = wo16 ? cx.f.h16 : nullptr;
    a.q16 = nullptr; a.k_self16 = nullptr; a.v_self16 = nullptr; a.ld16 = 0;
    a.cond_len = s.cond_len;  // ragged conditioning: conditioning rows per sample, S then being the slot pitch
    if (s.kw_len) { a.kw_table = s.kw_table; a.kw_len = s.kw_len; a.kw_pitch = s.kw_pitch; }  // per-slot key weights instead of attn_weights
    if (s.q_groups) {  // per-query key groups: this level's queries sit at off = sum over the finer levels of their query counts inside a row of the table
        const int p = m->cfg.patch_size;
        int off = 0;
        for (int l = 0; l < b.level; ++l) off += ((s.H / p) >> l) * ((s.W / p) >> l);
        a.q_groups = s.q_groups + off; a.qg_pitch = s.qg_pitch;
        a.k_groups = s.k_groups; a.kg_pitch = s.S;
    }
    if (attn16) {
        a.q16 = cx.f.g16; a.ld16 = nq;
        a.k_self16 = self ? cx.f.g16 + ch : nullptr; a.v_self16 = self ? cx.f.g16 + 2 * ch : nullptr;
    }
    RET_IF(launch_attention(a, cx.st));
    GemmArgs go = gemm_args(cx.f.h, ch, b.out_w->w.p, ch, x, ch, (int)rows, ch, ch);
    if (wo16) { go.A16 = cx.f.h16; go.W16 = wo16; }
    go.ep.bias = b.out_b->w.p;
    go.ep.residual = x; go.ep.ldr = ch;
    if (m->precision == 1 && b.emit_rowstat) go.ep.c16 = cx.f.x16;
    if (b.emit_rowstat) go.ep.rowstat_out = cx.f.rowstat;
    return launch_gemm(go, cx.f.splitk, kSplitKBudget, cx.st);
}

extern "C" int paella_unet_forward(paella_unet* m, const int64_t* tokens, const float* r, const void* cond, int B, int H, int W,
                                   int S, const float* attn_weights, int n_attn_weights, float* logits_out, void* ws,
                                   size_t ws_bytes, void* stream) {
    return paella_unet_forward_shared(m, tokens, r, cond, B, B, 0.f, 0.f, H, W, S, attn_weights, n_attn_weights, logits_out, ws, ws_bytes, stream);
}

// Classifier-free guidance evaluates the SAME tokens and timestep against two conditionings (reference src/utils.py:44-46).
// Everything before the first attention block never sees the conditioning, so with n_unique < B (tokens [n_unique,H,W] and
// r [n_unique] hold the distinct rows; batch rows b, b + n_unique, ... of `cond` share them) that prefix -- embedding,
// level-0 ResBlocks, the first down-sampler and ResBlock of level 1 -- is computed for the n_unique distinct rows only and
// replicated (activations, saved skips, LayerNorm statistics) where the paths diverge.
// The guidance mix l = mix_c * l_cond + mix_u * l_uncond (src/utils.py:47) can ride through the bias-free linear head
// (out_mapper, src/modules.py:184-187): with (mix_c, mix_u) != (0, 0) and B == 2 * n_unique the head runs once on
// mix_c * LN(z_cond) + mix_u * LN(z_uncond) and logits_out receives the n_unique MIXED rows (half the head FLOPs and logits bytes).
// `tail` != nullptr: the head GEMM runs with the fused sampling-tail epilogue (no logits are stored; tail->tokens_out receives
// the sampled tokens of the B (or, with the guidance mix, n_unique) output rows); logits_out is then unused.
// Per-request prompt weights (s.kw_table / kw_len / kw_pitch): one row of post-softmax key multipliers per conditioning SLOT of the launch (B rows: a guided step's
// two halves carry independent rows) instead of the one attn_weights vector.  kw_len == nullptr = no table.
// Regional prompts (s.q_groups / k_groups): per-query key groups for every attention block of a forward.  q [nb, qg_pitch] holds one row per conditioning slot of
// the launch with the queries of all levels, level-major (level l at offset sum_{j<l} (H/patch)(W/patch)/4^j); k [nb, kg_pitch] one mask per row of a slot.
// q_groups == nullptr = no tables.
static int unet_query_total(const paella_unet* m, int H, int W) {
    const int p = m->cfg.patch_size;
    int tot = 0;
    for (int l = 0; l < m->cfg.n_levels; ++l) tot += ((H / p) >> l) * ((W / p) >> l);
    return tot;
}
// validated BEFORE anything is enqueued (the model may be null here: the checks that need it come after the ones that do not)
static int rg_table_check(const char* who, const paella_unet* m, const paella_step_args& s) {
    if (!s.q_groups && !s.k_groups) return PAELLA_OK;
    if (!s.q_groups || !s.k_groups) { paella_set_error("%s: q_groups and k_groups must be given together (one key-group table without the other)", who); return PAELLA_ERR_ARG; }
    if (s.kg_pitch < s.S || s.qg_pitch < 1) { paella_set_error("%s: key-group pitches too small (kg_pitch %d < S %d, or qg_pitch %d < 1)", who, s.kg_pitch, s.S, s.qg_pitch); return PAELLA_ERR_ARG; }
    if (!m) { paella_set_error("%s: null model", who); return PAELLA_ERR_ARG; }
    if (m->precision == 1) { paella_set_error("%s: the key-group tables are not offered in the bf16 precision mode", who); return PAELLA_ERR_ARG; }
    const int p = m->cfg.patch_size, div = p << (m->cfg.n_levels - 1);
    if (s.H <= 0 || s.W <= 0 || s.H % div || s.W % div) { paella_set_error("%s: token grid %dx%d must be a positive multiple of %d", who, s.H, s.W, div); return PAELLA_ERR_ARG; }
    if (s.qg_pitch < unet_query_total(m, s.H, s.W)) {
        paella_set_error("%s: qg_pitch %d smaller than the %d queries of all levels of a %dx%d grid", who, s.qg_pitch, unet_query_total(m, s.H, s.W), s.H, s.W);
        return PAELLA_ERR_ARG;
    }
    return PAELLA_OK;
}

// One forward as its block s describes it (rules checked by run_step_block); tail = the converted tail block of a fused step (s.logits_out is then unused), or null.
static int unet_forward_impl(paella_unet* m, const paella_step_args& s, const TailArgs* tail, void* ws, size_t ws_bytes, void* stream) {
    if (!m || !m->finalized) { paella_set_error("model not finalized"); return PAELLA_ERR_STATE; }
    if (!s.tokens || !s.r || (!s.logits_out && !tail)) { paella_set_error("null argument"); return PAELLA_ERR_ARG; }
    const paella_unet_config& c = m->cfg;
    const int p = c.patch_size;
    const int div = p << (c.n_levels - 1);
    const int H = s.H, W = s.W, n_unique = s.n_unique;
    int B = s.B;
    if (B <= 0 || H <= 0 || W <= 0 || H % div || W % div) {
        paella_set_error("token grid %dx%d must be a positive multiple of %d", H, W, div);
        return PAELLA_ERR_ARG;
    }
    if (m->n_attn > 0 && (!s.cond || s.S <= 0)) { paella_set_error("conditioning cache missing"); return PAELLA_ERR_ARG; }
    FwdCtx cx = {m, s, (hipStream_t)stream, {}, B};
    Arena a(ws, ws_bytes);
    carve_forward(m, a, B, H, W, s.S, cx.f);
    if (!a.ok || !ws) { paella_set_error("workspace too small (%zu needed, %zu given)", a.off, ws_bytes); return PAELLA_ERR_WORKSPACE; }
    hipStream_t st = cx.st;
    FwdBuffers& f = cx.f;
    int split = -1;  // index in m->down of the first block that reads the conditioning
    for (size_t i = 0; i < m->down.size(); ++i)
        if (m->down[i].type == BT_ATTN) { split = (int)i; break; }
    if (n_unique <= 0 || n_unique > B || B % n_unique) { paella_set_error("n_unique must divide B"); return PAELLA_ERR_ARG; }
    const bool mix = s.mix_pairs || s.mix_c != 0.f || s.mix_u != 0.f;
    if (mix && B != 2 * n_unique) { paella_set_error("guidance mix needs B == 2 * n_unique"); return PAELLA_ERR_ARG; }
    const int Bfull = B;
    if (n_unique < B) {  // tokens / r hold the n_unique distinct rows: the prefix runs on them only
        if (split < 0) split = 0;  // no attention on the way down: replicate right after the embedding
        B = n_unique; cx.B = n_unique;
    }

    // timestep embedding + all TimestepBlock mappers
    if (m->ts_total > 0)
        RET_IF(launch_timestep(s.r, m->freqs.p, m->ts_w.p, m->ts_b.p, f.ts, B, c.c_r, m->ts_total, 10000.0f, f.remb, Bfull / B, st));

    // in_mapper + PixelUnshuffle + embedding conv + LayerNorm2d   (src/modules.py:126-134,271)
    const int h0 = H / p, w0 = W / p;
    const int64_t n0 = (int64_t)B * h0 * w0;
    RET_IF(launch_embed_ln_unshuffle(s.tokens, m->in_mapper->w.p, f.h, B, H, W, c.c_in, p, c.num_labels, 1e-6f, st));
    {
        GemmArgs g = gemm_args(f.h, c.c_in * p * p, m->embedding_w->w.p, c.c_in * p * p, f.g, c.c_hidden[0], (int)n0, c.c_hidden[0], c.c_in * p * p);
        g.ep.bias = m->embedding_b->w.p;
        RET_IF(launch_gemm(g, f.splitk, kSplitKBudget, st));
        RET_IF(launch_layernorm(f.g, f.xl[0], n0, c.c_hidden[0], 1e-6f, 1.f, 0.f, 0, 0, 0, st));
    }

    // ---- down ----
    float* x = f.xl[0];
    int h = h0, w = w0;
    for (size_t bi = 0; bi < m->down.size(); ++bi) {
        const Block& b = m->down[bi];
        if ((int)bi == split && B != Bfull) {
            // the paths diverge here: replicate the current activation, every saved skip and the LayerNorm statistics
            const int reps = Bfull / B;
            int lvl = 0;
            for (size_t j = 0; j < bi; ++j) if (m->down[j].type == BT_DOWN) lvl = m->down[j].level;
            for (int rep = 1; rep < reps; ++rep) {
                for (int l = 0; l <= lvl; ++l) {
                    const int64_t rows_l = (int64_t)B * (h0 >> l) * (w0 >> l);
                    const int cl = c.c_hidden[l];
                    RET_IF(launch_copy_rows(f.xl[l], cl, f.xl[l] + (size_t)rep * rows_l * cl, cl, rows_l, cl, st));
                }
                const int64_t rows_c = (int64_t)B * h * w;
                const int sc = c.c_hidden[lvl] / 16 * 2;
                if (f.rowstat && c.c_hidden[lvl] % 16 == 0)
                    RET_IF(launch_copy_rows(f.rowstat, sc, f.rowstat + (size_t)rep * rows_c * sc, sc, rows_c, sc, st));
                if (f.x16 && c.c_hidden[lvl] % 8 == 0) {  // bf16 fast mode: the bf16 copy of the current activation, as rows of c / 2 floats
                    const int c2 = c.c_hidden[lvl] / 2;
                    RET_IF(launch_copy_rows(reinterpret_cast<const float*>(f.x16), c2, reinterpret_cast<float*>(f.x16) + (size_t)rep * rows_c * c2, c2, rows_c, c2, st));
                }
            }
            B = Bfull; cx.B = Bfull;
        }
        switch (b.type) {
            case BT_DOWN: {  // LayerNorm2d + Conv2d(k2,s2): LN fused with the space-to-depth gather, then a GEMM
                const int64_t rows_in = (int64_t)B * h * w;
                const unsigned short* const w16 = ((4 * b.c_from) % 64) == 0 ? W16(m, b.conv_w) : nullptr;
                GemmArgs g = gemm_args(f.h, 4 * b.c_from, b.conv_w->w.p, 4 * b.c_from, f.xl[b.level], b.c_to, (int)(rows_in / 4), b.c_to, 4 * b.c_from);
                RET_IF(ln_operand(cx, g, b.conv_w, w16, false, x, rows_in, b.c_from, 1, h, w));
                h >>= 1; w >>= 1;
                g.ep.bias = b.conv_b->w.p;
                RET_IF(launch_gemm(g, f.splitk, kSplitKBudget, st));
                x = f.xl[b.level];
                break;
            }
            case BT_RES: case BT_FF: RET_IF(run_mlp_block(cx, b, x, nullptr, h, w)); break;
            case BT_ATTN: RET_IF(run_attn_block(cx, b, x, h, w)); break;
            case BT_TS:
                if (b.ts_standalone)
                    RET_IF(launch_scale_shift(x, f.ts + b.ts_offset, m->ts_total, (int64_t)B * h * w, h * w, b.c, st));
                break;
            default: break;
        }
    }
    if (B != Bfull) { paella_set_error("internal: shared prefix never diverged"); return PAELLA_ERR_STATE; }
    // ---- up ---- (x continues in place on the deepest level's buffer)
    for (const Block& b : m->up) {
        switch (b.type) {
            case BT_UP: {  // LayerNorm2d + ConvTranspose2d(k2,s2): GEMM with N = 4*c_to and a depth-to-space store
                const int64_t rows_in = (int64_t)B * h * w;
                float* dst = f.xu[b.level - 1];
                GemmArgs g = gemm_args(f.h, b.c_from, b.conv_w->w.p, b.c_from, dst, b.c_to, (int)rows_in, 4 * b.c_to, b.c_from);
                const unsigned short* const w16 = (b.c_from % 64) == 0 ? W16(m, b.conv_w) : nullptr;
                RET_IF(ln_operand(cx, g, b.conv_w, w16, b.ln_from_stats, x, rows_in, b.c_from));
                g.ep.bias = b.conv_b->w.p;
                g.ep.store_mode = STORE_D2S; g.ep.sH = h; g.ep.sW = w; g.ep.sC = b.c_to; g.ep.n_seg_x = 2;
                RET_IF(launch_gemm(g, f.splitk, kSplitKBudget, st));
                h <<= 1; w <<= 1;
                x = dst;
                break;
            }
            case BT_RES: case BT_FF: RET_IF(run_mlp_block(cx, b, x, b.has_skip ? f.xl[b.level] : nullptr, h, w)); break;
            case BT_ATTN: RET_IF(run_attn_block(cx, b, x, h, w)); break;
            case BT_TS:
                if (b.ts_standalone)
                    RET_IF(launch_scale_shift(x, f.ts + b.ts_offset, m->ts_total, (int64_t)B * h * w, h * w, b.c, st));
                break;
            default: break;
        }
    }
    // ---- clf + out_mapper (src/modules.py:179-187) ----
    {
        const int p2 = p * p;
        const int64_t n0 = (int64_t)B * h0 * w0;  // full batch again
        GemmArgs g = gemm_args(f.h, c.c_hidden[0], m->clf_w->w.p, c.c_hidden[0], f.g, c.c_out, (int)n0, c.c_out * p2, c.c_hidden[0]);
        const unsigned short* const wc16 = (c.c_hidden[0] % 64) == 0 ? W16(m, m->clf_w) : nullptr;
        RET_IF(ln_operand(cx, g, m->clf_w, wc16, m->clf_from_stats, x, n0, c.c_hidden[0]));
        g.ep.bias = m->clf_b->w.p;
        if (p == 2) { g.ep.store_mode = STORE_D2S; g.ep.sH = h0; g.ep.sW = w0; g.ep.sC = c.c_out; g.ep.n_seg_x = 2; }
        RET_IF(launch_gemm(g, f.splitk, kSplitKBudget, st));
        int64_t nt = (int64_t)B * H * W;
        const unsigned short* const wh16 = (c.c_out % 64) == 0 ? W16(m, m->out_mapper) : nullptr;  // bf16 fast mode: the head GEMM on bf16 operands
        if (wh16 && !mix) RET_IF(launch_layernorm16(f.g, nullptr, f.h16, nt, c.c_out, 1e-6f, 1.f, 0.f, 0, 0, 0, st));
        else RET_IF(launch_layernorm(f.g, f.h, nt, c.c_out, 1e-6f, 1.f, 0.f, 0, 0, 0, st));
        if (mix) {  // the head is linear and bias-free: mix its input instead of its output
            nt /= 2;
            if (s.mix_pairs) RET_IF(launch_axpby16_req(f.h, f.h + (size_t)nt * c.c_out, s.mix_pairs, n_unique, (int64_t)H * W * c.c_out, wh16 ? f.h16 : nullptr, st));
            else RET_IF(launch_axpby16(f.h, f.h + (size_t)nt * c.c_out, s.mix_c, s.mix_u, nt * c.c_out, wh16 ? f.h16 : nullptr, st));
        }
        GemmArgs go = gemm_args(f.h, c.c_out, m->out_mapper->w.p, c.c_out, tail ? nullptr : s.logits_out, c.num_labels, (int)nt, c.num_labels, c.c_out);
        if (wh16) { go.A16 = f.h16; go.W16 = wh16; }
        if (!tail) {
            // same tile config as the fused-tail launch below (one whole tile per workgroup, no K split): the two paths produce
            // bit-identical logits, hence identical tokens (also in the bf16 fast mode: both run the bf16 64x64 direct-to-LDS tile)
            RET_IF(launch_gemm_cfg(go, gemm_tail_config((int)nt, c.num_labels, wh16 != nullptr), 1, f.splitk, kSplitKBudget, st));
        } else {
            // out_mapper fused with the sampling tail (reference src/utils.py:44-50 materialises the logits; here they never leave
            // the registers): per row and column tile the best (score, label) lands in f.g (free after the LayerNorm above)
            const int tn = gemm_tail_tiles_n((int)nt, c.num_labels, wh16 != nullptr);
            if (tn > (c.num_labels + 63) / 64) { paella_set_error("internal: fused tail tiles narrower than 64 labels (tiles_n=%d)", tn); return PAELLA_ERR_STATE; }
            if (tail->rows != nt || tail->L != c.num_labels) { paella_set_error("fused tail: row / label count mismatch"); return PAELLA_ERR_ARG; }
            go.C = nullptr;
            go.ft.temperature = tail->temperature; go.ft.mode = tail->mode; go.ft.seed = tail->seed; go.ft.seed_ptr = tail->seed_ptr;
            go.ft.offset = tail->offset; go.ft.row_offset = tail->row_offset; go.ft.row_offset_ptr = tail->row_offset_ptr;
            go.rq = tail->rq;
            go.ft.part_score = f.g;
            go.ft.part_idx = reinterpret_cast<int*>(f.g + (size_t)nt * tn);
            RET_IF(launch_gemm_tail(go, st));
            RET_IF(launch_tail_finalize(*tail, go.ft.part_score, go.ft.part_idx, tn, st));
        }
    }
    return PAELLA_OK;
}

// ---------------------------------------------------------------------------
// The argument block of one forward (include/paella_hip.h: paella_step_args).  run_step_block is the one place where a block's rules are checked -- all before anything is
// enqueued, the model may still be null there -- and where it is handed to unet_forward_impl; a fused step's tail block goes through tail.hip: tail_block_convert.
// Every paella_unet_forward_shared* / _sample* entry point below fills a block, names itself and runs it; need (internal.h: kNeed*) = what its name promises beyond the block.
// ---------------------------------------------------------------------------
static int run_step_block(const char* who, paella_unet* m, const paella_step_args& s, int need, void* ws, size_t ws_bytes, void* stream) {
    if ((!s.tail && !s.logits_out) || ((need & kNeedPairs) && !s.mix_pairs)) { paella_set_error("%s: null argument (logits_out / mix_pairs)", who); return PAELLA_ERR_ARG; }
    if (s.mix_pairs && (s.mix_c != 0.f || s.mix_u != 0.f)) { paella_set_error("%s: a guidance pair table and a scalar mix exclude each other", who); return PAELLA_ERR_ARG; }
    if (s.kw_len && (!s.kw_table || s.kw_pitch < 1)) { paella_set_error("%s: kw_len needs kw_table and kw_pitch >= 1", who); return PAELLA_ERR_ARG; }
    if (s.kw_len && s.attn_weights) { paella_set_error("%s: one attn_weights vector and the key-weight table exclude each other", who); return PAELLA_ERR_ARG; }
    RET_IF(rg_table_check(who, m, s));
    TailArgs a;
    if (s.tail) {
        TailFilter f;
        TailStats st;
        int kind = 0;
        RET_IF(tail_block_convert(who, *s.tail, need, true, a, f, st, &kind));
        const bool mix = s.mix_pairs || s.mix_c != 0.f || s.mix_u != 0.f;
        if (!mix && s.n_unique != s.B) {
            paella_set_error("%s without a guidance mix needs n_unique == B (separate cond / uncond logits take the unfused path)", who);
            return PAELLA_ERR_ARG;
        }
        if (a.rq.rows_per_sample > 0 && (s.H <= 0 || s.W <= 0 || a.rq.rows_per_sample != s.H * s.W)) {
            paella_set_error("%s: rows_per_sample (%d) must equal H * W", who, a.rq.rows_per_sample);
            return PAELLA_ERR_ARG;
        }
        a.rows = (int64_t)(mix ? s.n_unique : s.B) * s.H * s.W;  // with the guidance mix the head emits the n_unique mixed rows
        a.L = m ? m->cfg.num_labels : 0;
    }
    return unet_forward_impl(m, s, s.tail ? &a : nullptr, ws, ws_bytes, stream);
}

extern "C" int paella_unet_step(paella_unet* m, const paella_step_args* args, size_t args_bytes, void* ws, size_t ws_bytes, void* stream) {
    if (args_bytes != sizeof(paella_step_args)) { paella_set_error("unet_step: args_bytes %zu is not this library's sizeof(paella_step_args) = %zu", args_bytes, sizeof(paella_step_args)); return PAELLA_ERR_ARG; }
    if (!args) { paella_set_error("unet_step: null argument"); return PAELLA_ERR_ARG; }
    return run_step_block("unet_step", m, *args, 0, ws, ws_bytes, stream);
}

// ---- the fixed-form entry points.  One that extends another IS that one when what it adds is absent: it then reports under the other's name.
// what every form takes; the guidance mix is (mix_c, mix_u) in the scalar forms and the pair table in the request forms
static paella_step_args step_block(const int64_t* tokens, const float* r, const void* cond, int B, int n_unique, float mix_c, float mix_u, const float* mix_pairs, int H,
                                   int W, int S, const int* cond_len, const float* attn_weights, int n_attn_weights) {
    paella_step_args s = {};
    s.tokens = tokens; s.r = r; s.cond = cond; s.B = B; s.n_unique = n_unique; s.mix_c = mix_c; s.mix_u = mix_u; s.mix_pairs = mix_pairs; s.H = H; s.W = W; s.S = S;
    s.cond_len = cond_len; s.attn_weights = attn_weights; s.n_attn_weights = n_attn_weights;
    return s;
}

// Ragged conditioning (ABI 8): `cond_len` right after S -- a DEVICE table [B] with the conditioning rows of each sample, S then being the slot pitch of `cond`
// (attention.hip: attn_cond_rows)
extern "C" int paella_unet_forward_shared_ragged(paella_unet* m, const int64_t* tokens, const float* r, const void* cond, int B, int n_unique,
                                                 float mix_c, float mix_u, int H, int W, int S, const int* cond_len, const float* attn_weights,
                                                 int n_attn_weights, float* logits_out, void* ws, size_t ws_bytes, void* stream) {
    paella_step_args s = step_block(tokens, r, cond, B, n_unique, mix_c, mix_u, nullptr, H, W, S, cond_len, attn_weights, n_attn_weights);
    s.logits_out = logits_out;
    return run_step_block("forward_shared", m, s, 0, ws, ws_bytes, stream);
}
extern "C" int paella_unet_forward_shared(paella_unet* m, const int64_t* tokens, const float* r, const void* cond, int B, int n_unique,
                                          float mix_c, float mix_u, int H, int W, int S, const float* attn_weights,
                                          int n_attn_weights, float* logits_out, void* ws, size_t ws_bytes, void* stream) {
    return paella_unet_forward_shared_ragged(m, tokens, r, cond, B, n_unique, mix_c, mix_u, H, W, S, nullptr, attn_weights, n_attn_weights, logits_out, ws, ws_bytes, stream);
}

// One whole sampling step for the counter-based noise mode: Paella.forward + the sampling tail (src/utils.py:43-54) with the head
// GEMM and the tail fused -- the [rows, num_labels] logits are never written.  Output rows: n_unique with the guidance mix
// (B == 2 * n_unique, (mix_c, mix_u) != (0, 0)), otherwise B (no guidance; n_unique must equal B).  The pin tables (common.h: TailArgs::pin_keep / pin_tokens) optional.
extern "C" int paella_unet_forward_sample_pin(paella_unet* m, const int64_t* tokens, const float* r, const void* cond, int B, int n_unique,
                                              float mix_c, float mix_u, int H, int W, int S, const int* cond_len, const float* attn_weights, int n_attn_weights,
                                              float temperature, int mode, uint64_t seed, const uint64_t* seed_ptr, uint64_t offset,
                                              int64_t row_offset, const int64_t* row_offset_ptr, const int64_t* init_noise, float t_next,
                                              const int64_t* pin_keep, const int64_t* pin_tokens, int64_t* tokens_out, void* ws, size_t ws_bytes, void* stream) {
    const paella_tail_args t = tail_block_scalar(nullptr, nullptr, 0, 0, 1.f, 0.f, temperature, mode, seed, seed_ptr, offset, row_offset, row_offset_ptr, init_noise, t_next,
                                                 pin_keep, pin_tokens, tokens_out, nullptr);
    paella_step_args s = step_block(tokens, r, cond, B, n_unique, mix_c, mix_u, nullptr, H, W, S, cond_len, attn_weights, n_attn_weights);
    s.tail = &t;
    return run_step_block("forward_sample", m, s, 0, ws, ws_bytes, stream);
}
extern "C" int paella_unet_forward_sample_ragged(paella_unet* m, const int64_t* tokens, const float* r, const void* cond, int B, int n_unique,
                                                 float mix_c, float mix_u, int H, int W, int S, const int* cond_len, const float* attn_weights, int n_attn_weights,
                                                 float temperature, int mode, uint64_t seed, const uint64_t* seed_ptr, uint64_t offset,
                                                 int64_t row_offset, const int64_t* row_offset_ptr, const int64_t* init_noise, float t_next,
                                                 int64_t* tokens_out, void* ws, size_t ws_bytes, void* stream) {
    return paella_unet_forward_sample_pin(m, tokens, r, cond, B, n_unique, mix_c, mix_u, H, W, S, cond_len, attn_weights, n_attn_weights, temperature, mode, seed, seed_ptr,
                                          offset, row_offset, row_offset_ptr, init_noise, t_next, nullptr, nullptr, tokens_out, ws, ws_bytes, stream);
}
extern "C" int paella_unet_forward_sample(paella_unet* m, const int64_t* tokens, const float* r, const void* cond, int B, int n_unique,
                                          float mix_c, float mix_u, int H, int W, int S, const float* attn_weights, int n_attn_weights,
                                          float temperature, int mode, uint64_t seed, const uint64_t* seed_ptr, uint64_t offset,
                                          int64_t row_offset, const int64_t* row_offset_ptr, const int64_t* init_noise, float t_next,
                                          int64_t* tokens_out, void* ws, size_t ws_bytes, void* stream) {
    return paella_unet_forward_sample_ragged(m, tokens, r, cond, B, n_unique, mix_c, mix_u, H, W, S, nullptr, attn_weights, n_attn_weights, temperature, mode, seed,
                                             seed_ptr, offset, row_offset, row_offset_ptr, init_noise, t_next, tokens_out, ws, ws_bytes, stream);
}

// Request batch (ABI 6): the logits forward with one guidance pair per sample (required here)
extern "C" int paella_unet_forward_shared_req_ragged(paella_unet* m, const int64_t* tokens, const float* r, const void* cond, int B, int n_unique,
                                                     const float* mix_pairs, int H, int W, int S, const int* cond_len, const float* attn_weights, int n_attn_weights,
                                                     float* logits_out, void* ws, size_t ws_bytes, void* stream) {
    paella_step_args s = step_block(tokens, r, cond, B, n_unique, 0.f, 0.f, mix_pairs, H, W, S, cond_len, attn_weights, n_attn_weights);
    s.logits_out = logits_out;
    return run_step_block("forward_shared_req", m, s, kNeedPairs, ws, ws_bytes, stream);
}
extern "C" int paella_unet_forward_shared_req(paella_unet* m, const int64_t* tokens, const float* r, const void* cond, int B, int n_unique,
                                              const float* mix_pairs, int H, int W, int S, const float* attn_weights, int n_attn_weights,
                                              float* logits_out, void* ws, size_t ws_bytes, void* stream) {
    return paella_unet_forward_shared_req_ragged(m, tokens, r, cond, B, n_unique, mix_pairs, H, W, S, nullptr, attn_weights, n_attn_weights, logits_out, ws, ws_bytes,
                                                 stream);
}
// Per-request prompt weights and regional prompts: the most general logits entry point -- the key-weight table in place of (attn_weights, n_attn_weights) and the
// key-group tables; mix_pairs may be NULL here (no guidance mix: the B rows of logits, n_unique dividing B as in paella_unet_forward_shared)
extern "C" int paella_unet_forward_shared_req_rg(paella_unet* m, const int64_t* tokens, const float* r, const void* cond, int B, int n_unique,
                                                 const float* mix_pairs, int H, int W, int S, const int* cond_len, const float* kw_table, const int* kw_len,
                                                 int kw_pitch, const int* q_groups, int qg_pitch, const int* k_groups, int kg_pitch, float* logits_out, void* ws,
                                                 size_t ws_bytes, void* stream) {
    paella_step_args s = step_block(tokens, r, cond, B, n_unique, 0.f, 0.f, mix_pairs, H, W, S, cond_len, nullptr, 0);
    s.kw_table = kw_table; s.kw_len = kw_len; s.kw_pitch = kw_pitch; s.q_groups = q_groups; s.qg_pitch = qg_pitch; s.k_groups = k_groups; s.kg_pitch = kg_pitch;
    s.logits_out = logits_out;
    return run_step_block(q_groups || k_groups ? "forward_shared_req_rg" : "forward_shared_req_kw", m, s, 0, ws, ws_bytes, stream);
}
extern "C" int paella_unet_forward_shared_req_kw(paella_unet* m, const int64_t* tokens, const float* r, const void* cond, int B, int n_unique,
                                                 const float* mix_pairs, int H, int W, int S, const int* cond_len, const float* kw_table, const int* kw_len,
                                                 int kw_pitch, float* logits_out, void* ws, size_t ws_bytes, void* stream) {
    return paella_unet_forward_shared_req_rg(m, tokens, r, cond, B, n_unique, mix_pairs, H, W, S, cond_len, kw_table, kw_len, kw_pitch, nullptr, 0, nullptr, 0, logits_out, ws,
                                             ws_bytes, stream);
}

// the request form of the fused step (the guidance pairs ride through the head: none left for the tail)
extern "C" int paella_unet_forward_sample_req_ragged(paella_unet* m, const int64_t* tokens, const float* r, const void* cond, int B, int n_unique,
                                                     const float* mix_pairs, int H, int W, int S, const int* cond_len, const float* attn_weights, int n_attn_weights,
                                                     const uint64_t* seeds, const float* temperature, int rows_per_sample, uint64_t offset,
                                                     const int64_t* init_noise, float t_next, int64_t* tokens_out, void* ws, size_t ws_bytes, void* stream) {
    paella_tail_args t = tail_block_stream(nullptr, nullptr, 0, 0, nullptr, temperature, seeds, rows_per_sample, nullptr, nullptr, nullptr, init_noise, nullptr, nullptr,
                                           nullptr, tokens_out, nullptr);
    t.offset = offset; t.t_next = t_next;
    paella_step_args s = step_block(tokens, r, cond, B, n_unique, 0.f, 0.f, mix_pairs, H, W, S, cond_len, attn_weights, n_attn_weights);
    s.tail = &t;
    return run_step_block("forward_sample_req", m, s, kNeedRequest, ws, ws_bytes, stream);
}
extern "C" int paella_unet_forward_sample_req(paella_unet* m, const int64_t* tokens, const float* r, const void* cond, int B, int n_unique,
                                              const float* mix_pairs, int H, int W, int S, const float* attn_weights, int n_attn_weights,
                                              const uint64_t* seeds, const float* temperature, int rows_per_sample, uint64_t offset,
                                              const int64_t* init_noise, float t_next, int64_t* tokens_out, void* ws, size_t ws_bytes, void* stream) {
    return paella_unet_forward_sample_req_ragged(m, tokens, r, cond, B, n_unique, mix_pairs, H, W, S, nullptr, attn_weights, n_attn_weights, seeds, temperature,
                                                 rows_per_sample, offset, init_noise, t_next, tokens_out, ws, ws_bytes, stream);
}
// Per-request prompt weights: the key-weight table in place of (attn_weights, n_attn_weights), plus the (nullable) pin tables of the sampling tail.
extern "C" int paella_unet_forward_sample_req_kw(paella_unet* m, const int64_t* tokens, const float* r, const void* cond, int B, int n_unique,
                                                 const float* mix_pairs, int H, int W, int S, const int* cond_len, const float* kw_table, const int* kw_len,
                                                 int kw_pitch, const uint64_t* seeds, const float* temperature, int rows_per_sample, uint64_t offset,
                                                 const int64_t* init_noise, float t_next, const int64_t* pin_keep, const int64_t* pin_tokens, const int* pin_on,
                                                 int64_t* tokens_out, void* ws, size_t ws_bytes, void* stream) {
    paella_tail_args t = tail_block_stream(nullptr, nullptr, 0, 0, nullptr, temperature, seeds, rows_per_sample, nullptr, nullptr, nullptr, init_noise, pin_keep, pin_tokens,
                                           pin_on, tokens_out, nullptr);
    t.offset = offset; t.t_next = t_next;
    paella_step_args s = step_block(tokens, r, cond, B, n_unique, 0.f, 0.f, mix_pairs, H, W, S, cond_len, nullptr, 0);
    s.kw_table = kw_table; s.kw_len = kw_len; s.kw_pitch = kw_pitch; s.tail = &t;
    return run_step_block("forward_sample_req_kw", m, s, kNeedRequest, ws, ws_bytes, stream);
}

// Request stream (ABI 7): the request form with the three per-request stream tables (common.h: ReqTables::step / t_next / active), all required here; the pin tables
// optional
extern "C" int paella_unet_forward_sample_stream_pin(paella_unet* m, const int64_t* tokens, const float* r, const void* cond, int B, int n_unique,
                                                     const float* mix_pairs, int H, int W, int S, const int* cond_len, const float* attn_weights,
                                                     int n_attn_weights, const uint64_t* seeds, const float* temperature, int rows_per_sample, const int* step,
                                                     const float* t_next, const int* active, const int64_t* init_noise, const int64_t* pin_keep,
                                                     const int64_t* pin_tokens, const int* pin_on, int64_t* tokens_out, void* ws, size_t ws_bytes, void* stream) {
    const paella_tail_args t = tail_block_stream(nullptr, nullptr, 0, 0, nullptr, temperature, seeds, rows_per_sample, step, t_next, active, init_noise, pin_keep,
                                                 pin_tokens, pin_on, tokens_out, nullptr);
    paella_step_args s = step_block(tokens, r, cond, B, n_unique, 0.f, 0.f, mix_pairs, H, W, S, cond_len, attn_weights, n_attn_weights);
    s.tail = &t;
    return run_step_block("forward_sample_stream", m, s, kNeedStream, ws, ws_bytes, stream);
}
extern "C" int paella_unet_forward_sample_stream_ragged(paella_unet* m, const int64_t* tokens, const float* r, const void* cond, int B, int n_unique,
                                                        const float* mix_pairs, int H, int W, int S, const int* cond_len, const float* attn_weights,
                                                        int n_attn_weights, const uint64_t* seeds, const float* temperature, int rows_per_sample, const int* step,
                                                        const float* t_next, const int* active, const int64_t* init_noise, int64_t* tokens_out, void* ws,
                                                        size_t ws_bytes, void* stream) {
    return paella_unet_forward_sample_stream_pin(m, tokens, r, cond, B, n_unique, mix_pairs, H, W, S, cond_len, attn_weights, n_attn_weights, seeds, temperature,
                                                 rows_per_sample, step, t_next, active, init_noise, nullptr, nullptr, nullptr, tokens_out, ws, ws_bytes, stream);
}
extern "C" int paella_unet_forward_sample_stream(paella_unet* m, const int64_t* tokens, const float* r, const void* cond, int B, int n_unique,
                                                 const float* mix_pairs, int H, int W, int S, const float* attn_weights, int n_attn_weights,
                                                 const uint64_t* seeds, const float* temperature, int rows_per_sample, const int* step,
                                                 const float* t_next, const int* active, const int64_t* init_noise, int64_t* tokens_out, void* ws,
                                                 size_t ws_bytes, void* stream) {
    return paella_unet_forward_sample_stream_ragged(m, tokens, r, cond, B, n_unique, mix_pairs, H, W, S, nullptr, attn_weights, n_attn_weights, seeds, temperature,
                                                    rows_per_sample, step, t_next, active, init_noise, tokens_out, ws, ws_bytes, stream);
}
// Per-request prompt weights and regional prompts: the most general tick of a stream -- the key-weight table in place of (attn_weights, n_attn_weights) and the
// key-group tables
extern "C" int paella_unet_forward_sample_stream_rg(paella_unet* m, const int64_t* tokens, const float* r, const void* cond, int B, int n_unique,
                                                    const float* mix_pairs, int H, int W, int S, const int* cond_len, const float* kw_table, const int* kw_len,
                                                    int kw_pitch, const int* q_groups, int qg_pitch, const int* k_groups, int kg_pitch, const uint64_t* seeds,
                                                    const float* temperature, int rows_per_sample, const int* step, const float* t_next, const int* active,
                                                    const int64_t* init_noise, const int64_t* pin_keep, const int64_t* pin_tokens, const int* pin_on,
                                                    int64_t* tokens_out, void* ws, size_t ws_bytes, void* stream) {
    const paella_tail_args t = tail_block_stream(nullptr, nullptr, 0, 0, nullptr, temperature, seeds, rows_per_sample, step, t_next, active, init_noise, pin_keep,
                                                 pin_tokens, pin_on, tokens_out, nullptr);
    paella_step_args s = step_block(tokens, r, cond, B, n_unique, 0.f, 0.f, mix_pairs, H, W, S, cond_len, nullptr, 0);
    s.kw_table = kw_table; s.kw_len = kw_len; s.kw_pitch = kw_pitch; s.q_groups = q_groups; s.qg_pitch = qg_pitch; s.k_groups = k_groups; s.kg_pitch = kg_pitch;
    s.tail = &t;
    return run_step_block(q_groups || k_groups ? "forward_sample_stream_rg" : "forward_sample_stream_kw", m, s, kNeedStream, ws, ws_bytes, stream);
}
extern "C" int paella_unet_forward_sample_stream_kw(paella_unet* m, const int64_t* tokens, const float* r, const void* cond, int B, int n_unique,
                                                    const float* mix_pairs, int H, int W, int S, const int* cond_len, const float* kw_table, const int* kw_len,
                                                    int kw_pitch, const uint64_t* seeds, const float* temperature, int rows_per_sample, const int* step,
                                                    const float* t_next, const int* active, const int64_t* init_noise, const int64_t* pin_keep,
                                                    const int64_t* pin_tokens, const int* pin_on, int64_t* tokens_out, void* ws, size_t ws_bytes, void* stream) {
    return paella_unet_forward_sample_stream_rg(m, tokens, r, cond, B, n_unique, mix_pairs, H, W, S, cond_len, kw_table, kw_len, kw_pitch, nullptr, 0, nullptr, 0, seeds,
                                                temperature, rows_per_sample, step, t_next, active, init_noise, pin_keep, pin_tokens, pin_on, tokens_out, ws, ws_bytes, stream);
}

extern "C" int paella_request_step(const float* program, int max_steps, int* pos, const int* len, int B, float* r, float* temperature, float* pairs,
                                   float* t_next, int* step, int* active, void* stream) {
    return launch_request_step(program, max_steps, pos, len, B, r, temperature, pairs, t_next, step, active, nullptr, nullptr, (hipStream_t)stream);
}
// paella_request_step for an editing stream: pin_policy int32 [B] (0 never, 1 every step, 2 final step only) -> pin_on int32 [B], this tick's flags
extern "C" int paella_request_step_pin(const float* program, int max_steps, int* pos, const int* len, int B, float* r, float* temperature, float* pairs,
                                       float* t_next, int* step, int* active, const int* pin_policy, int* pin_on, void* stream) {
    if (!!pin_policy != !!pin_on) { paella_set_error("request_step_pin: pin_policy and pin_on must be given together (a null output or a null policy table)"); return PAELLA_ERR_ARG; }
    return launch_request_step(program, max_steps, pos, len, B, r, temperature, pairs, t_next, step, active, pin_policy, pin_on, (hipStream_t)stream);
}

extern "C" int paella_start_tokens_req(const uint64_t* seeds, int B, int rows_per_sample, int num_labels, int64_t* tokens_out, void* stream) {
    return launch_start_tokens_req(seeds, B, rows_per_sample, num_labels, tokens_out, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------
// start tokens / add_noise / single-op entry points (the sampling tails: tail.hip)
// ---------------------------------------------------------------------------
extern "C" int paella_start_tokens(uint64_t seed, const uint64_t* seed_ptr, int64_t row_offset, const int64_t* row_offset_ptr, int num_labels,
                                   int64_t n, int64_t* tokens_out, void* stream) {
    return launch_start_tokens(seed, seed_ptr, row_offset, row_offset_ptr, num_labels, n, tokens_out, (hipStream_t)stream);
}

extern "C" int paella_add_noise(const int64_t* x, const float* t, const int64_t* mask_in, const int64_t* random_x, const float* rand_u,
                                uint64_t seed, uint64_t offset, int num_labels, int B, int64_t per_sample, int64_t* x_out,
                                int64_t* mask_out, void* stream) {
    if (!x || !x_out || (!mask_in && !t)) { paella_set_error("null argument"); return PAELLA_ERR_ARG; }
    return launch_add_noise(x, t, mask_in, random_x, rand_u, seed, offset, num_labels, B, per_sample, x_out, mask_out, (hipStream_t)stream);
}

extern "C" int paella_select_tokens(const int64_t* a, const int64_t* b, const int64_t* mask, const float* flag, int64_t fill, int64_t n, int64_t* out,
                                    void* stream) {
    if (n < 0) { paella_set_error("select_tokens: negative count"); return PAELLA_ERR_ARG; }
    return launch_select_tokens(a, b, mask, flag, fill, n, out, (hipStream_t)stream);
}

extern "C" int paella_op_gemm(const float* A, const float* W, const float* bias, const float* residual, float* C, int M, int N, int K,
                              int act, int tile_cfg, int splitk, void* ws, size_t ws_bytes, void* stream) {
    GemmArgs g = gemm_args(A, K, W, K, C, N, M, N, K);
    g.ep.bias = bias; g.ep.act = act; g.ep.residual = residual; g.ep.ldr = N;
    return launch_gemm_cfg(g, tile_cfg, splitk, ws, ws_bytes, (hipStream_t)stream);
}
// the A-operand prologue of the two GEMM test hooks: mode 1 = GRN apply, mode 2 = LayerNorm from row statistics, with the weight's row sums summed here into a
// cached scratch buffer (one extra M = 1 launch per call: timing loops over these hooks include it)
static int test_gemm_set_prologue(GemmArgs& g, int mode, const float* scale, const float* shift, int rows_per_sample, const float* ln_stats, hipStream_t st) {
    if (mode == 1) { g.a_scale = scale; g.a_shift = shift; g.a_rows_per_sample = rows_per_sample; }
    else if (mode == 2) {
        g.ln_stats = ln_stats; g.ln_nblk = g.K / 16; g.ln_eps = 1e-6f;
        static DevBuf ones, wsum;
        if (ones.n < (size_t)g.K) {
            std::vector<float> h((size_t)g.K, 1.0f);
            RET_IF(devbuf_alloc(ones, (size_t)g.K));
            HIP_CHECK_RET(hipMemcpy(ones.p, h.data(), (size_t)g.K * sizeof(float), hipMemcpyHostToDevice));
        }
        if (wsum.n < (size_t)g.N) RET_IF(devbuf_alloc(wsum, (size_t)g.N));
        GemmArgs gs = gemm_args(ones.p, g.K, g.W, g.ldw, wsum.p, g.N, 1, g.N, g.K);
        RET_IF(launch_gemm_cfg(gs, 5, 1, nullptr, 0, st));
        g.ln_wsum = wsum.p;
    }
    else if (mode != 0) { paella_set_error("prologue mode must be 0, 1 (scale / shift per sample) or 2 (LayerNorm from row statistics)"); return PAELLA_ERR_ARG; }
    return PAELLA_OK;
}
// test hook (test_hooks.h): the A-operand prologue variants of the GEMM with an explicit tile config / workgroup count
extern "C" int paella_test_gemm_prologue(const float* A, const float* W, float* C, int M, int N, int K, int mode, const float* scale,
                                         const float* shift, int rows_per_sample, const float* ln_stats, int tile_cfg, int splitk, void* ws,
                                         size_t ws_bytes, void* stream) {
    GemmArgs g = gemm_args(A, K, W, K, C, N, M, N, K);
    RET_IF(test_gemm_set_prologue(g, mode, scale, shift, rows_per_sample, ln_stats, (hipStream_t)stream));
    return launch_gemm_cfg(g, tile_cfg, splitk, ws, ws_bytes, (hipStream_t)stream);
}
// test hook (test_hooks.h): any fp32 GEMM launch, described field by field.  Everything is validated on the host BEFORE the first device call: the largest element
// index the launch can store into C / c16 (gemm_device.h: epilogue_write) and into the statistics (gemm.hip: ep_row) must fit the capacities the caller states
extern "C" size_t paella_test_gemm_args_size(void) { return sizeof(paella_test_gemm_args); }
static int test_gemm_max_store_index(const paella_test_gemm_args& a, long long* out) {
    const long long M = a.M, N = a.N;
    if (a.store_mode == STORE_PLAIN) {
        long long row = M - 1;
        if (a.remap_in > 0) {
            if (a.remap_out < 0 || a.remap_off < 0) { paella_set_error("gemm_desc: negative row remap"); return PAELLA_ERR_ARG; }
            const long long q = (M - 1) / a.remap_in, r = (M - 1) % a.remap_in;
            row = q * a.remap_out + r;                                           // the last row, or
            if (q > 0 && (q - 1) * a.remap_out + a.remap_in - 1 > row) row = (q - 1) * a.remap_out + a.remap_in - 1;  // the end of the last whole group (remap_out < remap_in)
            row += a.remap_off;
        }
        if (a.ldc < 0) { paella_set_error("gemm_desc: negative ldc"); return PAELLA_ERR_ARG; }
        *out = row * a.ldc + N - 1;
        return PAELLA_OK;
    }
    if (a.store_mode != STORE_D2S && a.store_mode != STORE_PIXSHUF_NCHW) { paella_set_error("gemm_desc: unknown store mode %d", a.store_mode); return PAELLA_ERR_ARG; }
    if (a.c16 || !a.C || a.remap_in > 0) { paella_set_error("gemm_desc: the bf16 copy, C == NULL and the row remap belong to the plain store"); return PAELLA_ERR_ARG; }
    if (a.sH < 1 || a.sW < 1 || a.sC < 1 || M % ((long long)a.sH * a.sW)) {
        paella_set_error("gemm_desc: a depth-to-space / pixel-shuffle store needs a source grid with M a multiple of sH * sW (M=%d sH=%d sW=%d sC=%d)", a.M, a.sH, a.sW, a.sC);
        return PAELLA_ERR_ARG;
    }
    const long long B = M / ((long long)a.sH * a.sW), H2 = 2ll * a.sH, W2 = 2ll * a.sW;
    if (a.store_mode == STORE_D2S) {
        if (a.n_seg_x < 1 || N % a.sC || a.py < 0 || a.px < 0 || a.ldc < 0) { paella_set_error("gemm_desc: bad depth-to-space store (N=%d sC=%d n_seg_x=%d py=%d px=%d)", a.N, a.sC, a.n_seg_x, a.py, a.px); return PAELLA_ERR_ARG; }
        const long long nseg = N / a.sC, dy = (nseg - 1) / a.n_seg_x, dx = (nseg < a.n_seg_x ? nseg : a.n_seg_x) - 1;
        const long long row = ((B - 1) * H2 + H2 - 2 + dy + a.py) * W2 + W2 - 2 + dx + a.px;
        *out = row * a.ldc + a.sC - 1;
    } else {
        *out = (((B - 1) * a.sC + (N - 1) / 4) * H2 + H2 - 1) * W2 + W2 - 1;
    }
    return PAELLA_OK;
}
extern "C" int paella_test_gemm_desc(const paella_test_gemm_args* a, int tile_cfg, int splitk, void* ws, size_t ws_bytes, void* stream) {
    if (!a || a->M <= 0 || a->N <= 0 || a->K <= 0 || !a->A || !a->W || (!a->C && !a->c16)) { paella_set_error("gemm_desc: null argument or empty problem"); return PAELLA_ERR_ARG; }
    long long last = 0;
    RET_IF(test_gemm_max_store_index(*a, &last));
    if ((a->C && (unsigned long long)last >= a->c_capacity) || (a->c16 && (unsigned long long)last >= a->c16_capacity)) {
        paella_set_error("gemm_desc: the launch stores up to element %lld, past the stated capacity (C %zu, c16 %zu)", last, a->C ? a->c_capacity : (size_t)0, a->c16 ? a->c16_capacity : (size_t)0);
        return PAELLA_ERR_ARG;
    }
    if (a->rowstat_out && (unsigned long long)a->M * (a->N / 16) * 2 > a->rowstat_capacity) {
        paella_set_error("gemm_desc: rowstat_out needs M * (N / 16) * 2 = %lld elements, capacity %zu", (long long)a->M * (a->N / 16) * 2, a->rowstat_capacity);
        return PAELLA_ERR_ARG;
    }
    if (a->sumsq_out && (unsigned long long)((a->M + 15) / 16) * a->N > a->sumsq_capacity) {
        paella_set_error("gemm_desc: sumsq_out needs ceil(M / 16) * N = %lld elements, capacity %zu", (long long)((a->M + 15) / 16) * a->N, a->sumsq_capacity);
        return PAELLA_ERR_ARG;
    }
    GemmArgs g = gemm_args(a->A, a->lda, a->W, a->ldw, a->C, a->ldc, a->M, a->N, a->K);
    Epilogue& e = g.ep;
    e.bias = a->bias; e.act = a->act; e.alpha = a->alpha; e.residual = a->residual; e.ldr = a->ldr;
    e.ts = a->ts; e.ts_stride = a->ts_stride; e.rows_per_sample = a->rows_per_sample > 0 ? a->rows_per_sample : 1;
    e.store_mode = a->store_mode; e.sH = a->sH; e.sW = a->sW; e.sC = a->sC; e.py = a->py; e.px = a->px; e.n_seg_x = a->n_seg_x;
    e.rowstat_out = a->rowstat_out; e.sumsq_out = a->sumsq_out;
    e.remap_in = a->remap_in; e.remap_out = a->remap_out; e.remap_off = a->remap_off;
    e.c16 = a->c16;
    if (a->cv_enabled) {
        g.cv.enabled = 1; g.cv.Hi = a->cv_Hi; g.cv.Wi = a->cv_Wi; g.cv.C = a->cv_C; g.cv.Ho = a->cv_Ho; g.cv.Wo = a->cv_Wo; g.cv.stride = a->cv_stride; g.cv.ntaps = a->cv_ntaps;
        g.cv.tw_log2 = a->cv_tw_log2; g.cv.oy0 = a->cv_oy0; g.cv.ox0 = a->cv_ox0; g.cv.tsign = a->cv_tsign;
    }
    RET_IF(test_gemm_set_prologue(g, a->mode, a->scale, a->shift, a->a_rows_per_sample, a->ln_stats, (hipStream_t)stream));
    return launch_gemm_cfg(g, tile_cfg, splitk, ws, ws_bytes, (hipStream_t)stream);
}
// test hook (test_hooks.h): the MLP pair of a ResBlock with GlobalResponseNorm finished inside the GEMMs (no finalize launch) -- the fused path of
// run_mlp_block on caller-provided tensors: out[M, c] = GRN(gelu(h W1^T + b1)) W2^T, hidden [M, 4c], gx [M / rps, 4c], part [M / rps, 4c / 16]
extern "C" int paella_test_mlp_grn_fused(const float* h, const float* W1, const float* b1, const float* gamma, const float* beta, const float* W2,
                                         float* hidden, float* gx, float* part, float* out, int M, int c, int rps, void* ws, size_t ws_bytes, void* stream) {
    const int tile = (rps % 16 == 0) ? gemm_grn_fused_tile(M, 4 * c, c, rps, true) : 0;
    if (!tile) { paella_set_error("fused GRN not applicable (M=%d c=%d rows per sample=%d)", M, c, rps); return PAELLA_ERR_ARG; }
    hipStream_t st = (hipStream_t)stream;
    const int np = (4 * c / 32) * 2;
    GemmArgs g1 = gemm_args(h, c, W1, c, hidden, 4 * c, M, 4 * c, c);
    g1.ep.bias = b1; g1.ep.act = ACT_GELU;
    g1.ep.grn_gx_out = gx; g1.ep.grn_part_out = part; g1.ep.grn_rps = rps; g1.ep.grn_np = np;
    g1.force_ring_cfg = tile;
    RET_IF(launch_gemm(g1, ws, ws_bytes, st));
    GemmArgs g2 = gemm_args(hidden, 4 * c, W2, 4 * c, out, c, M, c, 4 * c);
    g2.grn_gx = gx; g2.grn_part = part; g2.grn_np = np; g2.grn_gamma = gamma; g2.a_shift = beta; g2.a_rows_per_sample = rps;
    return launch_gemm(g2, ws, ws_bytes, st);
}
// test hook (test_hooks.h): one GEMM on bf16 operands (bit patterns supplied by the caller) with an explicit tile config / workgroup count;
// ln_stats != null folds a LayerNorm of the A rows into the epilogue (row sums of W16 computed here); C16 != null also stores the bf16 copy
extern "C" int paella_test_gemm_bf16(const unsigned short* A16, const unsigned short* W16, const float* bias, const float* residual, float* C, unsigned short* C16,
                                     int M, int N, int K, int act, const float* ln_stats, int tile_cfg, int splitk, void* ws, size_t ws_bytes, void* stream) {
    GemmArgs g = gemm_args(nullptr, K, nullptr, K, C, N, M, N, K);
    g.A16 = A16; g.W16 = W16;
    g.ep.bias = bias; g.ep.act = act; g.ep.residual = residual; g.ep.ldr = N; g.ep.c16 = C16;
    if (ln_stats) {
        static DevBuf wsum;
        if (wsum.n < (size_t)N) RET_IF(devbuf_alloc(wsum, (size_t)N));
        RET_IF(launch_rowsum_bf16(W16, wsum.p, N, K, (hipStream_t)stream));
        g.ln_stats = ln_stats; g.ln_nblk = K / 16; g.ln_eps = 1e-6f; g.ln_wsum = wsum.p;
    }
    return launch_gemm_cfg(g, tile_cfg, splitk, ws, ws_bytes, (hipStream_t)stream);
}
// test hook (test_hooks.h): the LayerNorm-folding bf16 GEMM as the model launches it -- bf16 copy A16 of the fp32 rows A32, statistics of the fp32 rows, and the
// fp32 rows themselves for the operand-side guard (blocks with |mean| / std above the fold threshold re-read and normalise them: gemm.hip, ln_fix)
extern "C" int paella_test_gemm_bf16_ln(const unsigned short* A16, const float* A32, const unsigned short* W16, float* C, int M, int N, int K, const float* ln_stats,
                                        int tile_cfg, int splitk, void* ws, size_t ws_bytes, void* stream) {
    if (!ln_stats) { paella_set_error("gemm_bf16_ln: statistics required"); return PAELLA_ERR_ARG; }
    GemmArgs g = gemm_args(A32, K, nullptr, K, C, N, M, N, K);
    g.A16 = A16; g.W16 = W16;
    static DevBuf wsum;
    if (wsum.n < (size_t)N) RET_IF(devbuf_alloc(wsum, (size_t)N));
    RET_IF(launch_rowsum_bf16(W16, wsum.p, N, K, (hipStream_t)stream));
    g.ln_stats = ln_stats; g.ln_nblk = K / 16; g.ln_eps = 1e-6f; g.ln_wsum = wsum.p;
    return launch_gemm_cfg(g, tile_cfg, splitk, ws, ws_bytes, (hipStream_t)stream);
}
// test hook (test_hooks.h): the fast mode's in-place GlobalResponseNorm apply on a bf16 tensor, h = bf16(h * scale[row / rows_per_sample] + shift)
extern "C" int paella_test_grn_apply16(unsigned short* h, const float* scale, const float* shift, int64_t rows, int rows_per_sample, int C, void* stream) {
    return launch_grn_apply16(h, scale, shift, rows, rows_per_sample, C, (hipStream_t)stream);
}
extern "C" int paella_op_layernorm(const float* x, float* y, int64_t rows, int C, float eps, void* stream) {
    return launch_layernorm(x, y, rows, C, eps, 1.f, 0.f, 0, 0, 0, (hipStream_t)stream);
}
extern "C" int paella_op_dwconv_ln(const float* x, const float* skip, const float* w, const float* bias, float* y, int B, int H, int W,
                                   int C, float eps, void* stream) {
    return launch_dwconv_ln(x, skip, w, bias, y, B, H, W, C, eps, (hipStream_t)stream);
}
extern "C" int paella_op_grn_scale(const float* g, const float* gamma, float* scale, float* tmp, int B, int rows_per_sample, int C,
                                   void* stream) {
    return launch_grn_scale(g, gamma, scale, tmp, B, rows_per_sample, C, (hipStream_t)stream);
}
static int op_attention_impl(const float* q, const float* k_self, const float* v_self, const float* k_cond, const float* v_cond, float* out, int B, int nhead, int D,
                             int Lq, int Lself, int Lcond, const int* cond_len, const float* key_weights, int n_kw, const float* kw_table, const int* kw_len,
                             int kw_pitch, const int* q_groups, int qg_pitch, const int* k_groups, int kg_pitch, void* stream) {
    AttnArgs a;
    const int ld = nhead * D;
    a.q = q; a.ldq = ld; a.k_self = k_self; a.v_self = v_self; a.ld_self = ld; a.k_cond = k_cond; a.v_cond = v_cond; a.ld_cond = ld;
    a.out = out; a.ldo = ld; a.B = B; a.nhead = nhead; a.D = D; a.Lq = Lq; a.Lself = Lself; a.Lcond = Lcond;
    a.scale = 1.0f / sqrtf((float)D); a.key_weights = key_weights; a.n_kw = key_weights ? n_kw : 0; a.out16 = nullptr;
    a.q16 = nullptr; a.k_self16 = nullptr; a.v_self16 = nullptr; a.ld16 = 0; a.cond_len = cond_len;
    a.kw_table = kw_table; a.kw_len = kw_len; a.kw_pitch = kw_pitch;
    a.q_groups = q_groups; a.qg_pitch = qg_pitch; a.k_groups = k_groups; a.kg_pitch = kg_pitch;
    return launch_attention(a, (hipStream_t)stream);
}
extern "C" int paella_op_attention_ragged(const float* q, const float* k_self, const float* v_self, const float* k_cond, const float* v_cond,
                                          float* out, int B, int nhead, int D, int Lq, int Lself, int Lcond, const int* cond_len, const float* key_weights,
                                          int n_kw, void* stream) {
    return op_attention_impl(q, k_self, v_self, k_cond, v_cond, out, B, nhead, D, Lq, Lself, Lcond, cond_len, key_weights, n_kw, nullptr, nullptr, 0, nullptr, 0, nullptr, 0, stream);
}
// per-sample key weights: the table (kw_table fp32 [B, kw_pitch], kw_len int32 [B]) in place of the shared vector; kw_len == NULL = no weights
extern "C" int paella_op_attention_kw(const float* q, const float* k_self, const float* v_self, const float* k_cond, const float* v_cond, float* out, int B, int nhead,
                                      int D, int Lq, int Lself, int Lcond, const int* cond_len, const float* kw_table, const int* kw_len, int kw_pitch, void* stream) {
    return op_attention_impl(q, k_self, v_self, k_cond, v_cond, out, B, nhead, D, Lq, Lself, Lcond, cond_len, nullptr, 0, kw_table, kw_len, kw_pitch, nullptr, 0, nullptr, 0, stream);
}
// per-query key groups on top of it (q_groups int32 [B, qg_pitch >= Lq], k_groups int32 [B, kg_pitch >= Lcond]; both NULL = the entry point above)
extern "C" int paella_op_attention_rg(const float* q, const float* k_self, const float* v_self, const float* k_cond, const float* v_cond, float* out, int B, int nhead,
                                      int D, int Lq, int Lself, int Lcond, const int* cond_len, const float* kw_table, const int* kw_len, int kw_pitch,
                                      const int* q_groups, int qg_pitch, const int* k_groups, int kg_pitch, void* stream) {
    return op_attention_impl(q, k_self, v_self, k_cond, v_cond, out, B, nhead, D, Lq, Lself, Lcond, cond_len, nullptr, 0, kw_table, kw_len, kw_pitch, q_groups, qg_pitch,
                             k_groups, kg_pitch, stream);
}
extern "C" int paella_op_attention(const float* q, const float* k_self, const float* v_self, const float* k_cond, const float* v_cond,
                                   float* out, int B, int nhead, int D, int Lq, int Lself, int Lcond, const float* key_weights,
                                   int n_kw, void* stream) {
    return paella_op_attention_ragged(q, k_self, v_self, k_cond, v_cond, out, B, nhead, D, Lq, Lself, Lcond, nullptr, key_weights, n_kw, stream);
}
// test hook (test_hooks.h): the bf16 attention core of the opt-in fast mode on caller-provided operands: q16 / ks16 / vs16 bf16 [B*L, nhead*D], kc / vc fp32, out16 bf16
static int test_attention_bf16_impl(const unsigned short* q16, const unsigned short* ks16, const unsigned short* vs16, const float* k_cond, const float* v_cond,
                                    unsigned short* out16, int B, int nhead, int D, int Lq, int Lself, int Lcond, const int* cond_len, const float* key_weights,
                                    int n_kw, const float* kw_table, const int* kw_len, int kw_pitch, void* stream) {
    AttnArgs a;
    const int ld = nhead * D;
    a.q = nullptr; a.ldq = ld; a.k_self = nullptr; a.v_self = nullptr; a.ld_self = ld; a.k_cond = k_cond; a.v_cond = v_cond; a.ld_cond = ld;
    a.out = nullptr; a.ldo = ld; a.B = B; a.nhead = nhead; a.D = D; a.Lq = Lq; a.Lself = Lself; a.Lcond = Lcond;
    a.scale = 1.0f / sqrtf((float)D); a.key_weights = key_weights; a.n_kw = key_weights ? n_kw : 0; a.out16 = out16;
    a.q16 = q16; a.k_self16 = ks16; a.v_self16 = vs16; a.ld16 = ld; a.cond_len = cond_len;
    a.kw_table = kw_table; a.kw_len = kw_len; a.kw_pitch = kw_pitch;
    return launch_attention(a, (hipStream_t)stream);
}
extern "C" int paella_test_attention_bf16_ragged(const unsigned short* q16, const unsigned short* ks16, const unsigned short* vs16, const float* k_cond,
                                                 const float* v_cond, unsigned short* out16, int B, int nhead, int D, int Lq, int Lself, int Lcond,
                                                 const int* cond_len, const float* key_weights, int n_kw, void* stream) {
    return test_attention_bf16_impl(q16, ks16, vs16, k_cond, v_cond, out16, B, nhead, D, Lq, Lself, Lcond, cond_len, key_weights, n_kw, nullptr, nullptr, 0, stream);
}
extern "C" int paella_test_attention_bf16_kw(const unsigned short* q16, const unsigned short* ks16, const unsigned short* vs16, const float* k_cond, const float* v_cond,
                                             unsigned short* out16, int B, int nhead, int D, int Lq, int Lself, int Lcond, const int* cond_len, const float* kw_table,
                                             const int* kw_len, int kw_pitch, void* stream) {
    return test_attention_bf16_impl(q16, ks16, vs16, k_cond, v_cond, out16, B, nhead, D, Lq, Lself, Lcond, cond_len, nullptr, 0, kw_table, kw_len, kw_pitch, stream);
}
extern "C" int paella_test_attention_bf16(const unsigned short* q16, const unsigned short* ks16, const unsigned short* vs16, const float* k_cond, const float* v_cond,
                                          unsigned short* out16, int B, int nhead, int D, int Lq, int Lself, int Lcond, const float* key_weights, int n_kw, void* stream) {
    return paella_test_attention_bf16_ragged(q16, ks16, vs16, k_cond, v_cond, out16, B, nhead, D, Lq, Lself, Lcond, nullptr, key_weights, n_kw, stream);
}
