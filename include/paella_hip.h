/*
 * paella_hip.h -- C ABI of libpaella_hip.so: the MI355X (gfx950) implementation of Paella's sampling hot path.
 *
 * The reference (dome272/Paella) is pure Python on PyTorch and has no FFI of its own; the drop-in
 * boundary is therefore the Python surface sample() / Paella / VQModel (paella_amd/ mirrors it), and this
 * header is what that Python surface -- or any other host language -- binds underneath.  Every entry point
 * names the reference code it replaces (file:line under the reference tree).
 *
 * Conventions
 *   - every pointer named dev_* / documented "device" is a HIP device pointer to contiguous fp32 / int64 data;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); all work is enqueued on it and
 *     no entry point on the per-step path synchronises the host;
 *   - functions return 0 on success, a negative PAELLA_ERR_* code otherwise; paella_last_error() returns a
 *     thread-local description of the last failure.  Nothing throws across this boundary;
 *   - the library owns only its repacked weight copies; activations, conditioning caches and workspaces are
 *     caller-owned device buffers whose sizes come from the *_bytes() queries;
 *   - every workspace (`ws`) begins with a small header of split-K arrival tickets: call paella_workspace_init() once
 *     on a freshly allocated workspace (a stream-ordered memset); the kernels leave the header zero afterwards.  One
 *     workspace must not be shared by calls that can run concurrently (one per stream / per captured graph);
 *   - handles are not thread-safe: one host thread per model per GPU (the reference's one-process-per-GPU
 *     layout, src_distributed/train.py:186-189).
 *   - activations inside the library are NHWC; logits are returned position-major [B, H, W, num_labels]
 *     (the Python shell hands the reference's [B, num_labels, H, W] shape back as a permuted view).
 */
#ifndef PAELLA_HIP_H
#define PAELLA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PAELLA_ABI_VERSION 8

#define PAELLA_OK 0
#define PAELLA_ERR_ARG -1       /* invalid argument / unsupported shape */
#define PAELLA_ERR_HIP -2       /* a HIP runtime call or kernel launch failed */
#define PAELLA_ERR_WORKSPACE -3 /* caller-provided buffer too small */
#define PAELLA_ERR_STATE -4     /* model not finalized / tensor missing */

#define PAELLA_MAX_LEVELS 8
#define PAELLA_MAX_BLOCK_TYPES 8

int paella_abi_version(void);
const char* paella_last_error(void);
/* Hash of the kernel sources this library was built from (paella_amd/_stamp.py); the Python binding refuses a library whose stamp differs
 * from the sources next to it. */
const char* paella_source_stamp(void);

/* Zeroes the header (paella_workspace_header_bytes() bytes) of a freshly allocated workspace; required once before the
 * workspace is first passed to any entry point below.  Enqueued on `stream`, no host synchronisation. */
int paella_workspace_init(void* ws, size_t ws_bytes, void* stream);
size_t paella_workspace_header_bytes(void);

/* ------------------------------------------------------------------------------------------------
 * Denoising UNet ("Paella", reference src/modules.py:109-283; alias DenoiseUNet)
 * ---------------------------------------------------------------------------------------------- */
typedef struct paella_unet paella_unet;

/* Mirrors the constructor arguments of reference src/modules.py:110-112. */
typedef struct paella_unet_config {
    int32_t c_in, c_out, num_labels, c_r, patch_size, c_cond;
    int32_t n_levels;
    int32_t c_hidden[PAELLA_MAX_LEVELS];
    int32_t nhead[PAELLA_MAX_LEVELS];
    int32_t blocks[PAELLA_MAX_LEVELS];
    char level_config[PAELLA_MAX_LEVELS][PAELLA_MAX_BLOCK_TYPES]; /* NUL-terminated, letters C T A F */
    int32_t clip_embd, byt5_embd, clip_seq_len, kernel_size, self_attn;
} paella_unet_config;

int paella_unet_create(const paella_unet_config* cfg, paella_unet** out);
void paella_unet_destroy(paella_unet* m);

/* Load one parameter by its reference state-dict key (e.g. "down_blocks.1.3.attention.attn.in_proj_weight")
 * in the reference's own layout; dev_src is a device pointer.  The library copies and repacks it into
 * kernel layout (NHWC-friendly conv weights, depth-to-space row order, ...).  May be called again later to
 * refresh a tensor. */
int paella_unet_load_tensor(paella_unet* m, const char* key, const float* dev_src, const int64_t* shape, int ndim,
                            void* stream);
/* Host table of the c_r/2 sinusoid frequencies exp(-k*log(1e4)/(c_r/2-1)) exactly as the reference computes
 * them (src/modules.py:215-216).  Optional: if never called the library computes them with expf(). */
int paella_unet_set_timestep_freqs(paella_unet* m, const float* host_freqs, int n);
/* Checks that every tensor the configuration needs has been loaded and builds the execution plan. */
int paella_unet_finalize(paella_unet* m, void* stream);

/* Sizes of the caller-owned buffers for a batch of B samples on an H x W token grid with S conditioning rows
 * per sample (S = S_byt5 + clip_seq_len*[clip] + clip_seq_len*n_clip_image). */
size_t paella_unet_cond_bytes(const paella_unet* m, int B, int S);
size_t paella_unet_workspace_bytes(const paella_unet* m, int B, int H, int W, int S);

/* Step-invariant conditioning work, hoisted out of the sampling loop: gen_c_embeddings
 * (src/modules.py:223-232; list-valued clip_image as utils/modules.py:229-235) followed, per AttnBlock, by
 * kv_mapper (src/modules.py:72-75,77) and the K/V in-projection of those rows (nn.MultiheadAttention).
 * byt5 [B, S_byt5, byt5_embd] (S_byt5 may be 0), clip [B, clip_embd] or NULL, clip_image: n_clip_image
 * pointers to [B, clip_embd].  Result goes to cond_out (paella_unet_cond_bytes(B, S) bytes). */
int paella_unet_cond_prepare(paella_unet* m, const float* byt5, int S_byt5, const float* clip,
                             const float* const* clip_image, int n_clip_image, int B, void* cond_out,
                             size_t cond_bytes, void* ws, size_t ws_bytes, void* stream);

/* gen_c_embeddings alone (src/modules.py:223-232): c_embed_out fp32 [B, S, c_cond]; ws needs
 * paella_unet_workspace_bytes() bytes. */
int paella_unet_c_embeddings(paella_unet* m, const float* byt5, int S_byt5, const float* clip,
                             const float* const* clip_image, int n_clip_image, int B, float* c_embed_out, void* ws,
                             size_t ws_bytes, void* stream);
/* gen_r_embedding (src/modules.py:212-221): r fp32 [B] -> r_embed_out fp32 [B, c_r] */
int paella_unet_r_embedding(paella_unet* m, const float* r, int B, float max_positions, float* r_embed_out,
                            void* stream);

/* OPT-IN fast mode of ONE model, outside the fp32 parity contract (no process-wide state): mode 1 routes the forward's dense contractions whose K is a
 * multiple of 64 through bf16-operand MFMA (v_mfma_f32_16x16x32_bf16, fp32 accumulation): bf16 shadow weights (made here / refreshed by finalize), bf16
 * activations between producer and consumer GEMMs (the 4c-wide MLP hidden tensor, LayerNorm and attention outputs, a bf16 copy of the residual stream where
 * a LayerNorm-folding GEMM reads it); the residual stream, statistics, attention, logits and the sampling tail stay fp32.  Mode 0 (default) is the exact
 * fp32 path, bit for bit.  Size workspaces (paella_unet_workspace_bytes) AFTER switching: mode 1 needs room for the bf16 activations.  The shadows stay
 * allocated until paella_unet_destroy (a HIP graph captured in mode 1 never dangles) and the switch to mode 0 does not synchronise. */
int paella_unet_set_precision(paella_unet* m, int mode, void* stream);
int paella_unet_get_precision(const paella_unet* m);

/* One denoising evaluation = Paella.forward (src/modules.py:263-275) with the conditioning already prepared.
 * tokens int64 [B,H,W]; r fp32 [B]; attn_weights (utils/alter_attention.py:23-34) fp32 [n_attn_weights] or NULL;
 * logits_out fp32 [B,H,W,num_labels]. */
int paella_unet_forward(paella_unet* m, const int64_t* tokens, const float* r, const void* cond, int B, int H, int W,
                        int S, const float* attn_weights, int n_attn_weights, float* logits_out, void* ws,
                        size_t ws_bytes, void* stream);
/* The same evaluation when batch rows b, b + n_unique, ... share tokens and r (classifier-free guidance: the conditional
 * and unconditional passes of src/utils.py:44-46 batched as 2 x n_unique rows against a B-row conditioning cache).
 * tokens is int64 [n_unique,H,W] and r fp32 [n_unique]: only the distinct rows are passed.  The blocks ahead of the first attention
 * block never see the conditioning and are computed once for the n_unique distinct rows.  n_unique must divide B;
 * n_unique == B with mix_c == mix_u == 0 is paella_unet_forward.
 * (mix_c, mix_u) != (0, 0) (needs B == 2 * n_unique) additionally folds the guidance mix of src/utils.py:47 through the
 * bias-free linear head (out_mapper, src/modules.py:184-187): logits_out then holds only the n_unique rows
 * mix_c * logits(cond) + mix_u * logits(uncond), fp32 [n_unique,H,W,num_labels], equal to mixing the two outputs up to
 * fp32 rounding. */
int paella_unet_forward_shared(paella_unet* m, const int64_t* tokens, const float* r, const void* cond, int B, int n_unique,
                               float mix_c, float mix_u, int H, int W, int S, const float* attn_weights,
                               int n_attn_weights, float* logits_out, void* ws, size_t ws_bytes, void* stream);

/* One whole sampling step in the counter-based (Philox) noise mode: Paella.forward followed by the sampling tail
 * (src/utils.py:43-54) with out_mapper (src/modules.py:184-187) and the tail FUSED: the categorical / argmax decision is taken
 * on the head GEMM's accumulators, the [rows, num_labels] logits tensor the reference materialises (:44-47) is never written.
 * Arguments as paella_unet_forward_shared + paella_sample_tail_ex; with a guidance mix (B == 2 * n_unique) tokens_out holds
 * n_unique x H x W tokens, without one B x H x W (n_unique == B).  Tokens are bit-identical to forward_shared + sample_tail_ex
 * on the same seed / offset / row_offset. */
int paella_unet_forward_sample(paella_unet* m, const int64_t* tokens, const float* r, const void* cond, int B, int n_unique,
                               float mix_c, float mix_u, int H, int W, int S, const float* attn_weights, int n_attn_weights,
                               float temperature, int mode, uint64_t seed, const uint64_t* seed_ptr, uint64_t offset,
                               int64_t row_offset, const int64_t* row_offset_ptr, const int64_t* init_noise, float t_next,
                               int64_t* tokens_out, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Sampling tail and add_noise (reference src/utils.py:45-54; src/modules.py:277-283)
 * ---------------------------------------------------------------------------------------------- */
/* logits_c / logits_u: fp32 [rows, L] (logits_u NULL = no classifier-free guidance);
 * mixes l = l_c*cfg + l_u*one_minus_cfg, divides by temperature, draws token = argmax softmax(l)/q with
 * q ~ Exp(1) (== torch.multinomial(softmax, 1)), then optionally renoises against init_noise with
 * u <= t_next.  mode 1 = argmax of the mixed logits (the T=0 extension).
 * noise_q [rows, L] / mask_u [rows]: caller-provided noise for bit-parity with torch; NULL = in-kernel
 * Philox4x32-10 keyed by (seed, offset).  sampled_out (optional) receives the pre-renoise draw. */
int paella_sample_tail(const float* logits_c, const float* logits_u, int64_t rows, int L, float cfg,
                       float one_minus_cfg, float temperature, int mode, const float* noise_q, uint64_t seed,
                       uint64_t offset, const int64_t* init_noise, const float* mask_u, float t_next,
                       int64_t* tokens_out, int64_t* sampled_out, void* stream);

/* Same, with (a) an optional DEVICE-resident seed word added to `seed` (seed_ptr may be NULL): a HIP graph that captured
 * the sampling loop can then be replayed with fresh noise by rewriting that one word; (b) row_offset: the Philox counters
 * are keyed by (row + row_offset), so a batch shard that owns global rows [lo, hi) passes lo * H * W and draws exactly the
 * noise the unsharded call draws for those rows (sharded == unsharded); (c) row_offset_ptr (may be NULL): a
 * DEVICE-resident word added to row_offset, so ONE captured graph serves any batch shard by rewriting that word. */
int paella_sample_tail_ex(const float* logits_c, const float* logits_u, int64_t rows, int L, float cfg,
                          float one_minus_cfg, float temperature, int mode, const float* noise_q, uint64_t seed,
                          const uint64_t* seed_ptr, uint64_t offset, int64_t row_offset, const int64_t* row_offset_ptr,
                          const int64_t* init_noise, const float* mask_u, float t_next, int64_t* tokens_out,
                          int64_t* sampled_out, void* stream);

/* Start tokens of the counter-based noise mode (the reference draws torch.randint(0, num_labels, (B,H,W)) from the global
 * generator, src/utils.py:37 -- a stream that cannot be sharded): tokens_out[i] = Philox(seed + *seed_ptr, i + row_offset +
 * *row_offset_ptr) mod num_labels for i in [0, n).  A shard that owns global rows [lo, hi) passes row_offset = lo * H * W and
 * n = (hi - lo) * H * W and obtains exactly its slice of the unsharded draw.  Either pointer may be NULL. */
int paella_start_tokens(uint64_t seed, const uint64_t* seed_ptr, int64_t row_offset, const int64_t* row_offset_ptr,
                        int num_labels, int64_t n, int64_t* tokens_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Request batch (ABI 6): the B samples of one call are B independent REQUESTS, each with its own seed, guidance pair and
 * temperature, read per step from DEVICE tables -- a captured graph serves any mix of them by rewriting the tables:
 *   seeds        uint64 [B]     (an int64 tensor holding the bit patterns)
 *   temperature  fp32   [B]     this step's row of a [steps, B] table; every entry > 0 (not checked on the device: the
 *                               caller validates; the argmax extension is not offered per request)
 *   pairs        fp32   [B, 2]  this step's (cfg, 1 - cfg), rounded by the caller as for the scalar entry points
 * Sample b = row / rows_per_sample draws exactly what the scalar entry point draws for it ALONE: seed = seeds[b],
 * row_offset = 0, rows = rows_per_sample, its own scalars -- counters are built from the position inside the sample,
 * never from the global row, so the result does not depend on the slot or on the batch-mates.  Categorical mode and
 * in-kernel Philox noise only.  The scalar entry points above keep their signatures and their tokens.
 * ---------------------------------------------------------------------------------------------- */
/* paella_sample_tail_ex per request; cfg_pairs may be NULL (no guidance: logits_u ignored as when it is NULL). */
int paella_sample_tail_req(const float* logits_c, const float* logits_u, int64_t rows, int L, const float* cfg_pairs,
                           const float* temperature, const uint64_t* seeds, int rows_per_sample, uint64_t offset,
                           const int64_t* init_noise, float t_next, int64_t* tokens_out, int64_t* sampled_out, void* stream);
/* paella_start_tokens per request: tokens_out[b * rows_per_sample + p] = the start token p of seeds[b]. */
int paella_start_tokens_req(const uint64_t* seeds, int B, int rows_per_sample, int num_labels, int64_t* tokens_out, void* stream);
/* paella_unet_forward_shared with one guidance pair per sample: mix_pairs [n_unique, 2] (required, B == 2 * n_unique);
 * logits_out holds the n_unique mixed rows.  A pair (1, 0) reproduces the conditional logits exactly only while the
 * unconditional activations are finite (0 * inf = NaN). */
int paella_unet_forward_shared_req(paella_unet* m, const int64_t* tokens, const float* r, const void* cond, int B, int n_unique,
                                   const float* mix_pairs, int H, int W, int S, const float* attn_weights, int n_attn_weights,
                                   float* logits_out, void* ws, size_t ws_bytes, void* stream);
/* paella_unet_forward_sample per request: mix_pairs [n_unique, 2] with B == 2 * n_unique, or NULL (no guidance,
 * n_unique == B); rows_per_sample must equal H * W.  Tokens are bit-identical to forward_shared_req + sample_tail_req. */
int paella_unet_forward_sample_req(paella_unet* m, const int64_t* tokens, const float* r, const void* cond, int B, int n_unique,
                                   const float* mix_pairs, int H, int W, int S, const float* attn_weights, int n_attn_weights,
                                   const uint64_t* seeds, const float* temperature, int rows_per_sample, uint64_t offset,
                                   const int64_t* init_noise, float t_next, int64_t* tokens_out, void* ws, size_t ws_bytes,
                                   void* stream);

/* ------------------------------------------------------------------------------------------------
 * Request stream (ABI 7): continuous batching.  The B slots of a fixed-shape batch hold requests that joined at different
 * ticks and run different numbers of steps; one tick = paella_request_step + paella_unet_forward_sample_stream, the same
 * launches whatever the slots hold, so ONE captured graph of a tick is replayed while requests come and go.  On top of the
 * request-batch tables, three DEVICE tables with one entry per slot replace the last per-launch scalars:
 *   step    int32 [B]  the request's OWN step index: the Philox step word of its categorical and renoise draws (was `offset`)
 *   t_next  fp32  [B]  its renoise threshold at this step (was `t_next`); negative = no renoise at this step (u >= 0)
 *   active  int32 [B]  0 = the slot holds no running request: its rows are computed and NOTHING is stored for them --
 *                      tokens_out (and sampled_out) keep their previous content, so the stream runs in place
 *                      (tokens_out == tokens) and a finished request's tokens stay in its slot until collected
 * All three tables and init_noise (the renoise source of every slot) are required: NULL is PAELLA_ERR_ARG.  With
 * step[b] = i, t_next[b] = t, active[b] = 1 for every b the tokens equal the *_req call with offset = i, t_next = t.
 * ---------------------------------------------------------------------------------------------- */
/* One tick of the slots' programs.  program fp32 [B, max_steps, 5], row j of slot b = (r, temperature, cfg, 1 - cfg, t_next)
 * of its step j; pos int32 [B] cursors; len int32 [B] step counts.  For every slot: active[b] = 0 <= pos[b] < min(len[b],
 * max_steps); an active slot gets r[b], temperature[b], pairs[b] (pairs may be NULL: no guidance), t_next[b] from row pos[b]
 * and its cursor advances; an idle one gets r 0, temperature 1, pair (1, 0), t_next -1.  step[b] = pos[b] before the advance. */
int paella_request_step(const float* program, int max_steps, int* pos, const int* len, int B, float* r, float* temperature,
                        float* pairs, float* t_next, int* step, int* active, void* stream);
/* paella_sample_tail_req in the stream form. */
int paella_sample_tail_stream(const float* logits_c, const float* logits_u, int64_t rows, int L, const float* cfg_pairs,
                              const float* temperature, const uint64_t* seeds, int rows_per_sample, const int* step,
                              const float* t_next, const int* active, const int64_t* init_noise, int64_t* tokens_out,
                              int64_t* sampled_out, void* stream);
/* paella_unet_forward_sample_req in the stream form; tokens_out may be `tokens` (the token gather at the head of the forward
 * and the token store at its tail are different kernels of one stream).  Bit-identical to forward_shared_req +
 * sample_tail_stream. */
int paella_unet_forward_sample_stream(paella_unet* m, const int64_t* tokens, const float* r, const void* cond, int B, int n_unique,
                                      const float* mix_pairs, int H, int W, int S, const float* attn_weights, int n_attn_weights,
                                      const uint64_t* seeds, const float* temperature, int rows_per_sample, const int* step,
                                      const float* t_next, const int* active, const int64_t* init_noise, int64_t* tokens_out,
                                      void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Ragged conditioning (ABI 8): the samples of ONE launch may have different numbers of conditioning rows.  The cache is
 * then B SLOTS of S rows each (S = the slot pitch, the `S` argument of every entry point below); sample b's real rows
 * [byt5 | clip | clip_image...] sit at the FRONT of slot b and a DEVICE table
 *   cond_len  int32 [B]   conditioning rows of sample b, clamped to [0, S] by the kernels
 * says how many there are.  Two properties hold in every attention kernel: (1) sample b of a ragged launch equals, bit for
 * bit, the same kernel launched for that sample alone with S = cond_len[b] and tightly packed rows; (2) rows >= cond_len[b]
 * of a slot are never read (they may hold anything, NaN included).  attn_weights weigh the last n keys of each sample's OWN
 * key sequence, so n must not exceed the shortest one (the caller validates).  cond_len == NULL is the non-ragged entry
 * point, bit for bit; every non-ragged entry point above keeps its signature and behaviour.
 * ---------------------------------------------------------------------------------------------- */
/* paella_unet_cond_prepare for a group of B samples of S = S_byt5 + ... rows each, written to the front of slots slot0 ..
 * slot0 + B - 1 (S_slot >= S rows per slot) of `cache`, a buffer of at least paella_unet_cond_bytes(slot0 + B, S_slot)
 * bytes; cond_len[slot0 .. slot0 + B) = S (stream-ordered).  The GEMM shapes are those of the plain call: the stored rows
 * equal its output bit for bit, and no byte outside them is written. */
int paella_unet_cond_prepare_slots(paella_unet* m, const float* byt5, int S_byt5, const float* clip,
                                   const float* const* clip_image, int n_clip_image, int B, int S_slot, int slot0,
                                   void* cache, size_t cache_bytes, int* cond_len, void* ws, size_t ws_bytes, void* stream);
/* The forward entry points with `cond_len` right after S; everything else as the entry point of the same name. */
int paella_unet_forward_shared_ragged(paella_unet* m, const int64_t* tokens, const float* r, const void* cond, int B, int n_unique,
                                      float mix_c, float mix_u, int H, int W, int S, const int* cond_len, const float* attn_weights,
                                      int n_attn_weights, float* logits_out, void* ws, size_t ws_bytes, void* stream);
int paella_unet_forward_sample_ragged(paella_unet* m, const int64_t* tokens, const float* r, const void* cond, int B, int n_unique,
                                      float mix_c, float mix_u, int H, int W, int S, const int* cond_len, const float* attn_weights,
                                      int n_attn_weights, float temperature, int mode, uint64_t seed, const uint64_t* seed_ptr,
                                      uint64_t offset, int64_t row_offset, const int64_t* row_offset_ptr, const int64_t* init_noise,
                                      float t_next, int64_t* tokens_out, void* ws, size_t ws_bytes, void* stream);
int paella_unet_forward_shared_req_ragged(paella_unet* m, const int64_t* tokens, const float* r, const void* cond, int B, int n_unique,
                                          const float* mix_pairs, int H, int W, int S, const int* cond_len, const float* attn_weights,
                                          int n_attn_weights, float* logits_out, void* ws, size_t ws_bytes, void* stream);
int paella_unet_forward_sample_req_ragged(paella_unet* m, const int64_t* tokens, const float* r, const void* cond, int B, int n_unique,
                                          const float* mix_pairs, int H, int W, int S, const int* cond_len, const float* attn_weights,
                                          int n_attn_weights, const uint64_t* seeds, const float* temperature, int rows_per_sample,
                                          uint64_t offset, const int64_t* init_noise, float t_next, int64_t* tokens_out, void* ws,
                                          size_t ws_bytes, void* stream);
int paella_unet_forward_sample_stream_ragged(paella_unet* m, const int64_t* tokens, const float* r, const void* cond, int B, int n_unique,
                                             const float* mix_pairs, int H, int W, int S, const int* cond_len, const float* attn_weights,
                                             int n_attn_weights, const uint64_t* seeds, const float* temperature, int rows_per_sample,
                                             const int* step, const float* t_next, const int* active, const int64_t* init_noise,
                                             int64_t* tokens_out, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Editing requests (ABI 8, extended ADDITIVELY: the entry points below were added without touching any existing signature, so the
 * version stays 8 and a caller of ABI 8 keeps working unchanged).  An inpainting / outpainting / structural-editing request knows part
 * of its token grid; the sampling tail itself re-imposes those tokens -- after the categorical draw and after the renoise:
 *   tokens_out[row] = (the pin applies to the row's slot && pin_keep[row] == 0) ? pin_tokens[row] : renoised token
 *   pin_keep    int64 [rows]  the mask type of paella_add_noise / paella_select_tokens: 1 = regenerate, 0 = known
 *   pin_tokens  int64 [rows]  the known tokens (read only where pin_keep is 0)
 *   pin_on      int32 [B]     request / stream forms only: this launch's flag per slot (paella_request_step_pin writes it); NULL =
 *                             the pin applies to every slot.  The scalar forms pin whenever the two row tables are given.
 * sampled_out stays the raw draw; a slot with active[b] == 0 still stores nothing, pinned or not.  pin_keep and pin_tokens come
 * together, pin_on only with them, the pin needs categorical mode: anything else is PAELLA_ERR_ARG.  With all pin tables NULL every
 * entry point below IS the entry point it extends -- same kernels, same launches, same tokens.
 * ---------------------------------------------------------------------------------------------- */
/* paella_request_step plus the pin policy of an editing stream: pin_policy int32 [B], per slot 0 = never, 1 = every step, 2 = the
 * request's final step only (pos[b] + 1 == len[b]); pin_on int32 [B] receives 1 for an active slot whose policy applies at this tick
 * and 0 otherwise (idle slots included).  Both NULL = paella_request_step; one without the other is PAELLA_ERR_ARG. */
int paella_request_step_pin(const float* program, int max_steps, int* pos, const int* len, int B, float* r, float* temperature,
                            float* pairs, float* t_next, int* step, int* active, const int* pin_policy, int* pin_on, void* stream);
/* paella_sample_tail_ex in the counter-based noise mode (no caller-provided noise) with the pin. */
int paella_sample_tail_pin(const float* logits_c, const float* logits_u, int64_t rows, int L, float cfg, float one_minus_cfg,
                           float temperature, int mode, uint64_t seed, const uint64_t* seed_ptr, uint64_t offset, int64_t row_offset,
                           const int64_t* row_offset_ptr, const int64_t* init_noise, float t_next, const int64_t* pin_keep,
                           const int64_t* pin_tokens, int64_t* tokens_out, int64_t* sampled_out, void* stream);
/* paella_sample_tail_stream with the pin. */
int paella_sample_tail_stream_pin(const float* logits_c, const float* logits_u, int64_t rows, int L, const float* cfg_pairs,
                                  const float* temperature, const uint64_t* seeds, int rows_per_sample, const int* step,
                                  const float* t_next, const int* active, const int64_t* init_noise, const int64_t* pin_keep,
                                  const int64_t* pin_tokens, const int* pin_on, int64_t* tokens_out, int64_t* sampled_out, void* stream);
/* paella_unet_forward_sample_ragged with the pin (cond_len may be NULL: the non-ragged entry point). */
int paella_unet_forward_sample_pin(paella_unet* m, const int64_t* tokens, const float* r, const void* cond, int B, int n_unique,
                                   float mix_c, float mix_u, int H, int W, int S, const int* cond_len, const float* attn_weights,
                                   int n_attn_weights, float temperature, int mode, uint64_t seed, const uint64_t* seed_ptr,
                                   uint64_t offset, int64_t row_offset, const int64_t* row_offset_ptr, const int64_t* init_noise,
                                   float t_next, const int64_t* pin_keep, const int64_t* pin_tokens, int64_t* tokens_out, void* ws,
                                   size_t ws_bytes, void* stream);
/* paella_unet_forward_sample_stream_ragged with the pin (cond_len may be NULL: the non-ragged entry point): the tick of an editing
 * stream.  Bit-identical to forward_shared_req(_ragged) + sample_tail_stream_pin. */
int paella_unet_forward_sample_stream_pin(paella_unet* m, const int64_t* tokens, const float* r, const void* cond, int B, int n_unique,
                                          const float* mix_pairs, int H, int W, int S, const int* cond_len, const float* attn_weights,
                                          int n_attn_weights, const uint64_t* seeds, const float* temperature, int rows_per_sample,
                                          const int* step, const float* t_next, const int* active, const int64_t* init_noise,
                                          const int64_t* pin_keep, const int64_t* pin_tokens, const int* pin_on, int64_t* tokens_out,
                                          void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Per-request prompt weights (ABI 8, extended ADDITIVELY as the editing entry points were: no existing signature changes, the version
 * stays 8).  attn_weights (utils/alter_attention.py:23-34: post-softmax multipliers of the LAST n keys, no renormalisation) is one
 * vector per launch in every entry point above.  The entry points below take two DEVICE tables with one row per conditioning SLOT of
 * the launch instead -- B rows, so the conditional and the unconditional half of a guided step (B == 2 * n_unique) carry independent
 * rows and every request of a batch its own:
 *   kw_table  fp32  [B, kw_pitch]  row b = the multipliers of slot b at its front
 *   kw_len    int32 [B]            how many there are; 0 = slot b is unweighted
 *   kw_pitch  int                  the row pitch in floats (>= 1)
 * Slot b weighs the last n = clamp(kw_len[b], 0, min(its own key count, kw_pitch)) keys of its OWN key sequence (self keys + its conditioning rows,
 * cond_len[b] of them in a ragged launch): key (count - n + i) is multiplied by kw_table[b * kw_pitch + i].  Three properties hold in
 * every attention kernel: (1) slot b of a table launch equals, bit for bit, the same kernel launched for that sample alone with the
 * shared vector = row b, n_attn_weights = n -- or with attn_weights == NULL when n == 0; (2) entries >= n of a row are never read
 * (they may hold anything, NaN included), and a row with n == 0 is not read at all; (3) kw_len == NULL: kw_table is ignored and each
 * entry point below IS the entry point it extends with attn_weights == NULL -- same launches, same results.  A count larger than the
 * slot's key sequence is clamped, which shifts the meaning of the row: the caller validates (paella_amd does, at admission).
 * Each entry point is the most general member of its family: cond_len is nullable (NULL = every slot has S rows), and so are the pin
 * tables of the two sampling ones (all NULL = the unpinned tail).  kw_len without kw_table, or kw_pitch < 1, is PAELLA_ERR_ARG.
 * ---------------------------------------------------------------------------------------------- */
/* paella_unet_forward_shared_req_ragged with the table.  mix_pairs may be NULL here: no guidance mix, logits_out holds the B rows
 * (n_unique dividing B as in paella_unet_forward_shared). */
int paella_unet_forward_shared_req_kw(paella_unet* m, const int64_t* tokens, const float* r, const void* cond, int B, int n_unique,
                                      const float* mix_pairs, int H, int W, int S, const int* cond_len, const float* kw_table,
                                      const int* kw_len, int kw_pitch, float* logits_out, void* ws, size_t ws_bytes, void* stream);
/* paella_unet_forward_sample_req_ragged with the table and the pin tables (pin_on may be NULL alone: the pin applies to every slot).
 * Tokens are bit-identical to forward_shared_req_kw + paella_sample_tail_req. */
int paella_unet_forward_sample_req_kw(paella_unet* m, const int64_t* tokens, const float* r, const void* cond, int B, int n_unique,
                                      const float* mix_pairs, int H, int W, int S, const int* cond_len, const float* kw_table,
                                      const int* kw_len, int kw_pitch, const uint64_t* seeds, const float* temperature,
                                      int rows_per_sample, uint64_t offset, const int64_t* init_noise, float t_next,
                                      const int64_t* pin_keep, const int64_t* pin_tokens, const int* pin_on, int64_t* tokens_out, void* ws,
                                      size_t ws_bytes, void* stream);
/* paella_unet_forward_sample_stream_pin with the table: the tick of a stream whose requests carry their own prompt weights. */
int paella_unet_forward_sample_stream_kw(paella_unet* m, const int64_t* tokens, const float* r, const void* cond, int B, int n_unique,
                                         const float* mix_pairs, int H, int W, int S, const int* cond_len, const float* kw_table,
                                         const int* kw_len, int kw_pitch, const uint64_t* seeds, const float* temperature,
                                         int rows_per_sample, const int* step, const float* t_next, const int* active,
                                         const int64_t* init_noise, const int64_t* pin_keep, const int64_t* pin_tokens, const int* pin_on,
                                         int64_t* tokens_out, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Regional prompts: per-query key groups (ABI 8, extended ADDITIVELY: no existing signature changes, the version stays 8).  In every
 * entry point above a query sees every conditioning row of its slot.  The entry points below take two more DEVICE tables, both or
 * neither (one alone is PAELLA_ERR_ARG), with one row per conditioning SLOT of the launch -- nb = B rows, 2 * n_unique in a guided step,
 * conditional slots first, as for kw_table:
 *   q_groups  int32 [nb, qg_pitch]  one bit mask per QUERY of every attention level, level-major inside a row: level l holds
 *                                   (H / patch)(W / patch) / 4^l queries (row-major positions of that level's grid) at offset
 *                                   off_l = sum_{j < l} (H / patch)(W / patch) / 4^j; qg_pitch >= Qtot = the sum over all levels.
 *                                   An attention block of level l passes base + off_l with pitch qg_pitch to its kernel
 *   k_groups  int32 [nb, kg_pitch]  one bit mask per conditioning ROW of the slot; kg_pitch >= S (the slot pitch)
 * Conditioning key c of slot b is VISIBLE to query q iff q_groups[b][q] & k_groups[b][c] != 0; self keys are always visible.  An
 * invisible key gets the score -inf before the softmax, like a row past cond_len.  What a bit means is the caller's business.
 * cond_len, attn weights and kw_table keep their meaning: weights address the last n keys of the slot's own key sequence by index,
 * visible or not, and act post-softmax on what is visible.  In every attention kernel: (1) a slot whose every conditioning key is
 * visible to every query computes the bits of the launch without the tables; (2) a slot whose keys [n, cond_len[b]) are invisible to
 * every query computes the bits of cond_len[b] = n -- but, unlike rows past cond_len, INVISIBLE ROWS ARE READ and multiplied by a zero
 * probability: every row below cond_len must be finite; (3) k_groups entries at or beyond cond_len[b] are without effect, and no read
 * leaves a row's pitch; (4) a query that sees no key at all (possible without self-attention only) gets a zero row, never NaN.
 * fp32 kernels only: PAELLA_ERR_ARG for a model in the bf16 precision mode, for pitches smaller than Qtot / S, and for one table without
 * the other -- all returned before anything is enqueued.  With both tables NULL each entry point IS the _kw one it extends.
 * ---------------------------------------------------------------------------------------------- */
int paella_unet_forward_shared_req_rg(paella_unet* m, const int64_t* tokens, const float* r, const void* cond, int B, int n_unique,
                                      const float* mix_pairs, int H, int W, int S, const int* cond_len, const float* kw_table,
                                      const int* kw_len, int kw_pitch, const int* q_groups, int qg_pitch, const int* k_groups,
                                      int kg_pitch, float* logits_out, void* ws, size_t ws_bytes, void* stream);
int paella_unet_forward_sample_stream_rg(paella_unet* m, const int64_t* tokens, const float* r, const void* cond, int B, int n_unique,
                                         const float* mix_pairs, int H, int W, int S, const int* cond_len, const float* kw_table,
                                         const int* kw_len, int kw_pitch, const int* q_groups, int qg_pitch, const int* k_groups,
                                         int kg_pitch, const uint64_t* seeds, const float* temperature, int rows_per_sample,
                                         const int* step, const float* t_next, const int* active, const int64_t* init_noise,
                                         const int64_t* pin_keep, const int64_t* pin_tokens, const int* pin_on, int64_t* tokens_out,
                                         void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Truncated sampling (ABI 8, extended ADDITIVELY: no existing signature changes, the version stays 8): top-k, nucleus (top-p) and
 * typical filtering of the categorical draw, on materialised logits (the fused head sees 64 columns at a time and has no row
 * statistics; feed these from the logits-returning forwards).  Per row, with z_i = fp32(mix_i * (1 / T)):
 *   A    = {i : z_i >= the top_k-th largest z}, ties kept; every label when top_k <= 0 or top_k >= L
 *   p    = softmax(z) over A
 *   top_p = P in (0, 1):        kept = {i in A : z_i >= v*},  v* the largest value with sum_{z_j >= v*} p_j >= P
 *   typical_mass = M in (0, 1): kept = {i in A : d_i <= d*},  d_i = |-log p_i - H|, H = -sum p log p, d* the smallest value with
 *                               sum_{d_j <= d*} p_j >= M
 *   neither:                    kept = A.  A mass of 1 is "off"; both below 1 is PAELLA_ERR_ARG (in a table row: top_p wins).
 *   min_tokens = n >= 1:        with a mass filter, the n first labels of A in that filter's order stay as well (ties kept)
 * token = the first arg-max over kept of the scores of the unfiltered tail, drawn from the same Philox words: the filter removes
 * candidates and never changes a random number, so a row whose kept set is every label yields the token of the entry point extended.
 * A row with a NaN or without a finite maximum is not filtered; a mass target that rounding keeps out of reach keeps A.  Renoise,
 * pin, sampled_out and active[] apply after the draw exactly as before.  Categorical mode and in-kernel noise only; L <= 16384
 * (a row lives in LDS), L % 4 == 0; anything else is PAELLA_ERR_ARG.
 * ---------------------------------------------------------------------------------------------- */
/* paella_sample_tail_pin with one filter setting for the launch. */
int paella_sample_tail_filter(const float* logits_c, const float* logits_u, int64_t rows, int L, float cfg, float one_minus_cfg,
                              float temperature, int mode, uint64_t seed, const uint64_t* seed_ptr, uint64_t offset, int64_t row_offset,
                              const int64_t* row_offset_ptr, const int64_t* init_noise, float t_next, const int64_t* pin_keep,
                              const int64_t* pin_tokens, int top_k, float top_p, float typical_mass, int min_tokens,
                              int64_t* tokens_out, int64_t* sampled_out, void* stream);
/* paella_sample_tail_stream_pin with one filter per request: DEVICE tables filter_k int32 [B, 2] = (top_k, min_tokens) and
 * filter_mass fp32 [B, 2] = (top_p, typical_mass), both or neither.  A request whose row says "off" takes the plain arg-max loop
 * (tokens of paella_sample_tail_stream_pin bit for bit); both NULL IS paella_sample_tail_stream_pin -- same kernel, same launch. */
int paella_sample_tail_stream_filter(const float* logits_c, const float* logits_u, int64_t rows, int L, const float* cfg_pairs,
                                     const float* temperature, const uint64_t* seeds, int rows_per_sample, const int* step,
                                     const float* t_next, const int* active, const int64_t* init_noise, const int64_t* pin_keep,
                                     const int64_t* pin_tokens, const int* pin_on, const int* filter_k, const float* filter_mass,
                                     int64_t* tokens_out, int64_t* sampled_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Confidence-ordered renoise and per-token confidence maps (ABI 8, extended ADDITIVELY: no existing signature changes, the version stays
 * 8).  Two additions, both categorical mode and in-kernel Philox noise only.
 * (1) Statistics of the draw.  With z, A, m and p = softmax(z) over A as under "Truncated sampling" (A = every label unless top_k is on),
 *     S = sum_A exp(z - m), E = sum_A (z - m) exp(z - m) and t the drawn label (always in A):
 *       logprob_out[row] = (z_t - m) - log S        entropy_out[row] = log S - E / S         fp32 [rows] each, either may be NULL
 *     from the sums the filter kernel forms, in their fixed order.  A row the filter would not filter (a NaN, no finite maximum) reports
 *     -inf / NaN.  Asking for them never changes a token: the draw is the filter tail's, bit for bit, any filter on or off; renoise, pin,
 *     sampled_out and active[] act as before (an inactive slot's statistics are not stored either).
 * (2) The renoise stage: which positions of a sample go back to init_noise after a step, decided per SAMPLE of rows_per_sample = H * W
 *     positions (1 ... 16384: a sample's keys live in LDS).  It runs after a tail called WITHOUT init_noise and WITHOUT the pin tables, on
 *     its raw draw.  free = the positions the pin does not own at this launch (pinned: pin_keep[row] == 0 and, stream form, pin_on[b] != 0).
 *       policy 0 (random):     tok = u <= t_next ? init_noise : drawn -- the coin of the tails above (same Philox words, same arithmetic):
 *                              tail without renoise + this stage == tail with init_noise, bit for bit
 *       policy 1 (confidence): exactly n = clamp(rint(t_next * |free|), 0, |free|) free positions are renoised (fp32 product, round to nearest
 *                              even; a negative t_next gives 0), the n smallest in (key(score), position index): score = logprob, or with
 *                              g = confidence_noise > 0, fma(-(g * t_next), log(-log u'), logprob) -- a Gumbel perturbation annealed with
 *                              t_next, u' from word 1 of the very Philox call whose word 0 is policy 0's coin (no new random stream: shards
 *                              and slots stay exact); key = the ascending order-preserving 32-bit key of the fp32 score, -0 == +0, NaN
 *                              first (the least confident), ties to the lower index
 *     then the pin: tokens_out[row] = pin_tokens[row] on a pinned position.  A slot with active[b] == 0 stores nothing.  tokens_out may
 *     alias drawn.  PAELLA_ERR_ARG, before anything is enqueued: rows not a multiple of rows_per_sample, rows_per_sample outside 1 ... 16384,
 *     one pin table without the other, policy 1 (stream form: a policy table) without logprob; scalar form: a policy other than 0 / 1, a
 *     negative or non-finite confidence_noise.
 * ---------------------------------------------------------------------------------------------- */
/* paella_sample_tail_filter plus the statistics; both outputs NULL IS paella_sample_tail_filter -- same kernel, same launch. */
int paella_sample_tail_stats(const float* logits_c, const float* logits_u, int64_t rows, int L, float cfg, float one_minus_cfg,
                             float temperature, int mode, uint64_t seed, const uint64_t* seed_ptr, uint64_t offset, int64_t row_offset,
                             const int64_t* row_offset_ptr, const int64_t* init_noise, float t_next, const int64_t* pin_keep,
                             const int64_t* pin_tokens, int top_k, float top_p, float typical_mass, int min_tokens, int64_t* tokens_out,
                             int64_t* sampled_out, float* logprob_out, float* entropy_out, void* stream);
/* paella_sample_tail_stream_filter plus the statistics; both outputs NULL IS that entry point.  With an output the filter tables stay
 * optional (both NULL = every request off). */
int paella_sample_tail_stream_stats(const float* logits_c, const float* logits_u, int64_t rows, int L, const float* cfg_pairs,
                                    const float* temperature, const uint64_t* seeds, int rows_per_sample, const int* step,
                                    const float* t_next, const int* active, const int64_t* init_noise, const int64_t* pin_keep,
                                    const int64_t* pin_tokens, const int* pin_on, const int* filter_k, const float* filter_mass,
                                    int64_t* tokens_out, int64_t* sampled_out, float* logprob_out, float* entropy_out, void* stream);
/* The renoise stage, scalar form: seed (+ *seed_ptr), step word `offset`, GLOBAL row offset (+ *row_offset_ptr; a multiple of
 * rows_per_sample for a batch shard, which then equals its rows of the unsharded call) and t_next as paella_sample_tail_ex takes them.
 * drawn int64 [rows], logprob fp32 [rows] (may be NULL with policy 0), init_noise int64 [rows]. */
int paella_renoise_select(const int64_t* drawn, const float* logprob, const int64_t* init_noise, int64_t rows, int rows_per_sample,
                          uint64_t seed, const uint64_t* seed_ptr, uint64_t offset, int64_t row_offset, const int64_t* row_offset_ptr,
                          float t_next, int policy, float confidence_noise, const int64_t* pin_keep, const int64_t* pin_tokens,
                          int64_t* tokens_out, void* stream);
/* The renoise stage, request / stream form: seeds, step, t_next, active per slot as paella_sample_tail_stream takes them (all required);
 * policy int32 [B] (1 = confidence, anything else random; NULL = every slot random) and confidence_noise fp32 [B] (NULL = 0). */
int paella_renoise_select_stream(const int64_t* drawn, const float* logprob, const int64_t* init_noise, int64_t rows, int rows_per_sample,
                                 const uint64_t* seeds, const int* step, const float* t_next, const int* active, const int* policy,
                                 const float* confidence_noise, const int64_t* pin_keep, const int64_t* pin_tokens, const int* pin_on,
                                 int64_t* tokens_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Argument blocks (ABI 8, extended ADDITIVELY: no existing signature changes, the version stays 8): ONE forward and ONE sampling tail,
 * each taking everything its family takes in a struct.  Zero / NULL = "not given"; which form runs follows from what is present, and
 * every paella_unet_forward_shared*, paella_unet_forward_sample* and paella_sample_tail* entry point above is a fixed-form convenience
 * that fills a block and calls the same runner -- same rules, same kernels, same launch arguments.  Both entry points refuse an
 * args_bytes other than the library's sizeof(block) with PAELLA_ERR_ARG before reading anything else, read the block during the call
 * only (no pointer to it is kept: it may live on the caller's stack, also while a graph is captured) and validate every rule before
 * anything is enqueued.
 * ---------------------------------------------------------------------------------------------- */
/* A sampling tail.  rows_per_sample > 0 = the request form (seeds, temperature_tab required; the scalar-form fields other than offset and
 * t_next are not read); step != NULL = its stream form (step, t_next_tab, active and init_noise all required; offset and t_next not read).
 * Filter: the scalar form filters when any of the four values is non-zero (they are then the values of paella_sample_tail_filter:
 * 1 = a mass that is off, min_tokens >= 1), the request form when the two tables are given.  A statistics output selects the statistics
 * tail, a filter the filter tail, neither the plain (pin) tail. */
typedef struct paella_tail_args {
    const float *logits_c, *logits_u; int64_t rows; int32_t L;                                                      /* inputs [rows, L]; logits_u NULL = no guidance */
    float cfg, one_minus_cfg, temperature; int32_t mode; uint64_t seed; const uint64_t* seed_ptr; uint64_t offset;  /* scalar form */
    int64_t row_offset; const int64_t* row_offset_ptr; float t_next; const float *noise_q, *mask_u;
    const uint64_t* seeds; const float *temperature_tab, *cfg_pairs; int32_t rows_per_sample;                       /* request tables */
    const int32_t* step; const float* t_next_tab; const int32_t* active;                                            /* stream tables */
    const int64_t *init_noise, *pin_keep, *pin_tokens; const int32_t* pin_on;                                       /* renoise source; pin */
    int32_t top_k; float top_p, typical_mass; int32_t min_tokens; const int32_t* filter_k; const float* filter_mass; /* filter */
    int64_t *tokens_out, *sampled_out; float *logprob_out, *entropy_out;                                            /* outputs */
} paella_tail_args;

/* One forward.  tail == NULL: the logits go to logits_out (mix_pairs, or a non-zero (mix_c, mix_u), folds the guidance mix through the
 * head).  tail != NULL: the fused step of paella_unet_forward_sample*; the library fills the block's rows and L, reads neither its logits,
 * cfg pair, caller-provided noise nor sampled_out, and refuses a filter or a statistics output (they need materialised logits); the
 * request form needs rows_per_sample == H * W.  attn_weights (one vector) or kw_len / kw_table (one row per slot), not both; q_groups
 * and k_groups both or neither. */
typedef struct paella_step_args {
    const int64_t* tokens; const float* r; const void* cond; int32_t B, n_unique; float mix_c, mix_u; const float* mix_pairs; int32_t H, W, S; const int32_t* cond_len;
    const float* attn_weights; int32_t n_attn_weights;
    const float* kw_table; const int32_t* kw_len; int32_t kw_pitch;
    const int32_t* q_groups; int32_t qg_pitch; const int32_t* k_groups; int32_t kg_pitch;
    float* logits_out; const paella_tail_args* tail;
} paella_step_args;

int paella_unet_step(paella_unet* m, const paella_step_args* args, size_t args_bytes, void* ws, size_t ws_bytes, void* stream);
int paella_sample_tail_args(const paella_tail_args* args, size_t args_bytes, void* stream);

/* x, random_x, mask int64 [B, per_sample]; t fp32 [B].  mask_in NULL -> mask = (u <= t[b]) with u = rand_u
 * (caller noise, [B, per_sample]) or Philox; random_x NULL -> Philox randint(0, num_labels). */
int paella_add_noise(const int64_t* x, const float* t, const int64_t* mask_in, const int64_t* random_x,
                     const float* rand_u, uint64_t seed, uint64_t offset, int num_labels, int B,
                     int64_t per_sample, int64_t* x_out, int64_t* mask_out, void* stream);

/* Token select on the [B,H,W] grid: out[i] = keep(i) ? a[i] : (b ? b[i] : fill) with keep(i) = (mask == NULL || mask[i] != 0) && (flag == NULL ||
 * *flag == 1.0f).  `flag` is a DEVICE fp32 word.  Replaces the two integer elementwise expressions of the eval path that used to run through ATen: the
 * inpainting wrapper's `out * mask + tokens * (1 - mask)` (the recipe src/modules.py:277-283 + src_distributed/utils.py:97-109, extension keep_known) and
 * the batch-sharded sampler's "-1 when the conditioning broadcast was flagged invalid" (paella_amd/dist.py); no host synchronisation, graph-capturable. */
int paella_select_tokens(const int64_t* a, const int64_t* b, const int64_t* mask, const float* flag, int64_t fill, int64_t n,
                         int64_t* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * VQGAN (reference src/vqgan.py:45-107)
 * ---------------------------------------------------------------------------------------------- */
typedef struct paella_vqgan paella_vqgan;
typedef struct paella_vqgan_config {
    int32_t levels, bottleneck_blocks, c_hidden, c_latent, codebook_size;
    float scale_factor;
} paella_vqgan_config;

int paella_vqgan_create(const paella_vqgan_config* cfg, paella_vqgan** out);
void paella_vqgan_destroy(paella_vqgan* v);
int paella_vqgan_load_tensor(paella_vqgan* v, const char* key, const float* dev_src, const int64_t* shape, int ndim,
                             void* stream);
int paella_vqgan_finalize(paella_vqgan* v, void* stream); /* synchronises the stream once (reads the BatchNorm statistics / ResBlock gammas to the host) */
/* OPT-IN fast mode of ONE VQGAN (outside the fp32 parity contract, as paella_unet_set_precision): mode 1 runs the MLP of every ResBlock whose width is a
 * multiple of 64 on bf16-operand MFMA with fp32 accumulation (bf16 shadow weights, bf16 LayerNorm output and hidden tensor); everything else stays fp32.
 * Mode 0 (default) is the exact path.  Size workspaces (paella_vqgan_workspace_bytes) AFTER switching. */
int paella_vqgan_set_precision(paella_vqgan* v, int mode, void* stream); /* mode 1 on a finalized model converts the shadows and waits for them; mode 0 frees nothing and never synchronises */
/* h, w = latent grid; covers decode and encode of the matching image size.  Exactly this many bytes suffice; fewer is PAELLA_ERR_WORKSPACE before
 * anything is enqueued */
size_t paella_vqgan_workspace_bytes(const paella_vqgan* v, int B, int h, int w);
/* decode_indices (src/vqgan.py:103-107): idx int64 [B,h,w] -> image fp32 NCHW [B,3,f*h,f*w], f = 2^levels */
int paella_vqgan_decode_indices(paella_vqgan* v, const int64_t* idx, int B, int h, int w, float* img_out, void* ws,
                                size_t ws_bytes, void* stream);
/* decode (src/vqgan.py:97-101): latents fp32 NCHW [B,c_latent,h,w] (already divided by scale_factor, as encode returns) */
int paella_vqgan_decode(paella_vqgan* v, const float* latents, int B, int h, int w, float* img_out, void* ws,
                        size_t ws_bytes, void* stream);
/* encode (src/vqgan.py:91-95): image fp32 NCHW [B,3,Hp,Wp] -> qe_out, x_out fp32 NCHW [B,c_latent,h,w] (both /scale_factor),
 * idx_out int64 [B,h,w], loss_out fp32 [1] = vq_loss + 0.25*commit_loss.  Any output pointer may be NULL. */
int paella_vqgan_encode(paella_vqgan* v, const float* img, int B, int Hp, int Wp, float* qe_out, float* x_out,
                        int64_t* idx_out, float* loss_out, void* ws, size_t ws_bytes, void* stream);
/* VectorQuantize.forward on rows [rows, c_latent] (src/vqgan.py:94; src_distributed/train.py:156): nearest codebook row per
 * input row -> idx_out int64 [rows], qe_out fp32 [rows, c_latent] (optional), mse_out fp32 [1] = mean((qe - x)^2) (optional;
 * the stand-in's vq_loss == commit_loss). */
int paella_vqgan_quantize_rows(paella_vqgan* v, const float* x, int64_t rows, int64_t* idx_out, float* qe_out,
                               float* mse_out, void* stream);
/* VectorQuantize.idx2vq (src/vqgan.py:104): out fp32 [rows, c_latent] = codebook[idx].  An index outside [0, codebook_size) is CLAMPED to the nearest
 * valid one (negative -> row 0, >= codebook_size -> the last row), here and in paella_vqgan_decode_indices: no error, never a read outside the codebook. */
int paella_vqgan_lookup_rows(paella_vqgan* v, const int64_t* idx, int64_t rows, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Single-op entry points (used by the parity tests and the kernel micro-benchmarks)
 * ---------------------------------------------------------------------------------------------- */
/* C[M,N] = act(A[M,K] . W[N,K]^T + bias) (+ residual); act: 0 none, 1 GELU(erf).  tile_cfg < 0 = heuristic; otherwise a
 * tile id with splitk > 0 -> tiles * splitk workgroups (classic split-K), splitk < 0 -> exactly -splitk workgroups walking
 * balanced contiguous (tile, K-step) ranges.  ws = an initialised workspace (split-K tickets + slabs) or NULL. */
int paella_op_gemm(const float* A, const float* W, const float* bias, const float* residual, float* C, int M, int N,
                   int K, int act, int tile_cfg, int splitk, void* ws, size_t ws_bytes, void* stream);
int paella_op_layernorm(const float* x, float* y, int64_t rows, int C, float eps, void* stream);
/* depthwise 3x3 (+ optional skip concat) + LayerNorm on NHWC x [B,H,W,C]; w/bias in reference layout are NOT
 * accepted here: w is [9][C] ([2][9][C] with skip) */
int paella_op_dwconv_ln(const float* x, const float* skip, const float* w, const float* bias, float* y, int B, int H,
                        int W, int C, float eps, void* stream);
int paella_op_grn_scale(const float* g, const float* gamma, float* scale, float* tmp, int B, int rows_per_sample,
                        int C, void* stream);
/* q [B*Lq, nhead*D]; k/v self [B*Lself, nhead*D]; k/v cond [B*Lcond, nhead*D]; out [B*Lq, nhead*D] */
int paella_op_attention(const float* q, const float* k_self, const float* v_self, const float* k_cond,
                        const float* v_cond, float* out, int B, int nhead, int D, int Lq, int Lself, int Lcond,
                        const float* key_weights, int n_kw, void* stream);
/* the same over B slots of Lcond conditioning rows of which sample b attends the first cond_len[b] (int32 DEVICE table [B]; NULL = all Lcond) */
int paella_op_attention_ragged(const float* q, const float* k_self, const float* v_self, const float* k_cond,
                               const float* v_cond, float* out, int B, int nhead, int D, int Lq, int Lself, int Lcond,
                               const int* cond_len, const float* key_weights, int n_kw, void* stream);
/* the same with one key-weight row per sample (kw_table fp32 [B, kw_pitch], kw_len int32 [B]: see "Per-request prompt weights") in place of the shared
 * vector; cond_len may be NULL, kw_len == NULL = no weights */
int paella_op_attention_kw(const float* q, const float* k_self, const float* v_self, const float* k_cond, const float* v_cond,
                           float* out, int B, int nhead, int D, int Lq, int Lself, int Lcond, const int* cond_len,
                           const float* kw_table, const int* kw_len, int kw_pitch, void* stream);
/* the same with per-query key groups (q_groups int32 [B, qg_pitch >= Lq], k_groups int32 [B, kg_pitch >= Lcond]: see "Regional prompts"); both NULL = the
 * entry point above, one alone or a pitch too small = PAELLA_ERR_ARG */
int paella_op_attention_rg(const float* q, const float* k_self, const float* v_self, const float* k_cond, const float* v_cond,
                           float* out, int B, int nhead, int D, int Lq, int Lself, int Lcond, const int* cond_len,
                           const float* kw_table, const int* kw_len, int kw_pitch, const int* q_groups, int qg_pitch,
                           const int* k_groups, int kg_pitch, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training loss head (ABI 8, extended ADDITIVELY: no existing signature changes, the version stays 8): the classifier
 * head (out_mapper: 1x1 convolution, no bias) with the label-smoothed cross-entropy of the reference's training loops
 * (src/train.py:63-71: nn.CrossEntropyLoss(label_smoothing=0.1, reduction='none')) fused into it, forward and backward.
 * The [rows, N] logits are never stored: the forward reduces every 64 x 64 logit tile in its epilogue, the backward
 * recomputes the tiles from h, w and lse.
 *   h fp32 [rows, K] row-major (the rows of the last LayerNorm2d in NHWC order), w fp32 [N, K] (out_mapper.1.weight),
 *   target int64 [rows], eps = label_smoothing in [0, 1).  With l[m, n] = sum_k h[m, k] w[n, k] on the exact fp32 path:
 *     lse[m]    = log sum_n exp(l[m, n])          (running maximum: finite for any finite logits)
 *     loss[m]   = (1 - eps) (lse[m] - l[m, target[m]]) + eps (lse[m] - (1 / N) sum_n l[m, n])
 *     argmax[m] = the label of the largest l[m, .], the LOWEST label on ties
 *   A target outside [0, N) (negative values included: what ignore_index = -100 amounts to under reduction = 'none')
 *   marks an IGNORED row: loss 0, no contribution to either gradient, lse and argmax still produced; w and the
 *   workspace are never indexed with it.  Nothing is validated on the host, nothing synchronises.
 *   Backward, g = grad_loss fp32 [rows]:  d[m, n] = g[m] (exp(l[m, n] - lse[m]) - (1 - eps) [n == target[m]] - eps / N),
 *   0 on an ignored row;  dh[m, k] = sum_n d[m, n] w[n, k],  dw[n, k] = sum_m d[m, n] h[m, k].  Both are WRITTEN, not
 *   accumulated into; dh_out or dw_out NULL = that kernel is not launched (a frozen head, inputs without gradient).
 * Shapes: K a multiple of 16 in 16...256, N a multiple of 16 in 16...65536 (not necessarily of the 64-label tile: the
 * tail columns are masked), rows in 1...2^24.  Anything else, a NULL required pointer, eps outside [0, 1) or not
 * finite: PAELLA_ERR_ARG; a workspace smaller than paella_head_loss_workspace_bytes: PAELLA_ERR_WORKSPACE -- both
 * before anything is enqueued.  The workspace holds one partial per (row, 64-label tile) in the forward; in the
 * backward one number per (row, tile) -- the row sums that renormalise exp(l - lse), so that the rounding of the ONE
 * fp32 lse per row does not reach the probabilities -- and a bounded number of [N, K] slabs (a split of the row range
 * of dw); never anything of rows x N: from 4096 rows up it stays below rows * N bytes, a quarter of one logits tensor.  One workspace serves both calls; it carries no
 * state between them and needs no initialisation.  Deterministic: no float atomics, every combine (partials in
 * ascending tile order, slabs in ascending share order) in an order fixed by the shape alone, so two runs give the
 * same bits.  No allocation, no synchronisation, capturable in a graph.
 * ---------------------------------------------------------------------------------------------- */
size_t paella_head_loss_workspace_bytes(int64_t rows, int N, int K); /* 0 for an unsupported shape */
int paella_head_loss_forward(const float* h, const float* w, const int64_t* target, int64_t rows, int N, int K,
                             float label_smoothing, float* loss_out, float* lse_out, int* argmax_out /* may be NULL */,
                             void* ws, size_t ws_bytes, void* stream);
int paella_head_loss_backward(const float* h, const float* w, const int64_t* target, const float* lse,
                              const float* grad_loss, int64_t rows, int N, int K, float label_smoothing,
                              float* dh_out /* may be NULL */, float* dw_out /* may be NULL */, void* ws,
                              size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training MLP activation (ABI 8, extended ADDITIVELY: no existing signature changes, the version stays 8): the
 * middle of every ResBlock / FeedForwardBlock MLP in train mode -- GELU -> GlobalResponseNorm -> Dropout
 * (reference src/modules.py:30-40, 49-53) -- as one op, forward and backward (paella_amd/csrc/grn_act.hip).
 *   u fp32 [B, P, C]: the rows of the first Linear in NHWC order, P = H * W positions per sample; gamma, beta fp32 [C].
 *   With h = GELU(u) by the engine's exact-path erf form (train and eval agree on the activation):
 *     G[b, c] = sqrt(sum_p h^2),  M[b] = mean_c G[b, c],  n = G / (M + 1e-6),
 *     y = h (1 + gamma_c n[b, c]) + beta_c,  z = keep y (1 / (1 - p_drop)).
 *   gx_out receives G as [B, C]: with u and gamma it is ALL the backward needs -- h, y and the mask are recomputed.
 *   Dropout: p_drop == 0 draws nothing and z == y.  Otherwise element e (its flat index in [B, P, C]) takes word e & 3
 *   of philox4x32(seed ^ 0xa0761d6478bd642f, counter (e >> 2, 0)) and is kept iff (word >> 8) * 2^-24 >= p_drop; the
 *   scale is the one fp32 division 1.0f / (1.0f - p_drop).  The backward regenerates the mask from (seed, e).
 *   Backward for a given dz fp32 [B, P, C]:  dy = keep dz / (1 - p),  dbeta_c = sum_{b, p} dy,  S[b, c] = sum_p dy h,
 *     dgamma_c = sum_b n[b, c] S[b, c],  dn = gamma_c S,  dG = dn / (M + eps) - (sum_c' dn[b, c'] G[b, c']) / (C (M + eps)^2),
 *     dh = dy (1 + gamma_c n) + (G > 0 ? dG / G : 0) h,  du = dh (Phi(u) + u phi(u)).
 *   du, dgamma and dbeta are WRITTEN, not accumulated into; each may be NULL, and with all three NULL nothing is
 *   launched.  A channel that is identically zero in a sample (G = 0) gets torch.norm's gradient there, 0.
 * Shapes: C a multiple of 4 in 4...16384, P in 1...2^20, B in 1...65535; every tensor and the workspace 16-byte
 * aligned; all element offsets are 64-bit.  Anything else, a NULL required pointer, p_drop outside [0, 1) or not
 * finite: PAELLA_ERR_ARG; a workspace smaller than paella_grn_act_workspace_bytes: PAELLA_ERR_WORKSPACE -- both
 * before anything is enqueued.  Each direction makes two passes over the tensor (column sums over strips of rows;
 * the apply) around small finalize launches.  The workspace holds the per-strip partials [B, strips, C] (one set in
 * the forward, two in the backward; a strip is at least 8 rows, so at most a quarter of one activation tensor) and four
 * [B, C] / [B] tables.  One workspace serves both calls; it carries no state between them and needs no
 * initialisation.  Deterministic: no float atomics, no tickets; partials are combined in ascending strip order,
 * the per-sample terms of dgamma / dbeta in ascending b, the sums over channels by a fixed tree, and the strip
 * count depends on (P, C) only -- two runs and two devices give the same bits, and the values of a sample depend
 * neither on its index b nor on the batch size.  No allocation, no synchronisation, capturable in a graph.
 * ---------------------------------------------------------------------------------------------- */
size_t paella_grn_act_workspace_bytes(int B, int P, int C); /* 0 for an unsupported shape */
int paella_grn_act_forward(const float* u, const float* gamma, const float* beta, int B, int P, int C, float p_drop,
                           uint64_t seed, float* z_out, float* gx_out, void* ws, size_t ws_bytes, void* stream);
int paella_grn_act_backward(const float* u, const float* gamma, const float* gx, const float* dz, int B, int P, int C,
                            float p_drop, uint64_t seed, float* du_out /* may be NULL */,
                            float* dgamma_out /* may be NULL */, float* dbeta_out /* may be NULL */, void* ws,
                            size_t ws_bytes, void* stream);
/* The same two calls with the seed read from DEVICE memory (added ADDITIVELY, the version stays 8): seed_dev is the
 * address of one 64-bit word (8-byte aligned; required when p_drop > 0, not read when p_drop == 0) that the drawing
 * kernels load when they RUN -- so a captured call draws the mask of whatever the word holds at each replay.  A call
 * whose word holds s gives the bits of the by-value call with seed = s, in both directions; the backward must find
 * the word its forward found. */
int paella_grn_act_forward_seed_dev(const float* u, const float* gamma, const float* beta, int B, int P, int C,
                                    float p_drop, const uint64_t* seed_dev, float* z_out, float* gx_out, void* ws,
                                    size_t ws_bytes, void* stream);
int paella_grn_act_backward_seed_dev(const float* u, const float* gamma, const float* gx, const float* dz, int B,
                                     int P, int C, float p_drop, const uint64_t* seed_dev,
                                     float* du_out /* may be NULL */, float* dgamma_out /* may be NULL */,
                                     float* dbeta_out /* may be NULL */, void* ws, size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training ResBlock front (ABI 8, extended ADDITIVELY: no existing signature changes, the version stays 8): the
 * front of every ResBlock in train mode -- [cat with the skip ->] depthwise Conv2d(k 3, zero padding, groups C) ->
 * LayerNorm2d(C, no affine) (reference src/modules.py:46-47, 55-58) -- as one op, forward and backward
 * (paella_amd/csrc/dwconv_train.hip).  Everything fp32.
 *   x [B, H, W, C] NHWC; skip [B, H, W, C] NHWC or NULL; w [C, J, 3, 3] exactly as the parameter is stored, J = 2
 *   with a skip, else 1; bias [C].  Output channel g reads concatenated channels J g + j; concatenated channel
 *   cc < C lives in x, cc >= C in skip at cc - C -- the concatenation is never formed.
 *   Forward:  a = conv3x3_zero_pad(xcat, w) + bias;  per position mean and var over C (two-pass, as the eval
 *     kernel), rstd = 1 / sqrt(var + eps);  y = (a - mean) rstd, NHWC.  rstd_out [B H W] (one float per position)
 *     is, with x, skip, w and y, ALL the backward needs.
 *   Backward for a given dy [B, H, W, C]:  c1 = mean_c dy,  c2 = mean_c(dy y),  da = rstd (dy - c1 - y c2);
 *     dbias[c] = sum_pos da;  dw[c][j][ky][kx] = sum_pos da[pos][c] xcat[pos + (ky - 1, kx - 1)][J c + j];
 *     dxcat[pos][J c + j] = sum_taps da[pos - (ky - 1, kx - 1)][c] w[c][j][ky][kx], split back into dx and dskip;
 *     positions outside the image contribute 0.  dx, dskip, dw (in the parameter's layout) and dbias are WRITTEN,
 *     not accumulated into; each may be NULL and is then not computed; with all four NULL nothing is launched.
 * Shapes: C a multiple of 4 in 4...8192, with a skip a multiple of 8 in 8...4096 (the eval kernel's limits);
 * B, H, W >= 1 with B H W <= 2^31 - 1; 3 x 3 only; every tensor and the workspace 16-byte aligned; eps positive
 * and finite; all element offsets are 64-bit.  Anything else, a NULL required pointer, dskip without skip:
 * PAELLA_ERR_ARG; a workspace too small for the call: PAELLA_ERR_WORKSPACE -- both before anything is enqueued.
 * Workspace (no state between calls, no initialisation):
 *   forward : the weights repacked to [J, 9, C]: 36 J C bytes rounded up to 256 -- which is what
 *             paella_dwconv_ln_train_workspace_bytes(1, 1, 1, C, has_skip) returns, and all the forward asks for;
 *   backward: da [B, H, W, C] (one activation tensor, rounded up to 256 bytes) and, when the positions fall into
 *             more than one strip, the per-strip partials of dw and dbias, strips x (9 J + 1) x C floats in two
 *             blocks rounded up to 256.  A strip is max(8 (9 J + 1), ceil(B H W / 1024)) positions, so the partials
 *             stay under a quarter of an activation tensor: at most 1.25 activation tensors + 768 bytes in all.
 *   paella_dwconv_ln_train_workspace_bytes returns the larger of the two; one workspace of that size serves both.
 * Deterministic: no float atomics, no tickets, every combine is a launch.  y, dx and dskip of a sample depend
 * neither on its index nor on the batch around it; dw and dbias are summed in fp64 inside a strip of consecutive
 * positions (b, y, x ascending) and the strips in ascending order, strips fixed by (B, H, W, C, J) alone.
 * No allocation, no synchronisation, capturable in a graph.
 * ---------------------------------------------------------------------------------------------- */
size_t paella_dwconv_ln_train_workspace_bytes(int B, int H, int W, int C, int has_skip); /* 0 for an unsupported shape */
int paella_dwconv_ln_train_forward(const float* x, const float* skip /* may be NULL */, const float* w,
                                   const float* bias, int B, int H, int W, int C, float eps, float* y_out,
                                   float* rstd_out, void* ws, size_t ws_bytes, void* stream);
int paella_dwconv_ln_train_backward(const float* x, const float* skip /* may be NULL */, const float* w,
                                    const float* y, const float* rstd, const float* dy, int B, int H, int W, int C,
                                    float* dx_out /* may be NULL */, float* dskip_out /* may be NULL */,
                                    float* dw_out /* may be NULL */, float* dbias_out /* may be NULL */, void* ws,
                                    size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training attention (ABI 8, extended ADDITIVELY: no existing signature changes, the version stays 8): the attention
 * core of every AttnBlock in train mode -- softmax(Q K^T / sqrt(D)) V with dropout on the probabilities
 * (nn.MultiheadAttention between its in- and out-projection; reference src/modules.py:7-19) -- as one op, forward and
 * backward, flash style (paella_amd/csrc/attn_train.hip).  Everything fp32.
 *   q [B, P, .], k and v [B, L, .]: head h occupies floats [h D, (h + 1) D) of a row; rows are ld* floats apart
 *   (each ld* a multiple of 4 and at least nhead D) and sample b starts at b * rows * ld -- so k and v may be the two
 *   halves of one [B, L, 2 nhead D] projection output, and dk and dv may be written into one such buffer, without a
 *   copy.  o and do are dense [B, P, nhead D]; lse is [B, nhead, P].
 *   Forward:  s = q k^T / sqrt(D);  lse = logsumexp_j s, computed over key tiles with the running row maximum
 *     subtracted;  pr = exp(s - lse);  o = (keep pr / (1 - p_drop)) v.  o_out and lse_out are ALL the forward leaves:
 *     no [P, L] array is ever in global memory.
 *   Dropout: p_drop == 0 draws nothing, the seed is then without meaning.  Otherwise element e, the flat index in
 *     [B, nhead, P, L4] with L4 = 4 ceil(L / 4) (a quad never straddles a row; 64-bit arithmetic), takes word e & 3
 *     of philox4x32(seed ^ 0xe7037ed1a0b428db, counter (e >> 2, 0)) and is kept iff (word >> 8) * 2^-24 >= p_drop;
 *     the scale is the one fp32 division 1.0f / (1.0f - p_drop).  The backward regenerates the mask from (seed, e).
 *   Backward for a given do:  delta_i = sum_c do_ic o_ic (= sum_j pr_ij keep_ij dpd_ij / (1 - p): why o is an
 *     input);  dpd = do v^T;  dp = keep dpd / (1 - p);  ds = pr (dp - delta);  dq = ds k / sqrt(D);
 *     dk = ds^T q / sqrt(D);  dv = (keep pr / (1 - p))^T do.  pr is recomputed from q, k and lse.  dq, dk and dv
 *     are WRITTEN, not accumulated into (the floats of a row outside [0, nhead D) are left untouched); each may be
 *     NULL and is then not computed; with all three NULL nothing is launched.
 * Shapes: D a multiple of 16 in 16...128; B and nhead in 1...65535; P and L in 1...2^20; B nhead P <= 2^31 - 1;
 * nhead D <= 2^24; every pointer and the workspace 16-byte aligned; 0 <= p_drop < 1; all element offsets are 64-bit.
 * Anything else or a NULL required pointer (q, k, v, o, lse, do): PAELLA_ERR_ARG; a workspace smaller than
 * paella_attn_train_workspace_bytes: PAELLA_ERR_WORKSPACE -- both before anything is enqueued.
 * Kernels: every workgroup is one wave that owns 16 queries (forward, dq) or 16 keys (dk / dv) of one
 * (sample, head) and walks the other axis in ascending 16-wide tiles on the exact-fp32 matrix cores; both backward
 * kernels recompute the score tile; delta comes from a pre-pass.  Tails in P and L are bounds, not padding.
 * Workspace: delta [B, nhead, P], rounded up to 256 bytes (the forward uses none of it); no state between calls, no
 * initialisation.  Deterministic: no float atomics, no tickets, no sum crosses a workgroup; the order of every sum
 * is fixed by (B, nhead, P, L, D) alone, and what a (sample, head) computes depends on that sample's data only.
 * No allocation, no synchronisation, capturable in a graph.
 * ---------------------------------------------------------------------------------------------- */
size_t paella_attn_train_workspace_bytes(int B, int nhead, int P, int L, int D); /* 0 for an unsupported shape */
int paella_attn_train_forward(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv, int B,
                              int nhead, int P, int L, int D, float p_drop, uint64_t seed, float* o_out,
                              float* lse_out, void* ws, size_t ws_bytes, void* stream);
int paella_attn_train_backward(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                               const float* o, const float* lse, const float* d_o, int B, int nhead, int P, int L,
                               int D, float p_drop, uint64_t seed, float* dq_out /* may be NULL */, int lddq,
                               float* dk_out /* may be NULL */, int lddk, float* dv_out /* may be NULL */, int lddv,
                               void* ws, size_t ws_bytes, void* stream);
/* The same two calls with the seed read from DEVICE memory (added ADDITIVELY, the version stays 8), as
 * paella_grn_act_*_seed_dev: seed_dev is one 8-byte aligned 64-bit word, required when p_drop > 0, loaded by the
 * drawing kernels when they run; a word that holds s gives the bits of the by-value call with seed = s. */
int paella_attn_train_forward_seed_dev(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                                       int B, int nhead, int P, int L, int D, float p_drop, const uint64_t* seed_dev,
                                       float* o_out, float* lse_out, void* ws, size_t ws_bytes, void* stream);
int paella_attn_train_backward_seed_dev(const float* q, int ldq, const float* k, int ldk, const float* v, int ldv,
                                        const float* o, const float* lse, const float* d_o, int B, int nhead, int P,
                                        int L, int D, float p_drop, const uint64_t* seed_dev,
                                        float* dq_out /* may be NULL */, int lddq, float* dk_out /* may be NULL */,
                                        int lddk, float* dv_out /* may be NULL */, int lddv, void* ws,
                                        size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training timestep modulation (ABI 8, extended ADDITIVELY: no existing signature changes, the version stays 8): the
 * joint between two blocks of a `C T [A]` unit in train mode -- the residual add that ends a ResBlock or a
 * FeedForwardBlock, the TimestepBlock (reference src/modules.py:99-106) and the LayerNorm2d(C, no affine) that
 * begins an AttnBlock or a FeedForwardBlock -- as one op, forward and backward (paella_amd/csrc/mod_train.hip).
 * Everything fp32.
 *   x [B, P, C] (NHWC, P = H W positions per sample); residual [B, P, C] or NULL; ab [B, 2C], the mapper's output
 *   as it is: a = ab[:, :C], b = ab[:, C:].
 *   Forward:  u = x + residual;  x' = fma(u, 1 + a, b) -> xp_out [B, P, C].  With z_out and rstd_out (both, or
 *     both NULL): per position mean and var of x' over C (two-pass, as the eval kernel), rstd = 1 / sqrt(var + eps),
 *     z = (x' - mean) rstd -> z_out [B, P, C], rstd_out [B, P].  With x, residual, ab and z, rstd is ALL the
 *     backward needs: u, x' and 1 + a are recomputed.
 *   Backward for given dxp and / or dz (each may be NULL = no gradient arrived there; at least one is required, and
 *     dz needs z and rstd):  g = dxp + rstd (dz - mean_c dz - z mean_c(dz z));  dx = g (1 + a), which is the gradient
 *     of x and of residual alike;  dab[b][c] = sum_p g u,  dab[b][C + c] = sum_p g,  with u = x + residual
 *     recomputed -- never x' divided by 1 + a, so a = -1 is an ordinary value.  dx_out [B, P, C] and dab_out
 *     [B, 2C] are WRITTEN, not accumulated into; each may be NULL and is then not computed; with both NULL nothing
 *     is launched.
 * Shapes: C a multiple of 4 in 4...8192; P in 1...2^20; B in 1...65535; B P <= 2^31 - 1; every tensor and the
 * workspace 16-byte aligned; eps positive and finite; all element offsets are 64-bit.  Anything else or a NULL
 * required pointer (x, ab, xp_out; x, ab in the backward): PAELLA_ERR_ARG; a workspace too small for the call:
 * PAELLA_ERR_WORKSPACE -- both before anything is enqueued.
 * Kernels: forward one launch, one wave per position.  Backward with dz: g (kept in the workspace) and dx, one wave
 * per position; then the sums over the positions of ONE sample in strips of max(16, ceil(P / 1024)) consecutive
 * positions, carried in fp64, one fp32 partial per (sample, strip, channel); then the partials in ascending strip
 * order.  Backward without dz: the summing pass reads dxp, x and residual once and writes dx as well.  A sample of one
 * strip is summed straight into dab_out.
 * Workspace (no state between calls, no initialisation; the forward uses none of it and checks none):
 *   has_layernorm (the backward is given dz): g [B, P, C] rounded up to 256 bytes; then, when P exceeds one strip,
 *   the partials B x strips x 2C floats rounded up to 256 bytes.  A supported shape that needs nothing is sized 256.
 * Deterministic: no float atomics, no tickets, every combine is a launch.  The strips depend on (P, C) alone, and
 * every value of a sample -- its row of dab included -- depends on that sample only: its bits depend neither on its
 * index nor on the batch around it.  No allocation, no synchronisation, capturable in a graph.
 * ---------------------------------------------------------------------------------------------- */
size_t paella_mod_ln_train_workspace_bytes(int B, int P, int C, int has_layernorm); /* 0 for an unsupported shape */
int paella_mod_ln_train_forward(const float* x, const float* residual /* may be NULL */, const float* ab, int B, int P,
                                int C, float eps, float* xp_out, float* z_out /* may be NULL */,
                                float* rstd_out /* NULL with z_out */, void* ws, size_t ws_bytes, void* stream);
int paella_mod_ln_train_backward(const float* x, const float* residual /* may be NULL */, const float* ab,
                                 const float* z /* may be NULL without dz */, const float* rstd /* NULL with z */,
                                 const float* dxp /* may be NULL */, const float* dz /* may be NULL */, int B, int P,
                                 int C, float* dx_out /* may be NULL */, float* dab_out /* may be NULL */, void* ws,
                                 size_t ws_bytes, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Training optimizer step (ABI 8, extended ADDITIVELY: no existing signature changes, the version stays 8): the
 * global gradient norm, `clip_grad_norm_`'s coefficient and the AdamW update of every parameter tensor as THREE
 * launches over a table of tensors (paella_amd/csrc/optim.hip).  The other half of a training iteration
 * (reference src/train.py:66-69: clip_grad_norm_(model.parameters(), 1.0); optimizer.step() with optim.AdamW).
 * Everything fp32; the sums and the per-tensor scalars in fp64.
 *   rows: n_tensors rows of paella_adamw_tensor that the DEVICE can read, one per parameter tensor, in the
 *   caller's order.  g == NULL: the tensor has no gradient this step and is skipped entirely (not in the norm, p /
 *   m / v / its step untouched; m and v may then be NULL too).  Work is cut into chunks of PAELLA_ADAMW_CHUNK
 *   consecutive elements of ONE tensor: row i owns the chunks [chunk_begin[i], chunk_begin[i + 1]) (the last row up
 *   to n_chunks), ceil(n / PAELLA_ADAMW_CHUNK) of them, or none for a row without a gradient or without elements.
 *   chunk_begin starts at 0 and ascends.  A kernel finds the row of a chunk by binary search over the table.
 *   Launch 1 (sumsq): per chunk, the sum of g^2 with every element widened to fp64 BEFORE it is squared (1e25 is an
 *     ordinary value), in a fixed order (lane, wave shuffle, LDS): one double per chunk into the workspace.
 *   Launch 2 (finalize, one workgroup): total = the chunk sums in ascending chunk order in a fixed tree;
 *     norm_out[0] = (float)sqrt(total);  finite = isfinite(total);
 *     coef = max_norm > 0 ? min(1, max_norm / (sqrt(total) + 1e-6)) : 1      (clip_grad_norm_'s formula with its clamp)
 *     and, in paella_adamw_step only, for every row with a gradient when finite: steps[i] += 1 (float32, the dtype
 *     torch's fused AdamW keeps on the device), step_size = lr / (1 - beta1^step) and 1 / sqrt(1 - beta2^step) in fp64.
 *   Launch 3 (update; paella_adamw_step only): when !finite every workgroup returns at once -- p, m, v and steps
 *     stay bit for bit (torch would write NaN into the weights).  Otherwise per element, torch's single-tensor
 *     AdamW arithmetic in fp32 with IEEE sqrt and division:
 *       g' = g coef;  p *= 1 - lr wd;  m += (g' - m)(1 - beta1);  v = v beta2 + (1 - beta2) g' g';
 *       p -= step_size m / (sqrt(v) rsqrt_bc2 + eps)
 *     g coef alone is formed in fp64 from the fp64 coef and rounded once (coef = 1 leaves g as it is): a coef rounded
 *     to fp32 would put one relative error into every element of every tensor.
 *     1 - lr wd, 1 - beta1 and 1 - beta2 are formed in fp64 from the row and rounded once.  g is never written.
 *   16-byte vectors where every pointer of a tensor is 16-byte aligned, else a scalar path for that tensor (uniform
 *   per chunk); all element offsets are 64-bit.
 * Arguments: rows, norm_out, the workspace (and steps [n_tensors] float32 in paella_adamw_step) are required;
 * n_tensors >= 0; n_chunks >= 0, and 0 when there is no tensor; max_norm not NaN (<= 0: no clipping; the norm is
 * still computed and a non-finite step still skipped).  Anything else: PAELLA_ERR_ARG; a workspace smaller than
 * paella_adamw_workspace_bytes(n_tensors, n_chunks) or not 16-byte aligned: PAELLA_ERR_WORKSPACE / PAELLA_ERR_ARG --
 * before anything is enqueued.  The plan: a table the HOST can read as well (pinned host memory) is checked before
 * anything is enqueued -- chunk_begin not ascending from 0 within n_chunks, or n < 0: PAELLA_ERR_ARG.  A table in
 * device memory cannot be read without a synchronisation: the finalize launch makes the same check there and a
 * plan that fails it is treated as a non-finite step (norm_out = NaN, nothing updated), and no kernel reads or
 * writes an element outside [0, n) of a row whatever chunk_begin says.
 * Workspace (no state between calls, no initialisation): 256 bytes of header (coef, finite), 2 doubles per tensor,
 * one double per chunk, each part rounded up to 256 bytes.
 * Deterministic: no atomics; the bits of the norm and of everything downstream are a function of the tensors'
 * sizes, order and values only -- not of the grid or of the scheduling.  No allocation, no synchronisation.
 * ---------------------------------------------------------------------------------------------- */
#define PAELLA_ADAMW_CHUNK 4096 /* elements per chunk; a multiple of 1024 */
typedef struct paella_adamw_tensor {
    float* p;            /* [n] the parameter */
    const float* g;      /* [n] its gradient; NULL = none this step */
    float* m;            /* [n] exp_avg */
    float* v;            /* [n] exp_avg_sq */
    int64_t n;           /* elements */
    int64_t chunk_begin; /* index of the tensor's first chunk */
    double lr, beta1, beta2, eps, weight_decay; /* as the caller's Python floats: 1 - beta2 must not be formed from an fp32 beta2 */
} paella_adamw_tensor;
int paella_adamw_chunk_elems(void); /* PAELLA_ADAMW_CHUNK */
size_t paella_adamw_workspace_bytes(int n_tensors, int64_t n_chunks); /* 0 for negative arguments */
int paella_adamw_grad_norm(const paella_adamw_tensor* rows, int n_tensors, int64_t n_chunks, float* norm_out, void* ws,
                           size_t ws_bytes, void* stream); /* launches 1 and 2; reads g and n only, touches no step */
int paella_adamw_step(const paella_adamw_tensor* rows, int n_tensors, int64_t n_chunks, float max_norm, float* steps,
                      float* norm_out, void* ws, size_t ws_bytes, void* stream);

/* ----------------------------------------------------------------------------------------------
 * Training linear on bf16 operands (ABI 8, extended ADDITIVELY: no existing signature changes, the version stays 8):
 * y = x W^T + b of a linear layer in train mode, forward and backward, with the three GEMMs on the bf16 matrix
 * cores and fp32 accumulation (paella_amd/csrc/linear_train.hip).  OPT-IN and OUTSIDE the fp32 parity contract, as
 * paella_unet_set_precision(1) is for inference.  Every tensor of the interface is fp32; only the GEMM operands are
 * rounded (round to nearest even, the bits of torch's .bfloat16()), into the workspace.
 *   x [M, K], w [N, K], bias [N] or NULL, y [M, N], dy [M, N], dx [M, K], dw [N, K], db [N], all dense row-major.
 *   Forward:  y = bf16(x) bf16(w)^T + bias            (products exact in fp32, fp32 accumulation, one rounding for the bias)
 *   Backward: dx = bf16(dy) bf16(w);  dw = bf16(dy)^T bf16(x);  db = the column sums of the UNROUNDED dy, carried in
 *     fp64 and rounded once.  dx_out, dw_out and db_out are WRITTEN, not accumulated into; each may be NULL and is then
 *     neither packed for nor computed (dx alone needs neither x nor the transposed dy); with all three NULL nothing is
 *     launched.  w is required for dx, x for dw.
 *   paella_pack_bf16: the pass that makes the operands, alone.  src [rows, cols] fp32 is read exactly once and any
 *     subset of out_rowmajor [rows, cols] bf16, out_transposed [cols, rows] bf16 and colsum [cols] fp32 (NULL = absent;
 *     at least one) is written.  Its workspace holds the column sums' partials and is needed only when colsum is given
 *     and the tensor is more than one strip: one double per (strip, column), rounded up to 256 bytes.
 * Shapes: M, N and K (rows and cols) positive multiples of 64 up to 65535 x 64 (the pack's grid) -- each of them is the reduction of one of
 * the three GEMMs; every tensor and the workspace 16-byte aligned.  Anything else or a NULL required pointer:
 * PAELLA_ERR_ARG; a workspace too small for the call: PAELLA_ERR_WORKSPACE -- both before anything is enqueued.
 * Launches.  Forward: pack x (row-major), pack w (row-major), the GEMM with the bias in its epilogue.  Backward:
 * one pack over dy (row-major for dx, transposed for dw, column sums for db, whichever are wanted) and, beyond one
 * strip, the finalize of the column sums; pack x (transposed) for dw; pack w (transposed) for dx; the dgrad GEMM; the
 * wgrad GEMM.  The GEMMs are gemm.hip's bf16-operand kernels under their own launch rules.
 * Workspace (no state between calls; `direction` 0 = forward, 1 = backward; `wants` = 1 dx | 2 dw | 4 db, ignored
 * by the forward): a split-K region first (the ticket header of PAELLA workspaces plus 64 MiB of slab space; the
 * entry points zero the header on the stream themselves before their first GEMM, nothing else is initialised), then
 * the bf16 operands of the call, each rounded up to 256 bytes, then the partials of db.
 * Deterministic: no float atomics in the pack; strips of max(4, ceil(row tiles / 256)) row tiles of 64 rows, a
 * function of the row count alone, partials added in ascending strip order.  The GEMMs combine split reductions in
 * a fixed order (gemm.hip).  No allocation, no synchronisation.
 * ---------------------------------------------------------------------------------------------- */
size_t paella_linear_train_workspace_bytes(int M, int N, int K, int direction, int wants); /* 0 for an unsupported shape */
int paella_linear_train_forward(const float* x, const float* w, const float* bias /* may be NULL */, float* y_out, int M,
                                int N, int K, void* ws, size_t ws_bytes, void* stream);
int paella_linear_train_backward(const float* x /* may be NULL without dw_out */, const float* w /* may be NULL without dx_out */,
                                 const float* dy, float* dx_out /* may be NULL */, float* dw_out /* may be NULL */,
                                 float* db_out /* may be NULL */, int M, int N, int K, void* ws, size_t ws_bytes,
                                 void* stream);
int paella_pack_bf16(const float* src, int rows, int cols, unsigned short* out_rowmajor /* may be NULL */,
                     unsigned short* out_transposed /* may be NULL */, float* colsum /* may be NULL */, void* ws,
                     size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training seed table (ABI 8, extended ADDITIVELY: no existing signature changes, the version stays 8): the
 * dropout seeds of one training forward as DEVICE words, re-derived by one launch per iteration -- what lets a
 * captured iteration (paella_amd.training.GraphTrainStep) draw other masks at every replay
 * (paella_amd/csrc/train_seeds.hip).
 *   state: uint64 [2 + n_sites] = (base, iteration, word[0 .. n_sites)), 8-byte aligned device memory the caller
 *   owns and initialises (base = the run's seed, iteration = 0).
 *   paella_train_seeds_advance: ONE launch.  iteration += 1, then for every site s
 *     word[s] = w0 | w1 << 32,  (w0, w1, ., .) = philox4x32(key = base, counter (s, iteration))
 *   with the Philox4x32-10 of the sampling tail and the dropout masks.  word[s] is what a *_seed_dev call takes.
 * n_sites in 1...paella_train_seeds_max_sites() (65536); anything else, a NULL or misaligned state: PAELLA_ERR_ARG
 * before anything is enqueued.  One workgroup walks the sites, so the count is read by every thread before one of
 * them replaces it.  No allocation, no synchronisation, capturable in a graph.
 * ---------------------------------------------------------------------------------------------- */
int paella_train_seeds_max_sites(void);
int paella_train_seeds_advance(uint64_t* state, int n_sites, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training token stem (ABI 8, extended ADDITIVELY: no existing signature changes, the version stays 8): the top of
 * the train-mode network -- token embedding, LayerNorm(c_in, no affine), PixelUnshuffle(patch) and the change to
 * NHWC rows (reference src/modules.py:126-131, 271) -- as one op, forward and backward
 * (paella_amd/csrc/embed_train.hip).
 *   tokens int64 [B, H, W]; table fp32 [num_labels, c_in] (in_mapper.0.weight as it is); rows fp32
 *   [B, H/p, W/p, c_in p^2], p = patch, with
 *     rows[b, oy, ox, c p^2 + dy p + dx] = LN(table[clamp(tokens[b, oy p + dy, ox p + dx])])[c]
 *   -- the A operand of the 1x1 convolution behind it as a linear.  A token outside [0, num_labels) is clamped into
 *   the range in BOTH directions, as the inference kernel clamps it: the clamped row is read and receives the
 *   gradient, and no address outside the table is ever formed.
 *   Forward:  the inference engine's own launch (one wave per output position; mean and var two-pass,
 *     rstd = 1 / sqrt(var + eps)), so rows_out holds the engine's bits.  Nothing is kept for the backward.
 *   Backward for given d_rows (the layout of rows):  with G[l] = the sum, over the positions n whose clamped token
 *     is l, of the de-interleaved gradient row at n, and xhat[l], rstd[l] recomputed from table[l] as the forward
 *     forms them:  dtable[l] = rstd ((G - mean_c G) - xhat mean_c(G xhat)).  The LayerNorm backward is linear in the
 *     arriving gradient for a fixed row, so summing first and applying it once per label is the same function as
 *     applying it per position.  dtable_out [num_labels, c_in] is WRITTEN, not accumulated into: the row of a label
 *     that no token holds is written as exact zeros, whatever the table holds there.
 * Shapes: patch 1 or 2, dividing H and W; c_in a multiple of 4 in 4...1024; num_labels in 1...65536;
 * B (H / patch) (W / patch) <= 2^31 - 1; every tensor and the workspace 16-byte aligned; eps positive and finite; all
 * element offsets are 64-bit.  Anything else or a NULL required pointer (tokens, table, rows_out; tokens, table,
 * d_rows, dtable_out): PAELLA_ERR_ARG; a workspace smaller than paella_embed_ln_train_workspace_bytes:
 * PAELLA_ERR_WORKSPACE -- both before anything is enqueued.
 * Kernel: the backward is ONE launch.  A workgroup owns min(256, 4096 / c_in) consecutive labels with their sums in
 * LDS, carried in fp64; it scans all B H W tokens in ascending order, 1024 at a time, compacts the positions that
 * hold one of its labels in ascending order and adds their gradient rows in that order, one thread per channel; then
 * one wave per label applies the LayerNorm backward -- statistics included in fp64, rounded once -- and stores.  The grid is ceil(num_labels / labels per
 * workgroup): a function of the shape.  Known weak spot: one label's additions are one workgroup's, serially -- when
 * most tokens share a label, that workgroup does most of the B H W row additions of the call.
 * Workspace: none is used; a supported shape is sized 256 bytes (0 says "unsupported") and both entry points check
 * what they are given.  Nothing in it is read.
 * Deterministic: no atomics of any kind, no tickets; every sum is one thread's, in ascending position order: the
 * bits of dtable are a function of (tokens, table, d_rows, shape) alone.  No allocation, no synchronisation, no
 * data-dependent launch geometry, capturable in a graph.
 * ---------------------------------------------------------------------------------------------- */
size_t paella_embed_ln_train_workspace_bytes(int B, int H, int W, int c_in, int patch,
                                             int num_labels); /* 0 for an unsupported shape */
int paella_embed_ln_train_forward(const int64_t* tokens, const float* table, int B, int H, int W, int c_in, int patch,
                                  int num_labels, float eps, float* rows_out, void* ws, size_t ws_bytes, void* stream);
int paella_embed_ln_train_backward(const int64_t* tokens, const float* table, const float* d_rows, int B, int H, int W,
                                   int c_in, int patch, int num_labels, float eps, float* dtable_out, void* ws,
                                   size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PAELLA_HIP_H */
