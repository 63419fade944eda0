// Host-side scaffold of the training ops (loss.hip, grn_act.hip, dwconv_train.hip): workspace layout and argument checks that every entry point makes the same
// way, and the strip rule of the ops that sum over positions.  Host helpers only -- no __device__ code lives here, so a change cannot move a kernel's code.
#pragma once
#include "common.h"
#include "../../include/paella_hip.h"

namespace train {

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }  // NULL (an output that is not wanted, no skip) counts as aligned

template <class... T>
inline bool all_aligned16(const T*... p) { return (aligned16(p) && ...); }

// `names` reads "u, gamma, beta, z and gx"
inline int check_required(const char* who, bool all_given, const char* names) {
    if (all_given) return PAELLA_OK;
    paella_set_error("%s: %s are required", who, names);
    return PAELLA_ERR_ARG;
}

template <class... T>
inline int check_tensors_aligned16(const char* who, const T*... p) {
    if (all_aligned16(p...)) return PAELLA_OK;
    paella_set_error("%s: every tensor must be 16-byte aligned", who);
    return PAELLA_ERR_ARG;
}

// the seed word of the *_seed_dev forms of the dropout ops: required where a mask is drawn, and a uint64 sits on 8 bytes
inline int check_seed_dev(const char* who, float p_drop, const uint64_t* seed_dev) {
    if (!(p_drop > 0.f) || (seed_dev && ((uintptr_t)seed_dev & 7) == 0)) return PAELLA_OK;
    paella_set_error("%s: seed_dev must be an 8-byte aligned device word when p_drop > 0", who);
    return PAELLA_ERR_ARG;
}

// The message is "<who>: workspace of <ws_bytes> bytes, <asks> <need><tail>": `asks` names the sizing function or the call, `tail` whatever follows the figure.
inline int check_workspace_size(const char* who, const void* ws, size_t ws_bytes, size_t need, const char* asks, const char* tail = "") {
    if (ws && ws_bytes >= need) return PAELLA_OK;
    paella_set_error("%s: workspace of %zu bytes, %s %zu%s", who, ws ? ws_bytes : (size_t)0, asks, need, tail);
    return PAELLA_ERR_WORKSPACE;
}

// ... and, for the ops that move 16-byte vectors through it, its alignment
inline int check_workspace(const char* who, const void* ws, size_t ws_bytes, size_t need, const char* asks, const char* tail = "") {
    const int rc = check_workspace_size(who, ws, ws_bytes, need, asks, tail);
    if (rc != PAELLA_OK) return rc;
    if (aligned16(ws)) return PAELLA_OK;
    paella_set_error("%s: the workspace must be 16-byte aligned", who);
    return PAELLA_ERR_ARG;
}

// The strip rule: n rows (positions) are summed in strips of `rows` consecutive ones, one partial per strip, the partials then added in ascending strip order.
// A strip has at least min_rows rows (which bounds the partials by a fraction of the tensor) and there are at most max_strips of them (which bounds the loop
// over the partials).  A function of its arguments only: the strips fix the summation order and hence the bits.
struct Strips {
    int rows, count;
};

inline Strips plan_strips(int64_t n, int64_t min_rows, int max_strips) {
    int64_t rows = min_rows;
    const int64_t floor_rows = (n + max_strips - 1) / max_strips;
    if (rows < floor_rows) rows = floor_rows;
    return {(int)rows, (int)((n + rows - 1) / rows)};
}

}  // namespace train
