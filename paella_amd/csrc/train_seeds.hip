// Device-side seed table of a captured training iteration: the 64-bit dropout seeds of one forward live in device memory and are re-derived by ONE launch per
// iteration, so a graph replay draws other masks than the replay before it (the *_seed_dev entry points of grn_act.hip and attn_train.hip read their word).
//
//   state uint64 [2 + n] = (base, iteration, word[0 .. n));   advance:  iteration += 1,  word[s] = w0 | w1 << 32 of philox4x32(key = base, ctr_lo = s, ctr_hi = iteration)
//
// ONE workgroup walks the sites: every thread reads `iteration` before the barrier and one thread writes it back after, so no thread can see the new count where
// it wants the old one -- with more workgroups that would take a second launch or a ticket.  The table of a forward has some dozen words (56 at the 570M model); the 65536
// sites the entry point takes at most are 64 Philox calls per thread.  Plain 64-bit vector stores.
#include "common.h"
#include "philox.h"
#include "train_common.h"

namespace {

constexpr int kSeedThreads = 1024;
constexpr int kMaxSites = 65536;

__global__ __launch_bounds__(kSeedThreads) void train_seeds_advance_kernel(uint64_t* __restrict__ state, int n_sites) {
    const uint64_t base = state[0];
    const uint64_t it = state[1] + 1ull;
    __syncthreads();  // every thread holds the old count before it is replaced
    if (threadIdx.x == 0) state[1] = it;
    for (int s = threadIdx.x; s < n_sites; s += kSeedThreads) {
        uint32_t w[4];
        philox4x32(base, (uint64_t)s, it, w);
        state[2 + s] = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
    }
}

}  // namespace

extern "C" int paella_train_seeds_max_sites(void) { return kMaxSites; }

extern "C" int paella_train_seeds_advance(uint64_t* state, int n_sites, void* stream) {
    const char* who = "train_seeds_advance";
    if (n_sites < 1 || n_sites > kMaxSites) {
        paella_set_error("%s: n_sites = %d (1...%d)", who, n_sites, kMaxSites);
        return PAELLA_ERR_ARG;
    }
    if (!state || ((uintptr_t)state & 7) != 0) {
        paella_set_error("%s: state must be an 8-byte aligned device array of 2 + n_sites words", who);
        return PAELLA_ERR_ARG;
    }
    hipLaunchKernelGGL(train_seeds_advance_kernel, dim3(1), dim3(kSeedThreads), 0, (hipStream_t)stream, state, n_sites);
    LAUNCH_CHECK_RET();
    return PAELLA_OK;
}
