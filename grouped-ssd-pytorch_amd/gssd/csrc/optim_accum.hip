// Gradient accumulation over micro-batches (gssd.optim.GradAccumulator) on the chunk scheme of optim.hip: one workgroup per CHUNK-element
// chunk of ONE tensor pair, every pair of the model in ONE launch.  Pure streaming: an accumulated element costs 12 bytes (read acc, g;
// write acc), the first of a cycle 8 (acc is not read, so fresh storage needs no zero-fill launch), a scale-only one 8.
//
// Per element, with w32 = (float)w -- the expression forms are part of the contract, results are bitwise reproducible:
//     FIRST item        acc = w32 * g
//     otherwise         acc = fmaf(w32, g, acc)
//     with `finalize`   then acc = acc * inv,  inv = (float)(1.0 / W_new)       (the same launch; an item without src takes only this)
// W, the running sum of the weights, is an fp64 device scalar the host never reads: W_new = (reset ? 0 : W_prev) + (double)w32.  Every
// workgroup reads W_prev before it writes anything, and the same launch leaves W_new there by the ticket of optim_avg.hip: a workgroup
// that has issued all its stores takes a ticket (atomic add on a word the accumulator owns, zero between launches), and the one whose
// ticket says that every other workgroup has taken its own -- so has read W_prev long before -- stores W_new and puts the ticket word
// back to 0.  No workgroup waits for another, nothing depends on dispatch order or on the grid being resident.
// IEEE semantics throughout: W_new == 0 gives inv = inf and inf / NaN elements, as a division by zero does in torch.
//
// acc is read and written through the same pointer: none of the pointers below is __restrict__.
#include "optim_util.h"

namespace {

typedef __attribute__((address_space(1))) unsigned gu32;
typedef __attribute__((address_space(1))) double gf64;

enum { ADD = 0, FIRST = 1, SCALE = 2 };                    // what a chunk does before the optional division

template <int MODE, bool FIN>
__device__ __forceinline__ float accum(const float acc, const float g, const float w, const float inv) {
    float r = MODE == FIRST ? w * g : MODE == ADD ? fmaf(w, g, acc) : acc;
    if (FIN) r = r * inv;
    return r;
}

// One chunk.  Where acc and g are 16-byte aligned: rounds of NV vectors per thread and array with all loads of a round issued before
// its first use (optim_avg.hip's lerp_vec); the rest (or all of it) element by element.
template <int MODE, bool FIN>
__device__ __forceinline__ void accum_chunk(gfloat* a, const gfloat* g, const int len, const float w, const float inv) {
    constexpr bool RD_A = MODE != FIRST, RD_G = MODE != SCALE;
    int done = 0;
    if (aligned16(a) && (!RD_G || aligned16(g))) {
        gfloat4* a4 = (gfloat4*)a;
        const gfloat4* g4 = (const gfloat4*)g;
        const int nv = len >> 2;
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        int i = threadIdx.x;
        // a full chunk is one round of NV vectors per thread and array, no bounds check inside; a short one goes vector by vector
        for (; i + (NV - 1) * THREADS < nv; i += NV * THREADS) {
            f32x4 av[NV], gv[NV];
#pragma unroll
            for (int k = 0; k < NV; ++k) av[k] = RD_A ? a4[i + k * THREADS] : zero, gv[k] = RD_G ? g4[i + k * THREADS] : zero;
#pragma unroll
            for (int k = 0; k < NV; ++k) {
#pragma unroll
                for (int e = 0; e < 4; ++e) av[k][e] = accum<MODE, FIN>(av[k][e], gv[k][e], w, inv);
                a4[i + k * THREADS] = av[k];
            }
        }
        for (; i < nv; i += THREADS) {
            f32x4 av = RD_A ? a4[i] : zero;
            const f32x4 gv = RD_G ? g4[i] : zero;
#pragma unroll
            for (int e = 0; e < 4; ++e) av[e] = accum<MODE, FIN>(av[e], gv[e], w, inv);
            a4[i] = av;
        }
        done = nv << 2;
    }
    for (int i = done + threadIdx.x; i < len; i += THREADS) a[i] = accum<MODE, FIN>(RD_A ? a[i] : 0.f, RD_G ? g[i] : 0.f, w, inv);
}

template <bool FIN>
__device__ __forceinline__ void accum_item(const gssd_accum_item& it, const gssd_sgd_chunk& ch, const float w, const float inv) {
    const int len = chunk_len(it, ch);
    gfloat* a = as_global(it.dst) + ch.off;
    const bool has_src = __builtin_amdgcn_readfirstlane(it.src != nullptr);
    const bool first = __builtin_amdgcn_readfirstlane(it.flags & GSSD_ACCUM_FIRST) != 0;
    if (!has_src) {
        if (FIN) accum_chunk<SCALE, FIN>(a, nullptr, len, w, inv);      // (without the division a scale-only item has nothing to do)
    } else if (first) {
        accum_chunk<FIRST, FIN>(a, as_global(it.src) + ch.off, len, w, inv);
    } else {
        accum_chunk<ADD, FIN>(a, as_global(it.src) + ch.off, len, w, inv);
    }
}

__global__ __launch_bounds__(THREADS) void grad_accumulate_kernel(const gssd_accum_item* items, const gssd_sgd_chunk* chunks, const double w_val,
                                                                  const void* w_dev, const int flags, gf64* wsum, gu32* ticket) {
    // the weight sum BEFORE this launch, in every thread: a vector load that bypasses the L1 (not the scalar path)
    const double w_prev = __hip_atomic_load(wsum, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    float w32 = (float)w_val;
    if (w_dev != nullptr) w32 = (flags & GSSD_ACCUM_W_F32) ? *(const float*)w_dev : (float)*(const double*)w_dev;
    const double w_new = ((flags & GSSD_ACCUM_RESET) ? 0.0 : w_prev) + (double)w32;
    const gssd_sgd_chunk ch = chunks[blockIdx.x];
    const gssd_accum_item it = items[ch.item];
    static_assert(CHUNK == NV * 4 * THREADS, "a full chunk is one round");
    if (flags & GSSD_ACCUM_FINALIZE) {
        accum_item<true>(it, ch, w32, (float)(1.0 / w_new));
    } else {
        accum_item<false>(it, ch, w32, 1.f);
    }
    // The ticket.  A wave that used w_prev had it in a register before it issued its first store, and it issued its stores before it
    // reached this barrier; thread 0, which needs it for w_new whatever its chunk did, waits for its own load below.  So this workgroup's
    // reads of the sum lie before its add, and the add that returns the last ticket lies behind the adds of all the others.
    __syncthreads();
    if (threadIdx.x == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (t == gridDim.x - 1) {                          // every other workgroup has taken its ticket, so has read the sum
            __hip_atomic_store(wsum, w_new, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

}  // namespace

extern "C" int gssd_grad_accumulate_f32(const gssd_accum_item* items, const gssd_sgd_chunk* chunks, int n_chunks, double w, const void* w_dev,
                                        int flags, double* weight_sum, uint32_t* ticket, gssd_stream_t stream) {
    GSSD_CHECK_ARG(items && chunks && n_chunks > 0 && weight_sum && ticket);
    GSSD_CHECK_ARG(w_dev != nullptr || w >= 0.0);          // a by-value weight: not negative, and a NaN is refused
    GSSD_CHECK_ARG((flags & ~(GSSD_ACCUM_W_F32 | GSSD_ACCUM_RESET | GSSD_ACCUM_FINALIZE)) == 0);
    hipLaunchKernelGGL(grad_accumulate_kernel, dim3(n_chunks), dim3(THREADS), 0, as_stream(stream), items, chunks, w, w_dev, flags,
                       (gf64*)weight_sum, (gu32*)ticket);
    GSSD_CHECK_LAUNCH();
    return GSSD_OK;
}
