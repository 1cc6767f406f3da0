// The averaged copy of a model's weights (EMA, or torch's equal SWA average) next to its optimizer, on the chunk scheme of optim.hip: one
// workgroup per CHUNK-element chunk of ONE tensor pair, every pair of the model in ONE launch.  Pure streaming: an averaged element costs
// 12 bytes (read a, b; write a), a copied 4-byte element 8, a copied int64 16.
//
// The number of updates so far lives on the device (torch's `n_averaged` buffer) and the host never reads it.  Every workgroup reads n
// before it writes anything; n == 0 turns every LERP item into a copy (torch's first update), the SWA rule takes its weight 1 / (n + 1)
// from it.  The same launch leaves n + 1 there: a workgroup that has issued all its stores takes a ticket (atomic add on a word the
// table owns, zero between launches), and the one whose ticket says that every other workgroup has taken its own -- so has read n long
// before -- stores n + 1 and puts the ticket word back to 0.  No workgroup waits for another, nothing depends on dispatch order or on
// the grid being resident, and a captured launch replays from the state the previous replay left.
//
// a is read and written through the same pointer: none of the pointers below is __restrict__.
#include "optim_util.h"

namespace {

typedef __attribute__((address_space(1))) unsigned gu32;
typedef __attribute__((address_space(1))) u32x4 gu32x4;
typedef __attribute__((address_space(1))) long long gi64;

// torch's lerp (ATen/native/Lerp.h): w = 0 leaves a, w = 1 gives b, to the bit
__device__ __forceinline__ float lerp(const float a, const float b, const float w, const float omw) {
    const float d = b - a;
    return w < 0.5f ? a + w * d : b - d * omw;
}

// NV (optim_util.h) 16-byte vectors per thread and array in flight: a full fp32 chunk is one round of them.
// a4[i] = lerp(a4[i], b4[i]) for i < nv.  Rounds of NV vectors per thread with all loads of a round issued before its first use and
// no bounds check inside; what is left of a short chunk one vector at a time.
__device__ __forceinline__ void lerp_vec(gfloat4* a4, const gfloat4* b4, const int nv, const float w, const float omw) {
    int i = threadIdx.x;
    for (; i + (NV - 1) * THREADS < nv; i += NV * THREADS) {
        f32x4 av[NV], bv[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) av[k] = a4[i + k * THREADS], bv[k] = b4[i + k * THREADS];
#pragma unroll
        for (int k = 0; k < NV; ++k) {
#pragma unroll
            for (int e = 0; e < 4; ++e) av[k][e] = lerp(av[k][e], bv[k][e], w, omw);
            a4[i + k * THREADS] = av[k];
        }
    }
    for (; i < nv; i += THREADS) {
        f32x4 av = a4[i];
        const f32x4 bv = b4[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) av[e] = lerp(av[e], bv[e], w, omw);
        a4[i] = av;
    }
}

// a4[i] = b4[i] for i < nv, in the same rounds
__device__ __forceinline__ void copy_vec(gu32x4* a4, const gu32x4* b4, const int nv) {
    int i = threadIdx.x;
    for (; i + (NV - 1) * THREADS < nv; i += NV * THREADS) {
        u32x4 v[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) v[k] = b4[i + k * THREADS];
#pragma unroll
        for (int k = 0; k < NV; ++k) a4[i + k * THREADS] = v[k];
    }
    for (; i < nv; i += THREADS) a4[i] = b4[i];
}

__global__ __launch_bounds__(THREADS) void avg_update_kernel(const gssd_avg_item* items, const gssd_sgd_chunk* chunks, const float w_ema,
                                                             gi64* count, gu32* ticket) {
    // the count BEFORE this launch, in every thread: a vector load that bypasses the L1 (not the scalar path)
    const long long n = __hip_atomic_load(count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const gssd_sgd_chunk ch = chunks[blockIdx.x];
    const gssd_avg_item it = items[ch.item];
    const int kind = __builtin_amdgcn_readfirstlane(it.kind);
    const int len = chunk_len(it, ch);
    static_assert(CHUNK == NV * 4 * THREADS, "a full chunk is one round");
    if (kind == GSSD_AVG_LERP && n != 0) {
        const float w = w_ema < 0.f ? 1.f / (float)(n + 1) : w_ema;
        const float omw = 1.f - w;
        gfloat* a = as_global((float*)it.dst) + ch.off;
        const gfloat* b = as_global((const float*)it.src) + ch.off;
        int done = 0;
        if (aligned16(a) && aligned16(b)) {
            lerp_vec((gfloat4*)a, (const gfloat4*)b, len >> 2, w, omw);
            done = len & ~3;
        }
        for (int i = done + threadIdx.x; i < len; i += THREADS) a[i] = lerp(a[i], b[i], w, omw);
    } else {
        // a copy in 4-byte words -- also every LERP item of a first update.  An int64 element is two words (its tensors are 8-byte
        // aligned, and the chunk's offset counts elements)
        const int words = kind == GSSD_AVG_COPY64 ? 2 : 1;
        gu32* a = (gu32*)it.dst + ch.off * words;
        const gu32* b = (const gu32*)it.src + ch.off * words;
        const int nw = len * words;
        int done = 0;
        if ((((uintptr_t)a | (uintptr_t)b) & 15) == 0) {
            copy_vec((gu32x4*)a, (const gu32x4*)b, nw >> 2);
            done = nw & ~3;
        }
        for (int i = done + threadIdx.x; i < nw; i += THREADS) a[i] = b[i];
    }
    // The ticket.  A wave that used n had it in a register before it issued its first store, and it issued its stores before it reached
    // this barrier; thread 0, which needs n for n + 1 even where its chunk is a copy, waits for its own load below.  So this workgroup's
    // reads of n lie before its add, and the add that returns the last ticket lies behind the adds of all the others.
    __syncthreads();
    if (threadIdx.x == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (t == gridDim.x - 1) {                          // every other workgroup has taken its ticket, so has read n
            __hip_atomic_store(count, n + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

}  // namespace

extern "C" int gssd_avg_update_f32(const gssd_avg_item* items, const gssd_sgd_chunk* chunks, int n_chunks, float w, int64_t* n_averaged,
                                   uint32_t* ticket, gssd_stream_t stream) {
    GSSD_CHECK_ARG(items && chunks && n_chunks > 0 && n_averaged && ticket);
    GSSD_CHECK_ARG(w <= 1.f);                              // [0, 1]: EMA with this weight of the source; negative: SWA; a NaN is refused
    hipLaunchKernelGGL(avg_update_kernel, dim3(n_chunks), dim3(THREADS), 0, as_stream(stream), items, chunks, w, (gi64*)n_averaged,
                       (gu32*)ticket);
    GSSD_CHECK_LAUNCH();
    return GSSD_OK;
}
