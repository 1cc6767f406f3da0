// The one core of the optimizer kernels (optim.hip: clip + SGD; optim_adam.hip: Adam / AdamW; optim_lars.hip: LARS / LAMB; optim_stats.hip:
// per-tensor statistics; optim_avg.hip: averaged weights; optim_accum.hip: gradient accumulation).  What they share lives here once:
//   the chunk scheme       CHUNK / THREADS / NV / NE, chunk_len, the global-address-space casts, load_share (a thread's share of a chunk);
//   the reductions         block_sum / block_sum2, bit-identical in every thread, and clip_coef / clip_step, the clip coefficient that
//                          every workgroup derives from the same partial sums;
//   group batching         GroupArgs<H> (HYPER_CAP groups' hyperparameters by value), for_group_batches on the host, group_slot on the device;
//   the update rules       momentum_update<RATIO> / momentum_chunk<RATIO> (SGD, and LARS with its ratio), moments_update / moments_consts
//                          (Adam and LAMB).  The expression forms are part of the contract: results are bitwise reproducible.
// Everything has internal linkage: each of the files carries its own copy.
#pragma once
#include "common.h"
#include "kernel_util.h"

namespace {

constexpr int CHUNK = 4096;            // elements per chunk: 4 x 16 bytes per thread and array
constexpr int THREADS = 256;
constexpr int NV = CHUNK / 4 / THREADS; // 16-byte vectors per thread and array of a full chunk
constexpr int NE = CHUNK / THREADS;     // elements per thread and array
constexpr int SUMSQ_MAX_BLOCKS = 1024; // partial sums every update workgroup re-reads (8 KiB, L2 resident)
constexpr int HYPER_CAP = 8;           // param groups per launch of a step kernel (by-value kernel argument)

// The tensors' pointers come out of the table, where the compiler cannot see their address space: saying "global" here turns the
// flat_load / flat_store it would emit (counted by vmcnt AND lgkmcnt) into global_load / global_store.
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) f32x4 gfloat4;
__device__ __forceinline__ gfloat* as_global(const float* p) { return (gfloat*)p; }

__device__ __forceinline__ bool aligned16(const gfloat* p) { return ((uintptr_t)p & 15) == 0; }

// sum over the workgroup, the same value (to the bit) in every thread: xor-butterfly inside the waves, then the four waves in order
__device__ __forceinline__ double block_sum(double v, double* red) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// block_sum for two sums behind one barrier (optim_lars.hip): red is [2][4]
__device__ __forceinline__ void block_sum2(double& a, double& b, double (*red)[4]) {
    a = wave_sum(a);
    b = wave_sum(b);
    if ((threadIdx.x & 63) == 0) red[0][threadIdx.x >> 6] = a, red[1][threadIdx.x >> 6] = b;
    __syncthreads();
    a = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    b = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
}

// elements of chunk `ch` of table item `it` (gssd_sgd_item / gssd_adam_item): CHUNK, or what is left of the tensor
template <class Item>
__device__ __forceinline__ int chunk_len(const Item& it, const gssd_sgd_chunk& ch) {
    const int64_t left = it.n - ch.off;
    return left < CHUNK ? (int)left : CHUNK;
}

// This thread's share of the `len` elements at a (null: none): NE of them and one of the up to three that a vector path leaves over.
// What the chunk does not have stays +0, which adds nothing to a sum of squares, a maximum of magnitudes or a count of non-finite values.
__device__ __forceinline__ void load_share(const gfloat* a, const int len, float (&x)[NE + 1]) {
#pragma unroll
    for (int k = 0; k <= NE; ++k) x[k] = 0.f;
    if (a == nullptr) return;
    if (aligned16(a)) {
        const gfloat4* a4 = (const gfloat4*)a;
        const int nv = len >> 2;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int i = threadIdx.x + k * THREADS;
            if (i < nv) {
                const f32x4 v = a4[i];
                x[4 * k] = v.x, x[4 * k + 1] = v.y, x[4 * k + 2] = v.z, x[4 * k + 3] = v.w;
            }
        }
        const int i = (nv << 2) + threadIdx.x;
        if (i < len) x[NE] = a[i];
    } else {
#pragma unroll
        for (int k = 0; k < NE; ++k) {
            const int i = threadIdx.x + k * THREADS;
            if (i < len) x[k] = a[i];
        }
    }
}

// torch.nn.utils.clip_grad_norm_: total = ||g||_2, coefficient = clamp(max_norm / (total + 1e-6), max = 1) -- a NaN stays a NaN
__device__ __forceinline__ float clip_coef(const double* partials, int n_partials, float max_norm, double* red, float& total) {
    double s = 0.0;
    for (int i = threadIdx.x; i < n_partials; i += THREADS) s += partials[i];
    s = block_sum(s, red);
    total = (float)sqrt(s);
    const float coef = max_norm / (total + 1e-6f);
    return coef > 1.f ? 1.f : coef;
}

// clip_coef, and the norm left in norm_out by the one workgroup that `writes_norm` names (block 0 of a step's first launch)
__device__ __forceinline__ float clip_step(const double* partials, int n_partials, float max_norm, double* red, const bool writes_norm,
                                           float* norm_out) {
    float total;
    const float c = clip_coef(partials, n_partials, max_norm, red, total);
    if (writes_norm && threadIdx.x == 0) norm_out[0] = total;
    return c;
}

inline int sumsq_blocks(int n_chunks) { return n_chunks < SUMSQ_MAX_BLOCKS ? n_chunks : SUMSQ_MAX_BLOCKS; }

// ---------------------------------------------------------------------------------------------- group batching
template <class H>
struct GroupArgs {
    H h[HYPER_CAP];
    int g0, ng;                        // this launch updates the groups [g0, g0 + ng)
};

// the groups [g0, g0 + HYPER_CAP) of a host array of n_groups, by value (none beyond the end)
template <class H>
inline GroupArgs<H> group_batch(const H* hyper, int n_groups, int g0) {
    GroupArgs<H> a = {};
    a.g0 = g0;
    a.ng = g0 >= n_groups ? 0 : (n_groups - g0 < HYPER_CAP ? n_groups - g0 : HYPER_CAP);
    for (int i = 0; i < a.ng; ++i) a.h[i] = hyper[g0 + i];
    return a;
}

// launch(batch) once per HYPER_CAP groups; the first launch error ends the walk
template <class H, class Launch>
inline int for_group_batches(const H* hyper, int n_groups, Launch launch) {
    for (int g0 = 0; g0 < n_groups; g0 += HYPER_CAP) {
        launch(group_batch(hyper, n_groups, g0));
        GSSD_CHECK_LAUNCH();
    }
    return GSSD_OK;
}

// index of `group` (an item's, the same in every thread of the workgroup) among the groups of this launch; negative: another launch's
template <class H>
__device__ __forceinline__ int group_slot(const GroupArgs<H>& a, const int group) {
    const int gi = __builtin_amdgcn_readfirstlane(group) - a.g0;
    return gi < a.ng ? gi : -1;
}

// ---------------------------------------------------------------------------------------------- the momentum rule (SGD, LARS)
struct Momentum {
    float lr, wd, mom, omd, r;         // omd = 1 - dampening; r: the trust ratio (RATIO only)
    bool nesterov, has_buf, first;
};

// the fields every momentum step fills alike, from gssd_sgd_hyper or gssd_lars_hyper and the item
template <class GH>
__device__ __forceinline__ Momentum momentum_of(const GH& gh, const gssd_sgd_item& it, const float r) {
    Momentum h;
    h.lr = (float)gh.lr, h.wd = (float)gh.weight_decay, h.mom = gh.momentum, h.omd = 1.f - gh.dampening, h.r = r;
    h.nesterov = gh.nesterov != 0, h.has_buf = it.buf != nullptr, h.first = (it.flags & 1) != 0;
    return h;
}

template <bool RATIO>
__device__ __forceinline__ void momentum_update(float& p, const float g, float& b, const float c, const Momentum& h) {
    const float cg = c * g;
    float d = h.wd != 0.f ? fmaf(h.wd, p, cg) : cg;
    if (RATIO) d = h.r * d;            // r = 1 (no adaptation): the product is exact, the rule is SGD's
    float step = d;
    if (h.has_buf) {
        b = h.first ? d : fmaf(h.mom, b, h.omd * d);
        step = h.nesterov ? fmaf(h.mom, b, d) : b;
    }
    p = fmaf(-h.lr, step, p);
}

// The update of one chunk.  Where p, g and buf are 16-byte aligned: NV vectors per thread and array, all loads of a thread issued
// before the first use; the rest (or all of it) element by element.  p and buf are read and written through the same pointer.
template <bool RATIO>
__device__ __forceinline__ void momentum_chunk(const gssd_sgd_item& it, const gssd_sgd_chunk& ch, const float c, const Momentum& h) {
    gfloat* p = as_global(it.p) + ch.off;
    const gfloat* g = as_global(it.g) + ch.off;
    gfloat* b = h.has_buf ? as_global(it.buf) + ch.off : nullptr;
    const int len = chunk_len(it, ch);
    const bool rd_b = h.has_buf && !h.first;
    int done = 0;
    if (aligned16(p) && aligned16(g) && aligned16(b)) {
        gfloat4* p4 = (gfloat4*)p;
        const gfloat4* g4 = (const gfloat4*)g;
        gfloat4* b4 = (gfloat4*)b;
        const int nv = len >> 2;
        f32x4 pv[NV], gv[NV], bv[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int i = threadIdx.x + k * THREADS;
            if (i < nv) {
                pv[k] = p4[i];
                gv[k] = g4[i];
                bv[k] = rd_b ? b4[i] : f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int i = threadIdx.x + k * THREADS;
            if (i < nv) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float pe = pv[k][e], be = bv[k][e];
                    momentum_update<RATIO>(pe, gv[k][e], be, c, h);
                    pv[k][e] = pe, bv[k][e] = be;
                }
                p4[i] = pv[k];
                if (h.has_buf) b4[i] = bv[k];
            }
        }
        done = nv << 2;
    }
    for (int i = done + threadIdx.x; i < len; i += THREADS) {
        float pv = p[i], bv = rd_b ? b[i] : 0.f;
        momentum_update<RATIO>(pv, g[i], bv, c, h);
        p[i] = pv;
        if (h.has_buf) b[i] = bv;
    }
}

// ---------------------------------------------------------------------------------------------- the moments (Adam, LAMB)
struct Moments {
    float b1, b2, omb1, omb2;          // omb = 1 - beta, rounded from the host's double
    float eps, wd, sqrt_bc2;           // sqrt(1 - beta2^step): formed in fp64, rounded once
};

// from gssd_adam_hyper or gssd_lamb_hyper; bc1 = 1 - beta1^step stays a double for the caller's own rounding point.  Without bias
// correction both corrections are 1.
template <class GH>
__device__ __forceinline__ Moments moments_consts(const GH& gh, const long long step, const bool bias_correction, double& bc1) {
    double bc2 = 1.0;
    bc1 = 1.0;
    if (bias_correction) bc1 = 1.0 - pow(gh.beta1, (double)step), bc2 = 1.0 - pow(gh.beta2, (double)step);
    Moments h;
    h.b1 = (float)gh.beta1, h.b2 = (float)gh.beta2, h.omb1 = gh.one_minus_beta1, h.omb2 = gh.one_minus_beta2;
    h.eps = gh.eps, h.wd = gh.weight_decay, h.sqrt_bc2 = (float)sqrt(bc2);
    return h;
}

// m = b1 m + (1 - b1) d;  v = b2 v + (1 - b2) d d
__device__ __forceinline__ void moments_update(float& m, float& v, const float d, const Moments& h) {
    m = fmaf(h.b1, m, h.omb1 * d);
    v = fmaf(h.omb2 * d, d, h.b2 * v);
}

}  // namespace
