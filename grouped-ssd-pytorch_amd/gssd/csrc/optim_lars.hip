// LARS (You et al. 2017: torch.optim.SGD's rule with the decayed gradient scaled per tensor) and LAMB (You et al. 2020: Adam's moments
// with a per-tensor ratio on the full update) on the chunk scheme of optim.hip / optim_adam.hip.  Both need a 2-norm over ONE tensor
// before any element of that tensor may move, and a tensor spreads over up to ~1 150 workgroups, so a step is two launches:
//
//   LARS  lars_norm_kernel   reads p, g: one 16-byte record {sum g^2, sum p^2} per chunk (squares and sums in fp64), and per workgroup
//                            the fp64 partial sum of g^2 over ITS chunks -- the <= 1024 partials clip_coef() consumes, so the global norm
//                            of the clip costs no launch of its own;
//         lars_step_kernel   one workgroup per chunk: re-adds the records of its item, forms r, updates p and buf in place.
//                            7 memory passes (read p, g | read g, p, buf; write p, buf), clip or no clip.
//   LAMB  lamb_kernel, moments phase   updates m, v in place, forms u from the fp32 m, v it STORES and the unchanged p, leaves
//                                      {sum u^2, sum p^2} per chunk;
//         lamb_kernel, update phase    re-adds the records of its item, forms r, re-forms u from the stored m, v and p -- the same
//                                      function on the same fp32 inputs, so bit for bit the u whose norm was taken -- and p -= lr r u.
//                            10 passes (read g, p, m, v; write m, v | read p, m, v; write p); storing u instead would cost 10 as well
//                            (write u | read u) and a fourth state-sized array.  The clip's norm is gssd_grad_sumsq_f32, a launch before.
//
// How the records reach the update: every workgroup of an item adds the item's records item_chunk0[i] .. item_chunk0[i + 1] itself, thread
// k taking the records k, k + 256, ..., then block_sum2 -- the same order in every workgroup of the item and in every run, so all chunks
// of a tensor apply the same r to the bit, without a ticket, an atomic or a grid-wide wait.  r is formed in fp64 and rounded to fp32 once.
// A norm that is exactly 0 gives r = 1; a NaN or inf norm gives a NaN r, which propagates as a NaN gradient does.
//
// Param groups beyond HYPER_CAP take further launches.  The phases of LAMB ride together: launch k runs the moments phase of the groups
// [8k, 8k + 8) and the update phase of [8k - 8, 8k), whose records the launch before left -- one more launch per 8 groups, not two.
//
// p, buf, m and v are read and written through the same pointer: none of the pointers below is __restrict__.
#include "optim_util.h"

namespace {

struct NormRec {                        // 16 bytes per chunk
    double sumsq_a;                     // LARS: of g (unclipped);  LAMB: of u
    double sumsq_p;
};
static_assert(sizeof(NormRec) == 16, "gssd_lars_workspace_bytes");

__device__ __forceinline__ double sumsq_share(const float (&x)[NE + 1]) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k <= NE; ++k) s += (double)x[k] * (double)x[k];
    return s;
}

// The sums of the records [c0, c1) of one item, the same values (to the bit) in every thread of every workgroup that asks
__device__ __forceinline__ void fold_records(const NormRec* recs, const int* item_chunk0, const int item, const int n_chunks, double& sa,
                                             double& sp, double (*red)[4]) {
    int c0 = item_chunk0[item], c1 = item_chunk0[item + 1];
    c0 = c0 < 0 ? 0 : c0, c1 = c1 > n_chunks ? n_chunks : c1;      // (a bad prefix reads no record that is not there)
    sa = 0.0, sp = 0.0;
    for (int c = c0 + (int)threadIdx.x; c < c1; c += THREADS) {
        const NormRec r = recs[c];
        sa += r.sumsq_a, sp += r.sumsq_p;
    }
    block_sum2(sa, sp, red);
}

// ---------------------------------------------------------------------------------------------- LARS
__global__ __launch_bounds__(THREADS) void lars_norm_kernel(const gssd_sgd_item* items, const gssd_sgd_chunk* chunks, const int n_chunks,
                                                            NormRec* recs, double* partials) {
    __shared__ double red[2][2][4];     // two barriers' worth: chunk k + 2 writes what chunk k read only behind chunk k + 1's barrier
    double part = 0.0;
    int par = 0;
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x, par ^= 1) {
        const gssd_sgd_chunk ch = chunks[c];
        const gssd_sgd_item it = items[ch.item];
        const int len = chunk_len(it, ch);
        float gx[NE + 1], px[NE + 1];
        load_share(as_global(it.g) + ch.off, len, gx);      // all loads of the thread issue here ...
        load_share(as_global(it.p) + ch.off, len, px);
        double sg = sumsq_share(gx), sp = sumsq_share(px);  // ... before the first use
        block_sum2(sg, sp, red[par]);
        if (threadIdx.x == 0) recs[c] = NormRec{sg, sp};
        part += sg;
    }
    if (partials != nullptr && threadIdx.x == 0) partials[blockIdx.x] = part;
}

__global__ __launch_bounds__(THREADS) void lars_step_kernel(const gssd_sgd_item* items, const gssd_sgd_chunk* chunks, const int n_chunks,
                                                            const int* item_chunk0, const int* item_slot, const NormRec* recs,
                                                            const GroupArgs<gssd_lars_hyper> hy, const double* partials, int n_partials,
                                                            float max_norm, float* norm_out, float* ratio_out) {
    __shared__ double red[4];
    __shared__ double red2[2][4];
    const float c = max_norm >= 0.f ? clip_step(partials, n_partials, max_norm, red, blockIdx.x == 0 && hy.g0 == 0, norm_out) : 1.f;
    const gssd_sgd_chunk ch = chunks[blockIdx.x];
    const gssd_sgd_item it = items[ch.item];
    const int gi = group_slot(hy, it.group);
    if (gi < 0) return;                                   // a group of another launch
    const gssd_lars_hyper gh = hy.h[gi];
    double sg, sp;
    fold_records(recs, item_chunk0, ch.item, n_chunks, sg, sp, red2);
    float r = 1.f;
    if (gh.adapt != 0) {
        const double wn = sqrt(sp), gn = (double)c * sqrt(sg);         // ||g'|| = c ||g||
        if (wn != 0.0 && gn != 0.0) r = (float)(gh.trust_coefficient * wn / (gn + gh.weight_decay * wn + gh.eps));
    }
    if (ch.off == 0 && threadIdx.x == 0) ratio_out[item_slot ? item_slot[ch.item] : ch.item] = r;
    momentum_chunk<true>(it, ch, c, momentum_of(gh, it, r));
}

// ---------------------------------------------------------------------------------------------- LAMB
struct Lamb : Moments {
    float bc1;                          // 1 - beta1^step, rounded once (1 without bias correction)
};

__device__ __forceinline__ Lamb lamb_consts(const gssd_lamb_hyper& gh, const long long step) {
    double bc1;
    Lamb h;
    static_cast<Moments&>(h) = moments_consts(gh, step, gh.bias_correction != 0, bc1);
    h.bc1 = (float)bc1;
    return h;
}

// The update direction from fp32 p, m, v.  BOTH phases call this: no contraction may be left to the compiler's view of the call site, so
// the one multiply-add is an explicit fma and the rest are single correctly rounded operations.
__device__ __forceinline__ float lamb_u(const float p, const float m, const float v, const Lamb& h) {
#pragma clang fp contract(off)
    const float den = sqrtf(v) / h.sqrt_bc2 + h.eps;
    const float q = (m / h.bc1) / den;
    return fmaf(h.wd, p, q);
}

__device__ __forceinline__ void lamb_moments(const float p, const float g, float& m, float& v, const float c, const Lamb& h, double& su,
                                             double& sp) {
    moments_update(m, v, c * g, h);
    const float u = lamb_u(p, m, v, h);
    su += (double)u * (double)u;
    sp += (double)p * (double)p;
}

__device__ __forceinline__ void lamb_moments_vec(const gfloat4* p4, const gfloat4* g4, gfloat4* m4, gfloat4* v4, int nv, const float c,
                                                 const Lamb& h, double& su, double& sp) {
    f32x4 pv[NV], gv[NV], mv[NV], vv[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int i = threadIdx.x + k * THREADS;
        if (i < nv) {
            pv[k] = p4[i];
            gv[k] = g4[i];
            mv[k] = m4[i];
            vv[k] = v4[i];
        }
    }
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int i = threadIdx.x + k * THREADS;
        if (i < nv) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float me = mv[k][e], ve = vv[k][e];
                lamb_moments(pv[k][e], gv[k][e], me, ve, c, h, su, sp);
                mv[k][e] = me, vv[k][e] = ve;
            }
            m4[i] = mv[k];
            v4[i] = vv[k];
        }
    }
}

// mo: the groups whose moments phase this launch runs;  up: the groups whose update phase it runs (their records are a launch old).
// MO / UP: whether the launch has such groups at all -- a step over up to eight groups runs <true, false> and then <false, true>, each
// with the registers of its own phase alone; <true, true> is the launch in the middle of a step over more than eight groups.
template <bool MO, bool UP>
__global__ __launch_bounds__(THREADS) void lamb_kernel(const gssd_adam_item* items, const gssd_sgd_chunk* chunks, const int n_chunks,
                                                       const int* item_chunk0, const int* item_slot, NormRec* recs,
                                                       const GroupArgs<gssd_lamb_hyper> mo, const GroupArgs<gssd_lamb_hyper> up,
                                                       const long long t, const double* partials, int n_partials, float max_norm,
                                                       float* norm_out, float* ratio_out) {
    __shared__ double red[4];
    __shared__ double red2[2][4];
    const gssd_sgd_chunk ch = chunks[blockIdx.x];
    const gssd_adam_item it = items[ch.item];
    const int gm = MO ? group_slot(mo, it.group) : -1, gu = UP ? group_slot(up, it.group) : -1;
    const bool in_mo = gm >= 0, in_up = gu >= 0;
    const bool writes_norm = MO && blockIdx.x == 0 && mo.g0 == 0;
    float c = 1.f;
    if (MO && max_norm >= 0.f && (in_mo || writes_norm))    // (the same answer in every thread of the workgroup)
        c = clip_step(partials, n_partials, max_norm, red, writes_norm, norm_out);
    if (!in_mo && !in_up) return;                         // a group of other launches
    gfloat* p = as_global(it.p) + ch.off;
    gfloat* m = as_global(it.m) + ch.off;
    gfloat* v = as_global(it.v) + ch.off;
    const int len = chunk_len(it, ch);
    if constexpr (MO) {
        if (in_mo) {
            const Lamb h = lamb_consts(mo.h[gm], t - it.t0);
            const gfloat* g = as_global(it.g) + ch.off;
            double su = 0.0, sp = 0.0;
            int done = 0;
            if (aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v)) {
                const int nv = len >> 2;
                lamb_moments_vec((const gfloat4*)p, (const gfloat4*)g, (gfloat4*)m, (gfloat4*)v, nv, c, h, su, sp);
                done = nv << 2;
            }
            for (int i = done + threadIdx.x; i < len; i += THREADS) {
                float me = m[i], ve = v[i];
                lamb_moments(p[i], g[i], me, ve, c, h, su, sp);
                m[i] = me, v[i] = ve;
            }
            block_sum2(su, sp, red2);
            if (threadIdx.x == 0) recs[blockIdx.x] = NormRec{su, sp};
            return;
        }
    }
    if constexpr (UP) {
        // the chunk's loads issue first: they do not depend on r, and the fold of the records and the fp64 constants run under them
        gfloat4* p4 = (gfloat4*)p;
        const gfloat4* m4 = (const gfloat4*)m;
        const gfloat4* v4 = (const gfloat4*)v;
        const int nv = (aligned16(p) && aligned16(m) && aligned16(v)) ? len >> 2 : 0;
        f32x4 pv[NV], mv[NV], vv[NV];
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int i = threadIdx.x + k * THREADS;
            if (i < nv) {
                pv[k] = p4[i];
                mv[k] = m4[i];
                vv[k] = v4[i];
            }
        }
        double su, sp;
        fold_records(recs, item_chunk0, ch.item, n_chunks, su, sp, red2);
        const gssd_lamb_hyper gh = up.h[gu];
        const Lamb h = lamb_consts(gh, t - it.t0);
        float r = 1.f;
        if (gh.adapt != 0) {
            const double wn = sqrt(sp), un = sqrt(su);
            if (wn != 0.0 && un != 0.0) r = (float)(wn / un);
        }
        if (ch.off == 0 && threadIdx.x == 0) ratio_out[item_slot ? item_slot[ch.item] : ch.item] = r;
        const float lr_r = (float)(gh.lr * (double)r);
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            const int i = threadIdx.x + k * THREADS;
            if (i < nv) {
#pragma unroll
                for (int e = 0; e < 4; ++e) pv[k][e] = fmaf(-lr_r, lamb_u(pv[k][e], mv[k][e], vv[k][e], h), pv[k][e]);
                p4[i] = pv[k];
            }
        }
        for (int i = (nv << 2) + threadIdx.x; i < len; i += THREADS) p[i] = fmaf(-lr_r, lamb_u(p[i], m[i], v[i], h), p[i]);
    }
}

}  // namespace

extern "C" long long gssd_lars_workspace_bytes(int n_chunks) { return n_chunks > 0 ? (long long)sizeof(NormRec) * n_chunks : 0; }

extern "C" int gssd_lars_step_f32(const gssd_sgd_item* items, const gssd_sgd_chunk* chunks, int n_chunks, const int* item_chunk0,
                                  const int* item_slot, const gssd_lars_hyper* hyper, int n_groups, void* workspace, double* partials,
                                  int n_partials, float max_norm, float* norm_out, float* ratio_out, gssd_stream_t stream) {
    GSSD_CHECK_ARG(items && chunks && n_chunks > 0 && item_chunk0 && hyper && n_groups > 0 && workspace && ratio_out);
    GSSD_CHECK_ARG(((uintptr_t)workspace & 7) == 0);
    const bool clip = max_norm >= 0.f;
    const int blocks = sumsq_blocks(n_chunks);
    GSSD_CHECK_ARG(!clip || (partials && n_partials == blocks && norm_out));
    hipLaunchKernelGGL(lars_norm_kernel, dim3(blocks), dim3(THREADS), 0, as_stream(stream), items, chunks, n_chunks, (NormRec*)workspace,
                       clip ? partials : (double*)nullptr);
    GSSD_CHECK_LAUNCH();
    return for_group_batches(hyper, n_groups, [&](const GroupArgs<gssd_lars_hyper>& hy) {
        hipLaunchKernelGGL(lars_step_kernel, dim3(n_chunks), dim3(THREADS), 0, as_stream(stream), items, chunks, n_chunks, item_chunk0,
                           item_slot, (const NormRec*)workspace, hy, (const double*)partials, n_partials, max_norm, norm_out, ratio_out);
    });
}

extern "C" int gssd_lamb_step_f32(const gssd_adam_item* items, const gssd_sgd_chunk* chunks, int n_chunks, const int* item_chunk0,
                                  const int* item_slot, const gssd_lamb_hyper* hyper, int n_groups, int64_t t, void* workspace,
                                  const double* partials, int n_partials, float max_norm, float* norm_out, float* ratio_out,
                                  gssd_stream_t stream) {
    GSSD_CHECK_ARG(items && chunks && n_chunks > 0 && item_chunk0 && hyper && n_groups > 0 && workspace && ratio_out);
    GSSD_CHECK_ARG(((uintptr_t)workspace & 7) == 0);
    const bool clip = max_norm >= 0.f;
    GSSD_CHECK_ARG(!clip || (partials && n_partials > 0 && norm_out));
    GroupArgs<gssd_lamb_hyper> prev = {};                 // the groups whose moments phase the launch before ran (none yet)
    for (int g0 = 0; g0 < n_groups || prev.ng > 0; g0 += HYPER_CAP) {
        const GroupArgs<gssd_lamb_hyper> mo = group_batch(hyper, n_groups, g0);
        auto kernel = mo.ng > 0 ? (prev.ng > 0 ? lamb_kernel<true, true> : lamb_kernel<true, false>) : lamb_kernel<false, true>;
        hipLaunchKernelGGL(kernel, dim3(n_chunks), dim3(THREADS), 0, as_stream(stream), items, chunks, n_chunks, item_chunk0, item_slot,
                           (NormRec*)workspace, mo, prev, (long long)t, partials, n_partials, max_norm, norm_out, ratio_out);
        GSSD_CHECK_LAUNCH();
        prev = mo;
    }
    return GSSD_OK;
}
