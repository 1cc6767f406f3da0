// Adam / AdamW (torch.optim.Adam's single-tensor rule, amsgrad included) on the chunk scheme of optim.hip: one workgroup per CHUNK-element
// chunk of ONE tensor, the clip coefficient re-derived from gssd_grad_sumsq_f32's partial sums in every workgroup (optim_util.h), p, m, v
// (and vmax) updated in place: 7 memory passes (read g, p, m, v; write p, m, v; 9 with amsgrad) + 1 for the norm.
//
// Step counts are per tensor in torch (a gradient that appears later starts its bias correction at step 1).  They travel as ONE integer:
// the launch takes the optimizer's launch count t by value, an item carries t0, its step is t - t0.  The bias corrections are formed per
// workgroup in fp64 from the groups' double lr / betas and rounded to fp32 once; the moments' weights 1 - beta come rounded from the host.
// m, v and vmax start as zeros: beta * 0 + (1 - beta) x is torch's first step, so no item needs a first-step flag.
//
// p, m, v and vmax are read and written through the same pointer: none of the pointers below is __restrict__.
#include "optim_util.h"

namespace {

struct Adam : Moments {
    float decay, step_size;            // 1 - lr wd (AdamW), lr / (1 - beta1^step)
    bool amsgrad, decoupled;
};

__device__ __forceinline__ void adam_update(float& p, const float g, float& m, float& v, float& vmax, const float c, const Adam& h) {
    float d = c * g;
    if (h.decoupled) {
        p *= h.decay;
    } else if (h.wd != 0.f) {
        d = fmaf(h.wd, p, d);
    }
    moments_update(m, v, d, h);
    float vh = v;
    if (h.amsgrad) {
        vmax = (v > vmax || v != v) ? v : vmax;            // torch.maximum: a NaN wins
        vh = vmax;
    }
    const float den = sqrtf(vh) / h.sqrt_bc2 + h.eps;
    p = fmaf(-h.step_size, m / den, p);
}

// all loads of a thread issue before the first use
__device__ __forceinline__ void adam_vec(gfloat4* p4, const gfloat4* g4, gfloat4* m4, gfloat4* v4, gfloat4* x4, int nv, const float c,
                                         const Adam& h) {
    f32x4 pv[NV], gv[NV], mv[NV], vv[NV], xv[NV];
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int i = threadIdx.x + k * THREADS;
        if (i < nv) {
            pv[k] = p4[i];
            gv[k] = g4[i];
            mv[k] = m4[i];
            vv[k] = v4[i];
            xv[k] = h.amsgrad ? x4[i] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        const int i = threadIdx.x + k * THREADS;
        if (i < nv) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float pe = pv[k][e], me = mv[k][e], ve = vv[k][e], xe = xv[k][e];
                adam_update(pe, gv[k][e], me, ve, xe, c, h);
                pv[k][e] = pe, mv[k][e] = me, vv[k][e] = ve, xv[k][e] = xe;
            }
            p4[i] = pv[k];
            m4[i] = mv[k];
            v4[i] = vv[k];
            if (h.amsgrad) x4[i] = xv[k];
        }
    }
}

__global__ __launch_bounds__(THREADS) void adam_step_kernel(const gssd_adam_item* items, const gssd_sgd_chunk* chunks,
                                                            const GroupArgs<gssd_adam_hyper> hy, const long long t, const double* partials,
                                                            int n_partials, float max_norm, float* norm_out) {
    __shared__ double red[4];
    const float c = max_norm >= 0.f ? clip_step(partials, n_partials, max_norm, red, blockIdx.x == 0 && hy.g0 == 0, norm_out) : 1.f;
    const gssd_sgd_chunk ch = chunks[blockIdx.x];
    const gssd_adam_item it = items[ch.item];
    const int gi = group_slot(hy, it.group);
    if (gi < 0) return;                                   // a group of another launch
    const gssd_adam_hyper gh = hy.h[gi];
    double bc1;
    Adam h;
    static_cast<Moments&>(h) = moments_consts(gh, t - it.t0, true, bc1);
    h.decay = (float)(1.0 - gh.lr * (double)gh.weight_decay), h.step_size = (float)(gh.lr / bc1);
    h.amsgrad = gh.amsgrad != 0 && it.vmax != nullptr, h.decoupled = gh.decoupled != 0;
    gfloat* p = as_global(it.p) + ch.off;
    const gfloat* g = as_global(it.g) + ch.off;
    gfloat* m = as_global(it.m) + ch.off;
    gfloat* v = as_global(it.v) + ch.off;
    gfloat* x = h.amsgrad ? as_global(it.vmax) + ch.off : nullptr;
    const int len = chunk_len(it, ch);
    int done = 0;
    if (aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v) && aligned16(x)) {
        const int nv = len >> 2;
        adam_vec((gfloat4*)p, (const gfloat4*)g, (gfloat4*)m, (gfloat4*)v, (gfloat4*)x, nv, c, h);
        done = nv << 2;
    }
    for (int i = done + threadIdx.x; i < len; i += THREADS) {
        float pe = p[i], me = m[i], ve = v[i], xe = h.amsgrad ? x[i] : 0.f;
        adam_update(pe, g[i], me, ve, xe, c, h);
        p[i] = pe, m[i] = me, v[i] = ve;
        if (h.amsgrad) x[i] = xe;
    }
}

}  // namespace

extern "C" int gssd_adam_step_f32(const gssd_adam_item* items, const gssd_sgd_chunk* chunks, int n_chunks, const gssd_adam_hyper* hyper,
                                  int n_groups, int64_t t, const double* partials, int n_partials, float max_norm, float* norm_out,
                                  gssd_stream_t stream) {
    GSSD_CHECK_ARG(items && chunks && n_chunks > 0 && hyper && n_groups > 0);
    const bool clip = max_norm >= 0.f;
    GSSD_CHECK_ARG(!clip || (partials && n_partials > 0 && norm_out));
    return for_group_batches(hyper, n_groups, [&](const GroupArgs<gssd_adam_hyper>& hy) {
        hipLaunchKernelGGL(adam_step_kernel, dim3(n_chunks), dim3(THREADS), 0, as_stream(stream), items, chunks, hy, (long long)t, partials,
                           n_partials, max_norm, norm_out);
    });
}
