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

struct AdamHyperArgs {
    gssd_adam_hyper h[HYPER_CAP];
    int g0, ng;                        // this launch updates the groups [g0, g0 + ng)
};

struct Adam {
    float b1, b2, omb1, omb2;          // omb = 1 - beta, rounded from the host's double
    float eps, wd, decay;              // decay = 1 - lr wd (AdamW)
    float step_size, sqrt_bc2;         // lr / (1 - beta1^step), sqrt(1 - beta2^step)
    bool amsgrad, decoupled;
};

__device__ __forceinline__ void adam_update(float& p, const float g, float& m, float& v, float& vmax, const float c, const Adam& h) {
    float d = c * g;
    if (h.decoupled) {
        p *= h.decay;
    } else if (h.wd != 0.f) {
        d = fmaf(h.wd, p, d);
    }
    m = fmaf(h.b1, m, h.omb1 * d);
    v = fmaf(h.omb2 * d, d, h.b2 * v);
    float vh = v;
    if (h.amsgrad) {
        vmax = (v > vmax || v != v) ? v : vmax;            // torch.maximum: a NaN wins
        vh = vmax;
    }
    const float den = sqrtf(vh) / h.sqrt_bc2 + h.eps;
    p = fmaf(-h.step_size, m / den, p);
}

// NV: 16-byte vectors per thread, known at compile time for a full chunk (all loads of a thread issue before the first use)
template <int NV>
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

__global__ __launch_bounds__(THREADS) void adam_step_kernel(const gssd_adam_item* items, const gssd_sgd_chunk* chunks, const AdamHyperArgs hy,
                                                            const long long t, const double* partials, int n_partials, float max_norm,
                                                            float* norm_out) {
    __shared__ double red[4];
    float c = 1.f;
    if (max_norm >= 0.f) {
        float total;
        c = clip_coef(partials, n_partials, max_norm, red, total);
        if (blockIdx.x == 0 && threadIdx.x == 0 && hy.g0 == 0) norm_out[0] = total;
    }
    const gssd_sgd_chunk ch = chunks[blockIdx.x];
    const gssd_adam_item it = items[ch.item];
    const int gi = __builtin_amdgcn_readfirstlane(it.group) - hy.g0;
    if (gi < 0 || gi >= hy.ng) return;                    // a group of another launch
    const gssd_adam_hyper gh = hy.h[gi];
    const double step = (double)(t - it.t0);
    const double bc1 = 1.0 - pow(gh.beta1, step), bc2 = 1.0 - pow(gh.beta2, step);
    Adam h;
    h.b1 = (float)gh.beta1, h.b2 = (float)gh.beta2, h.omb1 = gh.one_minus_beta1, h.omb2 = gh.one_minus_beta2;
    h.eps = gh.eps, h.wd = gh.weight_decay, h.decay = (float)(1.0 - gh.lr * (double)gh.weight_decay);
    h.step_size = (float)(gh.lr / bc1), h.sqrt_bc2 = (float)sqrt(bc2);
    h.amsgrad = gh.amsgrad != 0 && it.vmax != nullptr, h.decoupled = gh.decoupled != 0;
    gfloat* p = as_global(it.p) + ch.off;
    const gfloat* g = as_global(it.g) + ch.off;
    gfloat* m = as_global(it.m) + ch.off;
    gfloat* v = as_global(it.v) + ch.off;
    gfloat* x = h.amsgrad ? as_global(it.vmax) + ch.off : nullptr;
    const int len = chunk_len(it, ch);
    int done = 0;
    if (aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v) && aligned16(x)) {
        constexpr int NV = CHUNK / 4 / THREADS;
        const int nv = len >> 2;
        adam_vec<NV>((gfloat4*)p, (const gfloat4*)g, (gfloat4*)m, (gfloat4*)v, (gfloat4*)x, nv, c, h);
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
    for (int g0 = 0; g0 < n_groups; g0 += HYPER_CAP) {
        AdamHyperArgs hy = {};
        hy.g0 = g0;
        hy.ng = n_groups - g0 < HYPER_CAP ? n_groups - g0 : HYPER_CAP;
        for (int i = 0; i < hy.ng; ++i) hy.h[i] = hyper[g0 + i];
        hipLaunchKernelGGL(adam_step_kernel, dim3(n_chunks), dim3(THREADS), 0, as_stream(stream), items, chunks, hy, (long long)t, partials,
                           n_partials, max_norm, norm_out);
        GSSD_CHECK_LAUNCH();
    }
    return GSSD_OK;
}
