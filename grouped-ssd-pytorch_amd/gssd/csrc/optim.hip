// The optimizer step of the reference driver (train_lesion_multiphase_v2.py:252-253: clip_grad_norm_ then SGD.step() with momentum,
// weight decay and a second learning-rate group) as two launches over a device table of tensors: gssd_grad_sumsq_f32 leaves one fp64
// partial sum of g^2 per workgroup, gssd_sgd_step_f32 (or, stand-alone, gssd_grad_scale_clip_f32) adds them up again in EVERY workgroup
// -- same order everywhere, so every workgroup holds the same clip coefficient to the bit and no grid-wide hand-off is needed -- and
// updates p and buf in place: 5 memory passes (read g, p, buf; write p, buf) + 1 for the norm, where the ATen foreach form makes 11 + 3.
//
// Work is cut into chunks of CHUNK elements of ONE tensor (the host lists them: gssd/optim.py), one workgroup per chunk in the update
// kernels, so the 2.4 M-element DCN weight and the one-element sigma load the machine alike.  A chunk starts at a multiple of CHUNK
// elements, so its alignment is that of the tensors' base pointers.
//
// p and buf are read and written through the same pointer: none of the pointers below is __restrict__.
#include "optim_util.h"

namespace {

__global__ __launch_bounds__(THREADS) void grad_sumsq_kernel(const gssd_sgd_item* items, const gssd_sgd_chunk* chunks, int n_chunks,
                                                             double* partials) {
    __shared__ double red[4];
    double acc = 0.0;
    for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {
        const gssd_sgd_chunk ch = chunks[c];
        const gssd_sgd_item it = items[ch.item];
        const gfloat* g = as_global(it.g) + ch.off;
        const int len = chunk_len(it, ch);
        int done = 0;
        if (aligned16(g)) {
            const gfloat4* g4 = (const gfloat4*)g;
            const int nv = len >> 2;
#pragma unroll 4
            for (int i = threadIdx.x; i < nv; i += THREADS) {
                const f32x4 v = g4[i];
                acc += (double)v.x * (double)v.x + (double)v.y * (double)v.y + ((double)v.z * (double)v.z + (double)v.w * (double)v.w);
            }
            done = nv << 2;
        }
        for (int i = done + threadIdx.x; i < len; i += THREADS) acc += (double)g[i] * (double)g[i];
    }
    const double s = block_sum(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(THREADS) void sgd_step_kernel(const gssd_sgd_item* items, const gssd_sgd_chunk* chunks,
                                                           const GroupArgs<gssd_sgd_hyper> hy, const double* partials, int n_partials,
                                                           float max_norm, float* norm_out) {
    __shared__ double red[4];
    const float c = max_norm >= 0.f ? clip_step(partials, n_partials, max_norm, red, blockIdx.x == 0 && hy.g0 == 0, norm_out) : 1.f;
    const gssd_sgd_chunk ch = chunks[blockIdx.x];
    const gssd_sgd_item it = items[ch.item];
    const int gi = group_slot(hy, it.group);
    if (gi < 0) return;                                   // a group of another launch
    momentum_chunk<false>(it, ch, c, momentum_of(hy.h[gi], it, 1.f));
}

__global__ __launch_bounds__(THREADS) void grad_scale_clip_kernel(const gssd_sgd_item* items, const gssd_sgd_chunk* chunks,
                                                                  const double* partials, int n_partials, float max_norm, float* norm_out) {
    __shared__ double red[4];
    const float c = clip_step(partials, n_partials, max_norm, red, blockIdx.x == 0, norm_out);
    const gssd_sgd_chunk ch = chunks[blockIdx.x];
    const gssd_sgd_item it = items[ch.item];
    gfloat* g = as_global(it.g) + ch.off;                 // (the table's gradients are plain device memory: this kernel writes them)
    const int len = chunk_len(it, ch);
    int done = 0;
    if (aligned16(g)) {
        gfloat4* g4 = (gfloat4*)g;
        const int nv = len >> 2;
#pragma unroll 4
        for (int i = threadIdx.x; i < nv; i += THREADS) g4[i] = g4[i] * c;
        done = nv << 2;
    }
    for (int i = done + threadIdx.x; i < len; i += THREADS) g[i] = g[i] * c;
}

}  // namespace

extern "C" int gssd_optim_chunk_elems(void) { return CHUNK; }

extern "C" int gssd_optim_sumsq_blocks(int n_chunks) { return n_chunks > 0 ? sumsq_blocks(n_chunks) : 0; }

extern "C" int gssd_grad_sumsq_f32(const gssd_sgd_item* items, const gssd_sgd_chunk* chunks, int n_chunks, double* partials,
                                   gssd_stream_t stream) {
    GSSD_CHECK_ARG(items && chunks && n_chunks > 0 && partials);
    hipLaunchKernelGGL(grad_sumsq_kernel, dim3(sumsq_blocks(n_chunks)), dim3(THREADS), 0, as_stream(stream), items, chunks, n_chunks,
                       partials);
    GSSD_CHECK_LAUNCH();
    return GSSD_OK;
}

extern "C" int gssd_sgd_step_f32(const gssd_sgd_item* items, const gssd_sgd_chunk* chunks, int n_chunks, const gssd_sgd_hyper* hyper,
                                 int n_groups, const double* partials, int n_partials, float max_norm, float* norm_out,
                                 gssd_stream_t stream) {
    GSSD_CHECK_ARG(items && chunks && n_chunks > 0 && hyper && n_groups > 0);
    const bool clip = max_norm >= 0.f;
    GSSD_CHECK_ARG(!clip || (partials && n_partials > 0 && norm_out));
    return for_group_batches(hyper, n_groups, [&](const GroupArgs<gssd_sgd_hyper>& hy) {
        hipLaunchKernelGGL(sgd_step_kernel, dim3(n_chunks), dim3(THREADS), 0, as_stream(stream), items, chunks, hy, partials, n_partials,
                           max_norm, norm_out);
    });
}

extern "C" int gssd_grad_scale_clip_f32(const gssd_sgd_item* items, const gssd_sgd_chunk* chunks, int n_chunks, const double* partials,
                                        int n_partials, float max_norm, float* norm_out, gssd_stream_t stream) {
    GSSD_CHECK_ARG(items && chunks && n_chunks > 0 && partials && n_partials > 0 && norm_out);
    hipLaunchKernelGGL(grad_scale_clip_kernel, dim3(n_chunks), dim3(THREADS), 0, as_stream(stream), items, chunks, partials, n_partials,
                       max_norm, norm_out);
    GSSD_CHECK_LAUNCH();
    return GSSD_OK;
}
