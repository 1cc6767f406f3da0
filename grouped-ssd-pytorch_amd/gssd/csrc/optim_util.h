// What the optimizer kernels (optim.hip: clip + SGD; optim_adam.hip: Adam / AdamW; optim_lars.hip: LARS / LAMB) share: the chunk scheme,
// the global-address-space casts, the bit-identical workgroup sum and the clip coefficient that every workgroup derives from the same
// partial sums.  Everything has internal linkage: each of the files carries its own copy.
#pragma once
#include "common.h"
#include "kernel_util.h"

namespace {

constexpr int CHUNK = 4096;            // elements per chunk: 4 x 16 bytes per thread and array
constexpr int THREADS = 256;
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

// torch.nn.utils.clip_grad_norm_: total = ||g||_2, coefficient = clamp(max_norm / (total + 1e-6), max = 1) -- a NaN stays a NaN
__device__ __forceinline__ float clip_coef(const double* partials, int n_partials, float max_norm, double* red, float& total) {
    double s = 0.0;
    for (int i = threadIdx.x; i < n_partials; i += THREADS) s += partials[i];
    s = block_sum(s, red);
    total = (float)sqrt(s);
    const float coef = max_norm / (total + 1e-6f);
    return coef > 1.f ? 1.f : coef;
}

inline int sumsq_blocks(int n_chunks) { return n_chunks < SUMSQ_MAX_BLOCKS ? n_chunks : SUMSQ_MAX_BLOCKS; }

}  // namespace
