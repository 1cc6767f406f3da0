// The fp32 flash-style Self_Attn core kernel (see flash_attn.hip for the layout story), shared by the specialised entry
// gssd_self_attn_core_kv_f32 (flash_attn.hip) and the any-size entry gssd_self_attn_core_any_f32 (sa_any.hip).
#pragma once
#include <math.h>
#include "common.h"
#include "kernel_util.h"

namespace {

__device__ __attribute__((aligned(16))) float g_zero16[4] = {0.f, 0.f, 0.f, 0.f};

// Stage a [ROWS][QR quads] tile: lane L of a 1-KiB piece lands at (row_in = L / QR, slot = L % QR) and fetches logical quad
// slot ^ (row & SW).  row_ptr(row) -> global pointer of that row's first float or nullptr (zero row); quad_ok(quad) masks columns.
template <int ROWS, int QR, typename RowPtr, typename QuadOk>
__device__ __forceinline__ void stage_tile(float* lds, int wave, int lane, RowPtr row_ptr, QuadOk quad_ok) {
    constexpr int RPP = 64 / QR;                       // rows per 1-KiB piece
    constexpr int PIECES = ROWS / RPP;
    constexpr int SW = (QR < 16 ? QR : 16) - 1;
    const int row_in = lane / QR, slot = lane % QR;
#pragma unroll
    for (int p0 = 0; p0 < PIECES; p0 += 4) {
        const int piece = p0 + wave;
        if (PIECES % 4 != 0 && piece >= PIECES) break;
        const int row = piece * RPP + row_in;
        const int quad = slot ^ (row & SW);
        const float* rp = row_ptr(row);
        const float* src = (rp != nullptr && quad_ok(quad)) ? rp + 4 * quad : g_zero16;
        dma16(src, lds + piece * 256);
    }
}

// ANY (sa_any.hip): the launch covers c_real <= C2 real channels of its slice -- value rows beyond them are staged as zeros and their
// outputs are not stored; the specialised instances compile that test away.
template <int D, int C2, int BKV, bool ANY = false>
__global__ __launch_bounds__(256, (C2 > 256 ? 1 : 2)) void flash_attn_kernel(const float* __restrict__ tp, const float* __restrict__ kp,
                                                           const float* __restrict__ gT, float* __restrict__ out, int N, int Nk,
                                                           int Np, int qtiles, int d_real, int kstride, int out_bf16,
                                                           float* __restrict__ lse, int out_stride, int g_batch_rows, int c_real) {
    // out_stride / g_batch_rows: the launch may cover a C2-wide SLICE of wider rows (g channels 1024 = two launches of 512: the
    // accumulators of all 1024 would need 256 registers)
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const Ks = smem;                    // [BKV][D]
    float* const Vs = smem + BKV * D;          // [C2][BKV]
    constexpr int QRK = D / 4, QRV = BKV / 4;
    constexpr int SWK = (QRK < 16 ? QRK : 16) - 1, SWV = (QRV < 16 ? QRV : 16) - 1;
    constexpr int KT = BKV / 16, CT = C2 / 16, DI = D / 16;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, kq = lane >> 4;
    const int b = blockIdx.x / qtiles, qt = blockIdx.x - b * qtiles;
    const int q = qt * 64 + wave * 16 + r;                       // this lane's query (column of every C-layout tile)
    const int tps = 2 * d_real;                                   // floats per token of tp (d_real <= D; D - d_real zero filled)
    const float* tpb = tp + (size_t)b * N * tps;
    const float* kpb = kp + (size_t)b * Nk * kstride;            // keys: phi of the same tokens (kp = tp + d_real, Nk = N) or
    const float* gTb = gT + (size_t)b * g_batch_rows * Np;        // the pooled phi / g of max_pool_factor > 1 (Nk < N)

    // query fragments: B operand, lane (q, kq) holds theta[q][16 i + 4 kq + s]
    f32x4 qf[DI];
#pragma unroll
    for (int i = 0; i < DI; ++i) {
        qf[i] = (q < N && 16 * i + 4 * kq < d_real) ? *reinterpret_cast<const f32x4*>(tpb + (size_t)q * tps + 16 * i + 4 * kq)
                                                    : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    f32x4 o[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) o[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m_run = -INFINITY, l_run = 0.f;                        // l_run: this lane's share (its kq keys) of the row sum

    const int ntiles = (Nk + BKV - 1) / BKV;
    for (int t = 0; t < ntiles; ++t) {
        const int key0 = t * BKV;
        __syncthreads();                                          // every wave is done with the previous tiles
        stage_tile<BKV, QRK>(Ks, wave, lane,
                             [&](int row) { return key0 + row < Nk ? kpb + (size_t)(key0 + row) * kstride : (const float*)nullptr; },
                             [&](int quad) { return 4 * quad < d_real; });
        stage_tile<C2, QRV>(Vs, wave, lane,
                            [&](int row) { return !ANY || row < c_real ? gTb + (size_t)row * Np + key0 : (const float*)nullptr; },
                            [&](int quad) { return key0 + 4 * quad < Np; });
        __syncthreads();                                          // (waits for the DMA: vmcnt(0) + barrier)

        // ---- S^T = K . Q^T ----------------------------------------------------------------------------------------------------
        // (independent accumulators back to back: a dependent v_mfma_f32_16x16x4_f32 waits 40 cycles, an independent one 32)
        f32x4 s[KT];
#pragma unroll
        for (int kt = 0; kt < KT; ++kt) s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < DI; ++i) {
            f32x4 kf[KT];
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) {
                const int row = kt * 16 + r;
                kf[kt] = *reinterpret_cast<const f32x4*>(Ks + row * D + (((4 * i + kq) ^ (row & SWK)) << 2));
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int kt = 0; kt < KT; ++kt) s[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[kt][e], qf[i][e], s[kt], 0, 0, 0);
        }
        // ---- online softmax over the keys of this tile ----------------------------------------------------------------------------
        float mx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (key0 + kt * 16 + 4 * kq + e >= Nk) s[kt][e] = -INFINITY;
                mx = fmaxf(mx, s[kt][e]);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);                     // finite: every tile holds at least one valid key
        const float alpha = __expf(m_run - m_new);                // 0 on the first tile (m_run = -inf)
        float psum = 0.f;
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float p = __expf(s[kt][e] - m_new);
                s[kt][e] = p;
                psum += p;
            }
        l_run = l_run * alpha + psum;
        m_run = m_new;
        if (__any(alpha != 1.f)) {                                // the running maximum usually stops moving after a few tiles
#pragma unroll
            for (int c = 0; c < CT; ++c) o[c] *= alpha;
        }
        // ---- O^T += V . P^T -------------------------------------------------------------------------------------------------------
        constexpr int CG = CT < 4 ? CT : 4;
#pragma unroll
        for (int cg = 0; cg < CT; cg += CG) {
#pragma unroll
            for (int kt = 0; kt < KT; ++kt) {
                f32x4 vf[CG];
#pragma unroll
                for (int cc = 0; cc < CG; ++cc) {
                    const int row = (cg + cc) * 16 + r;
                    vf[cc] = *reinterpret_cast<const f32x4*>(Vs + row * BKV + (((4 * kt + kq) ^ (row & SWV)) << 2));
                }
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int cc = 0; cc < CG; ++cc)
                        o[cg + cc] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[cc][e], s[kt][e], o[cg + cc], 0, 0, 0);
            }
        }
    }
    // row sums: the four kq lanes of a query hold disjoint key subsets
    l_run += __shfl_xor(l_run, 16, 64);
    l_run += __shfl_xor(l_run, 32, 64);
    const float inv = 1.f / l_run;
    // log-sum-exp of the row's logits: the backward rebuilds the probabilities as exp(s - lse) in a GEMM epilogue (no softmax pass)
    if (lse != nullptr && q < N && kq == 0) lse[(size_t)b * N + q] = m_run + logf(l_run);
    if (q < N) {
        if (out_bf16) {             // bf16 storage mode (configs[4]): the o conv reads bf16
            unsigned short* dst = reinterpret_cast<unsigned short*>(out) + ((size_t)b * N + q) * out_stride + 4 * kq;
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                const f32x4 v = o[c] * inv;
                *reinterpret_cast<bf16x4*>(dst + 16 * c) = bf16x4{(__bf16)v[0], (__bf16)v[1], (__bf16)v[2], (__bf16)v[3]};
            }
        } else {
            float* dst = out + ((size_t)b * N + q) * out_stride + 4 * kq;
#pragma unroll
            for (int c = 0; c < CT; ++c)
                if (!ANY || 16 * c + 4 * kq < c_real) *reinterpret_cast<f32x4*>(dst + 16 * c) = o[c] * inv;
        }
    }
}

template <int D, int C2, int BKV, bool ANY = false>
int launch(const float* tp, const float* kp, const float* gT, float* out, int B, int N, int Nk, int Np, int d_real, int kstride,
           int out_bf16, float* lse, hipStream_t stream, int out_stride = C2, int g_batch_rows = C2, int c_real = C2) {
    constexpr int smem = (BKV * D + C2 * BKV) * (int)sizeof(float);
    static unsigned attr_mask = 0;
    auto kern = flash_attn_kernel<D, C2, BKV, ANY>;
    if (const int rc = gssd_max_dynamic_lds(&attr_mask, kern, smem)) return rc;
    const int qtiles = (N + 63) / 64;
    hipLaunchKernelGGL(kern, dim3(B * qtiles), dim3(256), smem, stream, tp, kp, gT, out, N, Nk, Np, qtiles, d_real, kstride, out_bf16, lse,
                       out_stride, g_batch_rows, c_real);
    GSSD_CHECK_LAUNCH();
    return GSSD_OK;
}

}  // namespace
