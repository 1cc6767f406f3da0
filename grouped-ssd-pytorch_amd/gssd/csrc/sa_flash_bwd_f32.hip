// fp32 flash-style backward of Self_Attn's attention core in key / value form (layers/self_attn.py:68-80) for the 128-channel blocks of
// PixelLink version "2s" (D = 16 theta | phi channels, C2 = 64 value channels, N = 150 x 150 = 22 500 tokens).  The explicit path of
// gssd/bwd_ops.py::_sa_explicit writes the attention map and its gradient, 2 x 4 N Nk bytes per image (4 GB at 150 x 150); this path
// keeps no map.  With S = theta keys^T, P = exp(S - lse) (lse: the rows' log-sum-exp kept by the training forward), dP = d(attn_g) values^T,
// D_i = <d(attn_g)_i, attn_g_i> (gssd_rowdot_f32) and dS = P o (dP - D):
//     d values = P^T d(attn_g),   d keys = dS^T theta,   d theta = dS keys.
// Keys / values are phi / g of the same tokens (max_pool_factor 1) or their P x P average-pooled copies; the caller un-pools the
// key-side gradients (gssd_sa_unpool_f32).  Two launches, no atomics, so the gradients are reproducible bit for bit:
//   own_keys_kernel   : a workgroup owns 64 keys (one per lane, accumulators in registers); its four waves split the queries, which
//                       stream through LDS in blocks of 64; the waves' partial sums are added in a fixed order at the end.
//   own_queries_kernel: a workgroup owns 64 queries; its four waves split the keys (streamed through LDS), S and dP are recomputed.
// Plain fp32 VALU work (every LDS read inside the loops is a broadcast): correct and memory-bounded, not tuned.
#include <math.h>
#include "common.h"

namespace {

constexpr int FD = 16, FC2 = 64;       // the one (D, C2) instance
constexpr int OWN = 64, STREAM = 64, WAVES = 4;
constexpr int SV_LD = FC2 + 1;         // value rows in LDS: odd stride, the transposing stores hit distinct banks

// dK_j, dV_j of the 64 keys of workgroup (b, kt)
__global__ __launch_bounds__(256) void own_keys_kernel(const float* __restrict__ tp, int qstride, const float* __restrict__ keys, int krow,
                                                       const float* __restrict__ gT, int Nkp, const float* __restrict__ dag,
                                                       const float* __restrict__ lse, const float* __restrict__ dvec, float* __restrict__ dk,
                                                       float* __restrict__ dv, int ld_kv, int N, int Nk, int ktiles) {
    __shared__ float smem[(WAVES - 1) * OWN * (FD + FC2)];              // query blocks while streaming; the waves' partial sums at the end
    float* sq = smem;                                                   // theta [STREAM][FD]
    float* sg = sq + STREAM * FD;                                       // d(attn_g) [STREAM][FC2]
    float* sl = sg + STREAM * FC2;                                      // lse [STREAM]
    float* sD = sl + STREAM;                                            // D [STREAM]
    const int b = blockIdx.x / ktiles, j0 = (blockIdx.x - b * ktiles) * OWN;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int j = j0 + lane;
    const bool jok = j < Nk;
    float kj[FD], vj[FC2], dkj[FD], dvj[FC2];
    const float* kb = keys + ((size_t)b * Nk + (jok ? j : 0)) * krow;
    const float* vb = gT + (size_t)b * FC2 * Nkp + (jok ? j : 0);
#pragma unroll
    for (int c = 0; c < FD; ++c) {
        kj[c] = jok ? kb[c] : 0.f;
        dkj[c] = 0.f;
    }
#pragma unroll
    for (int c = 0; c < FC2; ++c) {
        vj[c] = jok ? vb[(size_t)c * Nkp] : 0.f;
        dvj[c] = 0.f;
    }
    for (int i0 = 0; i0 < N; i0 += STREAM) {
        const int nq = min(STREAM, N - i0);
        __syncthreads();
        for (int e = threadIdx.x; e < nq * FD; e += 256) {
            const int r = e / FD, c = e - r * FD;
            sq[e] = tp[((size_t)b * N + i0 + r) * qstride + c];
        }
        for (int e = threadIdx.x; e < nq * FC2; e += 256) sg[e] = dag[((size_t)b * N + i0) * FC2 + e];
        if (threadIdx.x < nq) {
            sl[threadIdx.x] = lse[(size_t)b * N + i0 + threadIdx.x];
            sD[threadIdx.x] = dvec[(size_t)b * N + i0 + threadIdx.x];
        }
        __syncthreads();
        for (int q = w; q < nq; q += WAVES) {
            const float* th = sq + q * FD;
            const float* g = sg + q * FC2;
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < FD; ++c) s = __builtin_fmaf(th[c], kj[c], s);
            const float p = expf(s - sl[q]);
            float dp = 0.f;
#pragma unroll
            for (int c = 0; c < FC2; ++c) {
                const float gc = g[c];
                dp = __builtin_fmaf(gc, vj[c], dp);
                dvj[c] = __builtin_fmaf(p, gc, dvj[c]);
            }
            const float ds = p * (dp - sD[q]);
#pragma unroll
            for (int c = 0; c < FD; ++c) dkj[c] = __builtin_fmaf(ds, th[c], dkj[c]);
        }
    }
    // waves 1 .. 3 hand their partial sums to wave 0, which adds them in wave order
    __syncthreads();
    if (w > 0) {
        float* part = smem + (size_t)(w - 1) * OWN * (FD + FC2) + lane;
#pragma unroll
        for (int c = 0; c < FD; ++c) part[c * OWN] = dkj[c];
#pragma unroll
        for (int c = 0; c < FC2; ++c) part[(FD + c) * OWN] = dvj[c];
    }
    __syncthreads();
    if (w == 0 && jok) {
        for (int v = 0; v < WAVES - 1; ++v) {
            const float* part = smem + (size_t)v * OWN * (FD + FC2) + lane;
#pragma unroll
            for (int c = 0; c < FD; ++c) dkj[c] += part[c * OWN];
#pragma unroll
            for (int c = 0; c < FC2; ++c) dvj[c] += part[(FD + c) * OWN];
        }
        float* ok = dk + ((size_t)b * Nk + j) * ld_kv;
        float* ov = dv + ((size_t)b * Nk + j) * ld_kv;
#pragma unroll
        for (int c = 0; c < FD; ++c) ok[c] = dkj[c];
#pragma unroll
        for (int c = 0; c < FC2; ++c) ov[c] = dvj[c];
    }
}

// d theta_i of the 64 queries of workgroup (b, qt)
__global__ __launch_bounds__(256) void own_queries_kernel(const float* __restrict__ tp, int qstride, const float* __restrict__ keys,
                                                          int krow, const float* __restrict__ gT, int Nkp, const float* __restrict__ dag,
                                                          const float* __restrict__ lse, const float* __restrict__ dvec,
                                                          float* __restrict__ dq, int ld_q, int N, int Nk, int qtiles) {
    __shared__ float sk[STREAM * FD];                                   // keys [STREAM][FD]
    __shared__ float sv[STREAM * SV_LD];                                // values [STREAM][SV_LD]
    __shared__ float part[(WAVES - 1) * OWN * FD];
    const int b = blockIdx.x / qtiles, i0 = (blockIdx.x - b * qtiles) * OWN;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int i = i0 + lane;
    const bool iok = i < N;
    const size_t row = (size_t)b * N + (iok ? i : 0);
    float th[FD], g[FC2], dth[FD];
#pragma unroll
    for (int c = 0; c < FD; ++c) {
        th[c] = iok ? tp[row * qstride + c] : 0.f;
        dth[c] = 0.f;
    }
#pragma unroll
    for (int c = 0; c < FC2; ++c) g[c] = iok ? dag[row * FC2 + c] : 0.f;
    const float l = iok ? lse[row] : 0.f, D = iok ? dvec[row] : 0.f;
    for (int j0 = 0; j0 < Nk; j0 += STREAM) {
        const int nk = min(STREAM, Nk - j0);
        __syncthreads();
        for (int e = threadIdx.x; e < nk * FD; e += 256) {
            const int r = e / FD, c = e - r * FD;
            sk[e] = keys[((size_t)b * Nk + j0 + r) * krow + c];
        }
        for (int e = threadIdx.x; e < STREAM * FC2; e += 256) {        // g^T [C2][Nkp] -> [key][channel]
            const int c = e / STREAM, r = e - c * STREAM;
            if (r < nk) sv[r * SV_LD + c] = gT[((size_t)b * FC2 + c) * Nkp + j0 + r];
        }
        __syncthreads();
        for (int q = w; q < nk; q += WAVES) {
            const float* kr = sk + q * FD;
            const float* vr = sv + q * SV_LD;
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < FD; ++c) s = __builtin_fmaf(th[c], kr[c], s);
            const float p = expf(s - l);
            float dp = 0.f;
#pragma unroll
            for (int c = 0; c < FC2; ++c) dp = __builtin_fmaf(g[c], vr[c], dp);
            const float ds = p * (dp - D);
#pragma unroll
            for (int c = 0; c < FD; ++c) dth[c] = __builtin_fmaf(ds, kr[c], dth[c]);
        }
    }
    if (w > 0) {
#pragma unroll
        for (int c = 0; c < FD; ++c) part[((w - 1) * FD + c) * OWN + lane] = dth[c];
    }
    __syncthreads();
    if (w == 0 && iok) {
        for (int v = 0; v < WAVES - 1; ++v)
#pragma unroll
            for (int c = 0; c < FD; ++c) dth[c] += part[(v * FD + c) * OWN + lane];
        float* o = dq + ((size_t)b * N + i) * ld_q;
#pragma unroll
        for (int c = 0; c < FD; ++c) o[c] = dth[c];
    }
}

}  // namespace

extern "C" int gssd_self_attn_flash_bwd_f32_supported(int D, int C2) { return D == FD && C2 == FC2 ? 1 : 0; }

extern "C" int gssd_self_attn_flash_bwd_f32(const float* tp, int qstride, const float* keys, int krow, const float* gT, int Nkp,
                                            const float* dag, const float* lse, const float* dvec, float* dq, int ld_q, float* dk, float* dv,
                                            int ld_kv, int B, int N, int Nk, int D, int C2, gssd_stream_t stream) {
    GSSD_CHECK_ARG(tp && keys && gT && dag && lse && dvec && dq && dk && dv && B > 0 && N > 0 && Nk > 0);
    GSSD_CHECK_ARG(gssd_self_attn_flash_bwd_f32_supported(D, C2) && qstride >= D && krow >= D && Nkp >= Nk && ld_q >= D && ld_kv >= D);
    const long long ktiles = (Nk + OWN - 1) / OWN, qtiles = (N + OWN - 1) / OWN;
    GSSD_CHECK_ARG(B * ktiles < (1ll << 31) && B * qtiles < (1ll << 31));
    hipLaunchKernelGGL(own_keys_kernel, dim3((unsigned)(B * ktiles)), dim3(256), 0, as_stream(stream), tp, qstride, keys, krow, gT, Nkp, dag,
                       lse, dvec, dk, dv, ld_kv, N, Nk, (int)ktiles);
    GSSD_CHECK_LAUNCH();
    hipLaunchKernelGGL(own_queries_kernel, dim3((unsigned)(B * qtiles)), dim3(256), 0, as_stream(stream), tp, qstride, keys, krow, gT, Nkp,
                       dag, lse, dvec, dq, ld_q, N, Nk, (int)qtiles);
    GSSD_CHECK_LAUNCH();
    return GSSD_OK;
}
