// Self_Attn's attention core, forward and backward, for ANY projection width (layers/self_attn.py:68-80): the kernels under the
// standalone module (gssd/self_attn_op.py).  D theta | phi channels and C2 value channels are multiples of 4 (4 <= D <= 256,
// 4 <= C2 <= 1024); a caller whose real widths are not pads with zero channels.
//
// Forward, gssd_self_attn_core_any_f32: flash_attn_kernel (flash_attn_core.h) at the D bucket {16, 32, 64, 128, 256} that holds D
// (the columns [D, bucket) are zero filled in LDS and registers), over channel slices of 256 (64 when C2 <= 64 and D <= 32): one launch
// per slice, each recomputing the logits; a last slice narrower than the template stages zero rows and stores its real channels only.
//
// Backward, gssd_self_attn_flash_bwd_any_f32: the maths of sa_flash_bwd_f32.hip -- P = exp(S - lse), dP = dag V^T, dS = P o (dP - dvec),
// dV = P^T dag, dK = dS^T theta, dQ = dS K -- with all five products on v_mfma_f32_16x16x4_f32, two launches, no atomics, no LDS, no
// barrier: every wave owns 16 rows of one side and walks the other side in steps of 64, so the sums are taken in one fixed order and
// the results are reproducible bit for bit.  As in the forward, every tile is kept in the "column = owner" orientation, which makes
// the C layout of one product (lane (r, kq) holds rows 4 kq + {0..3} of column r) the B-operand layout of the next:
//   own_queries (lane column r = query):  S^T = K Q^T,  dP^T = V dag^T,  dS^T in registers,  dQ^T += K^T dS^T
//   own_keys    (lane column r = key):    S = Q K^T,    dP = dag V^T,    P, dS in registers,  dK^T += theta^T dS,  dV^T += dag^T P
// and every result lands as four consecutive channels of one token = one 16-byte store.  Register budget per wave (512 with one wave
// per SIMD): own_keys holds the key fragment (D / 4) and the dK accumulators (D / 4) next to 16 x CS of dV -- CS = 256 channels
// (64 registers) up to D = 64, 128 above.  Wider C2 is cut into slices of CS along gridDim.y: slice 0 does the complete dP reduction
// and dK, the others recompute S and P only (dV needs no dS).  A operands are read straight from global memory through L1 (each is
// used by the four waves of the workgroup); rows beyond N / Nk and channels beyond D / C2 are loaded as zeros and P is masked, so they
// contribute exactly 0, and nothing is stored beyond D / C2 columns or N / Nk rows.
#include "flash_attn_core.h"

namespace {

__device__ __forceinline__ f32x4 ld4(const float* p, bool ok) { return ok ? *reinterpret_cast<const f32x4*>(p) : f32x4{0.f, 0.f, 0.f, 0.f}; }
__device__ __forceinline__ float ld1(const float* p, bool ok) { return ok ? *p : 0.f; }
__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

constexpr int STEP = 4;                       // 16-row tiles of the streamed side per step (independent MFMA chains)

// dQ of the 64 queries of workgroup (b, qt); wave w owns 16 of them
template <int DB>
__global__ __launch_bounds__(256) void bwd_own_queries(const float* __restrict__ tp, int qstride, const float* __restrict__ keys, int krow,
                                                       const float* __restrict__ gT, int Nkp, const float* __restrict__ dag,
                                                       const float* __restrict__ lse, const float* __restrict__ dvec,
                                                       float* __restrict__ dq, int ld_q, int N, int Nk, int D, int C2, int qtiles) {
    constexpr int DI = DB / 16, DG = DI < 4 ? DI : 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, kq = lane >> 4;
    const int b = blockIdx.x / qtiles, q0 = (blockIdx.x - b * qtiles) * 64 + wave * 16;
    if (q0 >= N) return;                                               // (no barrier in this kernel)
    const int q = q0 + r;
    const bool qok = q < N;
    const size_t qrow = (size_t)b * N + (qok ? q : 0);
    const float* kb = keys + (size_t)b * Nk * krow;
    const float* vb = gT + (size_t)b * C2 * Nkp;
    const float* dgq = dag + qrow * C2;
    f32x4 qf[DI], acc[DI];                                             // B operand: theta[q][16 i + 4 kq + e]
#pragma unroll
    for (int i = 0; i < DI; ++i) {
        qf[i] = ld4(tp + qrow * qstride + 16 * i + 4 * kq, qok && 16 * i + 4 * kq < D);
        acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const float l = ld1(lse + qrow, qok), dvq = ld1(dvec + qrow, qok);
    for (int key0 = 0; key0 < Nk; key0 += 16 * STEP) {
        f32x4 s[STEP], dp[STEP];
#pragma unroll
        for (int t = 0; t < STEP; ++t) s[t] = dp[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        // S^T = K Q^T: A = keys[key0 + 16 t + r][16 i + 4 kq + e]
#pragma unroll
        for (int i = 0; i < DI; ++i) {
            if (16 * i >= D) break;
            f32x4 kf[STEP];
#pragma unroll
            for (int t = 0; t < STEP; ++t) {
                const int key = key0 + 16 * t + r;
                kf[t] = ld4(kb + (size_t)key * krow + 16 * i + 4 * kq, key < Nk && 16 * i + 4 * kq < D);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int t = 0; t < STEP; ++t) s[t] = mfma4(kf[t][e], qf[i][e], s[t]);
        }
        // dP^T = V dag^T over ALL C2 channels: A = V[key][c + e] = gT[c + e][key], B = dag[q][c + e], c = c0 + 4 kq
        for (int c0 = 0; c0 < C2; c0 += 16) {
            const int c = c0 + 4 * kq;
            const bool cok = c < C2;
            const f32x4 g = ld4(dgq + c, qok && cok);
            f32x4 vf[STEP];
#pragma unroll
            for (int t = 0; t < STEP; ++t) {
                const int key = key0 + 16 * t + r;
#pragma unroll
                for (int e = 0; e < 4; ++e) vf[t][e] = ld1(vb + (size_t)(c + e) * Nkp + key, cok && key < Nk);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int t = 0; t < STEP; ++t) dp[t] = mfma4(vf[t][e], g[e], dp[t]);
        }
        // dS^T[key = 16 t + 4 kq + e][q]: the B operand of the last product
#pragma unroll
        for (int t = 0; t < STEP; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool ok = qok && key0 + 16 * t + 4 * kq + e < Nk;
                const float p = ok ? __expf(s[t][e] - l) : 0.f;
                s[t][e] = ok ? p * (dp[t][e] - dvq) : 0.f;
            }
        // dQ^T += K^T dS^T: A = keys[key0 + 16 t + 4 kq + e][16 i + r]
#pragma unroll
        for (int ig = 0; ig < DI; ig += DG) {
            if (16 * ig >= D) break;
#pragma unroll
            for (int t = 0; t < STEP; ++t) {
                f32x4 a[DG];
#pragma unroll
                for (int ii = 0; ii < DG; ++ii)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int key = key0 + 16 * t + 4 * kq + e, d = 16 * (ig + ii) + r;
                        a[ii][e] = ld1(kb + (size_t)key * krow + d, key < Nk && d < D);
                    }
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int ii = 0; ii < DG; ++ii) acc[ig + ii] = mfma4(a[ii][e], s[t][e], acc[ig + ii]);
            }
        }
    }
    if (qok) {                                                         // lane holds dQ[q][16 i + 4 kq + {0..3}]
        float* o = dq + qrow * ld_q + 4 * kq;
#pragma unroll
        for (int i = 0; i < DI; ++i)
            if (16 * i + 4 * kq < D) *reinterpret_cast<f32x4*>(o + 16 * i) = acc[i];
    }
}

// dK (slice 0) and the channels [CS y, CS (y + 1)) of dV of the 64 keys of workgroup (b, kt); wave w owns 16 of them
template <int DB, int CS>
__global__ __launch_bounds__(256) void bwd_own_keys(const float* __restrict__ tp, int qstride, const float* __restrict__ keys, int krow,
                                                    const float* __restrict__ gT, int Nkp, const float* __restrict__ dag,
                                                    const float* __restrict__ lse, const float* __restrict__ dvec, float* __restrict__ dk,
                                                    float* __restrict__ dv, int ld_kv, int N, int Nk, int D, int C2, int ktiles) {
    constexpr int DI = DB / 16, DG = DI < 4 ? DI : 4, CT = CS / 16, CG = 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, kq = lane >> 4;
    const int b = blockIdx.x / ktiles, k0 = (blockIdx.x - b * ktiles) * 64 + wave * 16;
    if (k0 >= Nk) return;                                              // (no barrier in this kernel)
    const int cs0 = blockIdx.y * CS;
    const bool first = blockIdx.y == 0;                                // the slice that also owns dP, dS and dK
    const int key = k0 + r;
    const bool kok = key < Nk;
    const size_t krow_i = (size_t)b * Nk + (kok ? key : 0);
    const float* tpb = tp + (size_t)b * N * qstride;
    const float* dgb = dag + (size_t)b * N * C2;
    const float* vb = gT + (size_t)b * C2 * Nkp + (kok ? key : 0);
    const float* lb = lse + (size_t)b * N;
    const float* db = dvec + (size_t)b * N;
    f32x4 kf[DI], dka[DI], dva[CT];                                    // B operand: keys[key][16 i + 4 kq + e]
#pragma unroll
    for (int i = 0; i < DI; ++i) {
        kf[i] = ld4(keys + krow_i * krow + 16 * i + 4 * kq, kok && 16 * i + 4 * kq < D);
        dka[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int c = 0; c < CT; ++c) dva[c] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int q0 = 0; q0 < N; q0 += 16 * STEP) {
        f32x4 s[STEP], p[STEP];
#pragma unroll
        for (int t = 0; t < STEP; ++t) s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        // S = Q K^T: A = theta[q0 + 16 t + r][16 i + 4 kq + e]
#pragma unroll
        for (int i = 0; i < DI; ++i) {
            if (16 * i >= D) break;
            f32x4 a[STEP];
#pragma unroll
            for (int t = 0; t < STEP; ++t) {
                const int q = q0 + 16 * t + r;
                a[t] = ld4(tpb + (size_t)q * qstride + 16 * i + 4 * kq, q < N && 16 * i + 4 * kq < D);
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int t = 0; t < STEP; ++t) s[t] = mfma4(a[t][e], kf[i][e], s[t]);
        }
        // P[q = 16 t + 4 kq + e][key]
#pragma unroll
        for (int t = 0; t < STEP; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int q = q0 + 16 * t + 4 * kq + e;
                const bool ok = kok && q < N;
                p[t][e] = ok ? __expf(s[t][e] - lb[ok ? q : 0]) : 0.f;
            }
        if (first) {
            // dP = dag V^T over ALL C2 channels: A = dag[q][c + e], B = V[key][c + e] = gT[c + e][key], c = c0 + 4 kq
            f32x4 dp[STEP];
#pragma unroll
            for (int t = 0; t < STEP; ++t) dp[t] = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int c0 = 0; c0 < C2; c0 += 16) {
                const int c = c0 + 4 * kq;
                const bool cok = c < C2;
                f32x4 vf, g[STEP];
#pragma unroll
                for (int e = 0; e < 4; ++e) vf[e] = ld1(vb + (size_t)(c + e) * Nkp, cok && kok);
#pragma unroll
                for (int t = 0; t < STEP; ++t) {
                    const int q = q0 + 16 * t + r;
                    g[t] = ld4(dgb + (size_t)q * C2 + c, q < N && cok);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int t = 0; t < STEP; ++t) dp[t] = mfma4(g[t][e], vf[e], dp[t]);
            }
            // dS, then dK^T += theta^T dS: A = theta[q0 + 16 t + 4 kq + e][16 i + r]
#pragma unroll
            for (int t = 0; t < STEP; ++t)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int q = q0 + 16 * t + 4 * kq + e;
                    const bool ok = kok && q < N;
                    s[t][e] = ok ? p[t][e] * (dp[t][e] - db[ok ? q : 0]) : 0.f;
                }
#pragma unroll
            for (int ig = 0; ig < DI; ig += DG) {
                if (16 * ig >= D) break;
#pragma unroll
                for (int t = 0; t < STEP; ++t) {
                    f32x4 a[DG];
#pragma unroll
                    for (int ii = 0; ii < DG; ++ii)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const int q = q0 + 16 * t + 4 * kq + e, d = 16 * (ig + ii) + r;
                            a[ii][e] = ld1(tpb + (size_t)q * qstride + d, q < N && d < D);
                        }
#pragma unroll
                    for (int e = 0; e < 4; ++e)
#pragma unroll
                        for (int ii = 0; ii < DG; ++ii) dka[ig + ii] = mfma4(a[ii][e], s[t][e], dka[ig + ii]);
                }
            }
        }
        // dV^T += dag^T P: A = dag[q0 + 16 t + 4 kq + e][cs0 + 16 c + r]
#pragma unroll
        for (int cg = 0; cg < CT; cg += CG) {
            if (cs0 + 16 * cg >= C2) break;
#pragma unroll
            for (int t = 0; t < STEP; ++t) {
                f32x4 a[CG];
#pragma unroll
                for (int cc = 0; cc < CG; ++cc)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int q = q0 + 16 * t + 4 * kq + e, c = cs0 + 16 * (cg + cc) + r;
                        a[cc][e] = ld1(dgb + (size_t)q * C2 + c, q < N && c < C2);
                    }
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int cc = 0; cc < CG; ++cc) dva[cg + cc] = mfma4(a[cc][e], p[t][e], dva[cg + cc]);
            }
        }
    }
    if (kok) {                                                         // lane holds dK[key][16 i + 4 kq + {0..3}], dV[key][cs0 + 16 c + 4 kq + {0..3}]
        if (first) {
            float* o = dk + krow_i * ld_kv + 4 * kq;
#pragma unroll
            for (int i = 0; i < DI; ++i)
                if (16 * i + 4 * kq < D) *reinterpret_cast<f32x4*>(o + 16 * i) = dka[i];
        }
        float* o = dv + krow_i * ld_kv + cs0 + 4 * kq;
#pragma unroll
        for (int c = 0; c < CT; ++c)
            if (cs0 + 16 * c + 4 * kq < C2) *reinterpret_cast<f32x4*>(o + 16 * c) = dva[c];
    }
}

struct BwdArgs {
    const float *tp, *keys, *gT, *dag, *lse, *dvec;
    float *dq, *dk, *dv;
    int qstride, krow, Nkp, ld_q, ld_kv, B, N, Nk, D, C2;
};

template <int DB>
int launch_bwd(const BwdArgs& a, hipStream_t s) {
    constexpr int CS = DB <= 64 ? 256 : 128;
    const int ktiles = (a.Nk + 63) / 64, qtiles = (a.N + 63) / 64, slices = (a.C2 + CS - 1) / CS;
    hipLaunchKernelGGL((bwd_own_keys<DB, CS>), dim3((unsigned)(a.B * ktiles), (unsigned)slices), dim3(256), 0, s, a.tp, a.qstride, a.keys,
                       a.krow, a.gT, a.Nkp, a.dag, a.lse, a.dvec, a.dk, a.dv, a.ld_kv, a.N, a.Nk, a.D, a.C2, ktiles);
    GSSD_CHECK_LAUNCH();
    hipLaunchKernelGGL((bwd_own_queries<DB>), dim3((unsigned)(a.B * qtiles)), dim3(256), 0, s, a.tp, a.qstride, a.keys, a.krow, a.gT, a.Nkp,
                       a.dag, a.lse, a.dvec, a.dq, a.ld_q, a.N, a.Nk, a.D, a.C2, qtiles);
    GSSD_CHECK_LAUNCH();
    return GSSD_OK;
}

// the forward at D bucket DB: channel slices of 256 (one of 64 for the narrow blocks)
template <int DB>
int launch_fwd(const float* tp, const float* kp, const float* gT, float* out, int B, int N, int Nk, int Nkp, int D, int C2, int kstride,
               float* lse, hipStream_t s) {
    constexpr int BKV = DB <= 64 ? 64 : 32;        // (BKV D + slice BKV) 4 bytes: at most the 80 KB of the (64, 256) instance
    if constexpr (DB <= 32) {
        if (C2 <= 64) return launch<DB, 64, BKV, true>(tp, kp, gT, out, B, N, Nk, Nkp, D, kstride, 0, lse, s, C2, C2, C2);
    }
    for (int c0 = 0; c0 < C2; c0 += 256) {
        const int rc = launch<DB, 256, BKV, true>(tp, kp, gT + (size_t)c0 * Nkp, out + c0, B, N, Nk, Nkp, D, kstride, 0,
                                                  c0 == 0 ? lse : nullptr, s, C2, C2, C2 - c0 < 256 ? C2 - c0 : 256);
        if (rc != GSSD_OK) return rc;
    }
    return GSSD_OK;
}

inline bool al16(const void* p) { return ((uintptr_t)p % 16) == 0; }

}  // namespace

#define GSSD_SA_ANY_WIDTHS(D, C2)                                                                                                      \
    do {                                                                                                                               \
        if (!((D) >= 4 && (D) <= 256 && (D) % 4 == 0 && (C2) >= 4 && (C2) <= 1024 && (C2) % 4 == 0)) {                                   \
            gssd_set_error("self-attention (any size): theta/phi channels %d, g channels %d: multiples of 4 with 4 <= D <= 256 and "  \
                           "4 <= C2 <= 1024 (pad with zero channels)", (D), (C2));                                                     \
            return GSSD_EINVAL;                                                                                                        \
        }                                                                                                                              \
    } while (0)

extern "C" int gssd_self_attn_core_any_f32(const float* tp, const float* kp, const float* gT, float* out, int B, int N, int Nk, int Nkp,
                                           int D, int C2, int kstride, float* lse, gssd_stream_t stream) {
    GSSD_CHECK_ARG(tp && kp && gT && out && B > 0 && N > 0 && Nk > 0 && Nkp >= Nk && Nkp % 4 == 0);
    GSSD_SA_ANY_WIDTHS(D, C2);
    GSSD_CHECK_ARG(kstride >= D && kstride % 4 == 0);
    GSSD_CHECK_ARG(al16(tp) && al16(kp) && al16(gT) && al16(out) && al16(lse));
    GSSD_CHECK_ARG((long long)B * ((N + 63) / 64) < (1ll << 31));
    hipStream_t s = as_stream(stream);
    if (D <= 16) return launch_fwd<16>(tp, kp, gT, out, B, N, Nk, Nkp, D, C2, kstride, lse, s);
    if (D <= 32) return launch_fwd<32>(tp, kp, gT, out, B, N, Nk, Nkp, D, C2, kstride, lse, s);
    if (D <= 64) return launch_fwd<64>(tp, kp, gT, out, B, N, Nk, Nkp, D, C2, kstride, lse, s);
    if (D <= 128) return launch_fwd<128>(tp, kp, gT, out, B, N, Nk, Nkp, D, C2, kstride, lse, s);
    return launch_fwd<256>(tp, kp, gT, out, B, N, Nk, Nkp, D, C2, kstride, lse, s);
}

extern "C" int gssd_self_attn_flash_bwd_any_f32(const float* tp, int qstride, const float* keys, int krow, const float* gT, int Nkp,
                                                const float* dag, const float* lse, const float* dvec, float* dq, int ld_q, float* dk,
                                                float* dv, int ld_kv, int B, int N, int Nk, int D, int C2, gssd_stream_t stream) {
    GSSD_CHECK_ARG(tp && keys && gT && dag && lse && dvec && dq && dk && dv && B > 0 && N > 0 && Nk > 0);
    GSSD_SA_ANY_WIDTHS(D, C2);
    GSSD_CHECK_ARG(qstride >= D && krow >= D && Nkp >= Nk && ld_q >= D && ld_kv >= D && ld_kv >= C2);
    GSSD_CHECK_ARG(qstride % 4 == 0 && krow % 4 == 0 && Nkp % 4 == 0 && ld_q % 4 == 0 && ld_kv % 4 == 0);
    GSSD_CHECK_ARG(al16(tp) && al16(keys) && al16(gT) && al16(dag) && al16(lse) && al16(dvec) && al16(dq) && al16(dk) && al16(dv));
    GSSD_CHECK_ARG((long long)B * ((N + 63) / 64) < (1ll << 31) && (long long)B * ((Nk + 63) / 64) < (1ll << 31));
    const BwdArgs a{tp, keys, gT, dag, lse, dvec, dq, dk, dv, qstride, krow, Nkp, ld_q, ld_kv, B, N, Nk, D, C2};
    hipStream_t s = as_stream(stream);
    if (D <= 16) return launch_bwd<16>(a, s);
    if (D <= 32) return launch_bwd<32>(a, s);
    if (D <= 64) return launch_bwd<64>(a, s);
    if (D <= 128) return launch_bwd<128>(a, s);
    return launch_bwd<256>(a, s);
}
