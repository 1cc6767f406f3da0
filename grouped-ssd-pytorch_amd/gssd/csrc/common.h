// Shared helpers for the gfx950 kernels of libgssd_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "gssd_hip.h"

void gssd_set_error(const char* fmt, ...);

#define GSSD_CHECK_ARG(cond)                                                          \
    do {                                                                              \
        if (!(cond)) {                                                                \
            gssd_set_error("%s:%d: invalid argument: %s", __FILE__, __LINE__, #cond); \
            return GSSD_EINVAL;                                                       \
        }                                                                             \
    } while (0)

#define GSSD_CHECK_LAUNCH()                                                                     \
    do {                                                                                        \
        hipError_t e__ = hipGetLastError();                                                     \
        if (e__ != hipSuccess) {                                                                \
            gssd_set_error("%s:%d: launch failed: %s", __FILE__, __LINE__, hipGetErrorString(e__)); \
            return GSSD_ELAUNCH;                                                                \
        }                                                                                       \
    } while (0)

static inline hipStream_t as_stream(gssd_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

// Raises a kernel's dynamic-LDS limit (hipFuncAttributeMaxDynamicSharedMemorySize; a launch with more than 48 KB needs it) once per
// device.  The attribute is per DEVICE: `mask` is the launch site's own `static unsigned`, one "done" bit per device id, so a process
// that touches several GPUs (tests on cuda:1, one-process multi-device callers) never launches a large-LDS kernel without it.  Launches
// come from two host threads (the forward from the caller's, the backward from autograd's): the bit is published (release) only AFTER
// hipFuncSetAttribute has returned success, so a thread that sees it set (acquire: the one atomic load of the steady state) may launch;
// two threads racing on an unset bit both set the attribute (idempotent), and a failed call is retried by the next launch.
// A launch site that picks one of two kernels at run time passes both and shares one mask.  Returns GSSD_OK or GSSD_ELAUNCH.
template <typename K, typename K2 = void()>
static inline int gssd_max_dynamic_lds(unsigned* mask, K* kernel, size_t bytes, K2* kernel2 = nullptr, size_t bytes2 = 0) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    const bool tracked = dev >= 0 && dev < 32;
    if (tracked && (__atomic_load_n(mask, __ATOMIC_ACQUIRE) & (1u << dev))) return GSSD_OK;
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) {
        gssd_set_error("hipFuncSetAttribute(max dynamic LDS = %zu) failed", bytes);
        return GSSD_ELAUNCH;
    }
    if (kernel2 &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(kernel2), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes2) != hipSuccess) {
        gssd_set_error("hipFuncSetAttribute(max dynamic LDS = %zu) failed", bytes2);
        return GSSD_ELAUNCH;
    }
    if (tracked) (void)__atomic_fetch_or(mask, 1u << dev, __ATOMIC_RELEASE);
    return GSSD_OK;
}

// Environment switches are read once per process (function-local `static const` at the site that asks).  The common kind is ON unless
// its value starts with '0' (unset, empty, "1", anything else: on); the presence-only and numeric switches are read where they are used.
static inline bool gssd_env_off(const char* name) {
    const char* e = getenv(name);
    return e && e[0] == '0';
}
// GSSD_X6_F16=0 turns the fp16 planes of the fp32-equivalent kernels off everywhere: bf16 planes only (runtime.hip)
bool gssd_x6_f16_enabled();

// BatchNorm batch sums (gssd_conv_desc::stats) may be kept in `rep` replicas of [2 * Cout] doubles: a workgroup adds into replica
// (workgroup id mod rep), the consumers (gssd_bn_finalize_*, gssd_bn_relu_pool_*, gssd_bn_bwd_finalize_f32) add the replicas up in a
// fixed order.  Why: device-scope fp64 atomics on one cache line are served one after the other (~8 ns each, measured round 4); the
// persistent trunk kernels flush all their workgroups' sums at the END of the launch -- 131 k atomics on 16 lines = a 60 us serial
// tail on a 140 us kernel (profiles/r04_thin_knockout_before.txt).  16 - 32 replicas make the tail 2 - 4 us.
__device__ __forceinline__ double* gssd_stats_replica(double* stats, int rep, int cout) {
    return rep > 1 ? stats + (size_t)((blockIdx.x + 7u * blockIdx.y + 13u * blockIdx.z) % (unsigned)rep) * (2 * (size_t)cout) : stats;
}
__device__ __forceinline__ double gssd_stats_sum(const double* stats, int idx, int two_c, int rep) {
    double s = stats[idx];
    for (int r = 1; r < rep; ++r) s += stats[idx + (size_t)r * two_c];
    return s;
}

// 64-lane wavefront reductions (gfx950: wave = 64)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// What the conv dispatchers hand down their gssd_try_* / launch chain: the stream to launch on, or (name != nullptr) the buffer
// gssd_conv2d_kernel_name / gssd_conv2d_wgrad_kernel_name want the chosen kernel instance's name in.  A launch site names its instance FIRST -- before any HIP call
// or claimed resource -- so the query runs the dispatch's own control flow and touches no device.
struct gssd_conv_ctx {
    hipStream_t stream = nullptr;
    char* name = nullptr;
    int cap = 0;
    int tile_m = 0;                 // out, when naming: pixels per workgroup of a conv_flat_bf16 instance (gssd_conv_flat_bf16_takes)
};
// writes the name (printf-style) into c.name: GSSD_OK, or GSSD_EINVAL when it does not fit c.cap (runtime.hip)
int gssd_name_kernel(const gssd_conv_ctx& c, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

// The implicit-GEMM tile of a launch the specialised kernels left to conv_igemm.hip / conv_bf16.hip (the two share their tilings).
enum gssd_igemm_tile { GSSD_TILE_32x64, GSSD_TILE_64x64, GSSD_TILE_128x128, GSSD_TILE_128x64, GSSD_TILE_128x32, GSSD_TILE_128x16 };
static inline gssd_igemm_tile gssd_pick_igemm_tile(const gssd_conv_desc& d, int M, int images) {
    const int cout_g = d.Cout / d.groups;
    // small maps (<= 10 x 10 at batch 32; per-image GEMMs of <= 100 tokens): 32- / 64-row tiles, three-stage K loop
    static const bool no_small = getenv("GSSD_NO_SMALL_TILES") != nullptr;       // ablation switch
    if (!no_small && cout_g > 32 && d.split_k == 1 && !(d.out_mode == GSSD_OUT_SPLIT_T && d.split_n % 64 != 0)) {
        // (per-image GEMMs count all their images: the 19 x 19 projections -- 361 tokens x 32 images -- keep the 128-row tiles)
        const long long mtot = (long long)M * images;
        if (mtot <= 512 || (d.m_per_image && mtot <= 4096 && M <= 128)) return GSSD_TILE_32x64;
        if (mtot <= 4096) return GSSD_TILE_64x64;
    }
    if (cout_g > 64) {
        // 128x128 tiles run 2 workgroups per CU (LDS), 128x64 tiles 3: pick the one whose last round of workgroups is
        // fuller (wave quantisation decides small 19x19 / 38x38 layers); the wide tile wins ties (less B re-read).
        const long long mt = (M + 127) / 128, z = d.m_per_image ? images : d.split_k;
        const long long b128 = mt * d.groups * ((cout_g + 127) / 128) * z, b64 = mt * d.groups * ((cout_g + 63) / 64) * z;
        const double e128 = (double)b128 / (double)(((b128 + 511) / 512) * 512);
        const double e64 = 0.94 * (double)b64 / (double)(((b64 + 767) / 768) * 768);
        // short reductions (K <= 256: the attention output conv) are prologue / epilogue bound: three resident 128x64
        // workgroups per CU overlap those phases better than two 128x128 ones
        // (the three-stage K loop of the small tiles on these 128-row tiles: bf16 fwd + loss 3.87 -> 4.11 ms, measured round 4)
        if (e64 > e128 || d.K <= 256 || (d.out_mode == GSSD_OUT_SPLIT_T && d.split_n % 128 != 0)) return GSSD_TILE_128x64;
        return GSSD_TILE_128x128;
    }
    return cout_g > 32 ? GSSD_TILE_128x64 : cout_g > 16 ? GSSD_TILE_128x32 : GSSD_TILE_128x16;
}

// conv_igemm.hip / conv_bf16.hip: the two conv entry points' validation + dispatch (launches on c.stream, or names into c.name)
int gssd_conv_dispatch_f32(const gssd_conv_desc* d, gssd_conv_ctx& c);
int gssd_conv_dispatch_bf16(const gssd_conv_desc* d, gssd_conv_ctx& c);
// The gssd_try_* below: 1 = not this kernel's descriptor (the dispatcher goes on), else the GSSD_* code of the launch (or of naming it).
// conv_thin.hip: returns 1 when the descriptor is not one of the thin grouped 3x3 shapes, else a GSSD_* code
int gssd_try_conv_thin(const gssd_conv_desc& d, gssd_conv_ctx& c);
// conv_wino.hip: returns 1 when the descriptor is not a Winograd shape / has no transformed weights
int gssd_try_conv_wino(const gssd_conv_desc& d, gssd_conv_ctx& c);
int gssd_try_conv_x6(const gssd_conv_desc& d, gssd_conv_ctx& c);      // csrc/conv_x6.hip: 1 = not taken
// conv_wino_x6.hip: Winograd with three-plane bf16 operands; its U planes are stored behind the fp32 U of gssd_winograd_weight_f32
long long gssd_wino_x6_plane_elems(int cout_g, int groups, int cin_g);  // bf16 elements (0: not a shape it takes)
int gssd_wino_x6_pack(const float* w_packed, void* Ux, int Cout, int groups, int cin_g, int row_stride, hipStream_t stream);
bool gssd_wino_x6_enabled();                                             // GSSD_WINO_X6=0 switches it off
bool gssd_wino_x6_wanted(const gssd_conv_desc& d);                        // the shapes it takes by default (GSSD_WINO_X6=2: all it can)
int gssd_launch_conv_wino_x6(const gssd_conv_desc& d, const void* Ux, gssd_conv_ctx& c);
// conv_patch_x6.hip: dense 3x3 convs with many input channels and <= 128 outputs, fp16 planes (GSSD_CONV_F16_OK launches with wgt_patch); else 1
int gssd_try_conv_patch_x6(const gssd_conv_desc& d, gssd_conv_ctx& c);
// conv_thin_x6.hip: conv1_2 / conv2_1 / conv2_2 shape classes on the bf16 matrix cores with three-plane operands; else returns 1
int gssd_try_conv_thin_x6(const gssd_conv_desc& d, gssd_conv_ctx& c);
// conv_thin_wino.hip: conv1_2's shape class (4 x 16 -> 16 channels, large map) with Winograd weights; else returns 1
int gssd_try_conv_thin_wino(const gssd_conv_desc& d, gssd_conv_ctx& c);
// The weight gradient's chain (conv_wgrad.hip: gssd_conv2d_wgrad_f32 and, with a name sink in `c`, gssd_conv2d_wgrad_kernel_name):
// conv_thin_wgrad.hip: conv1_1 / conv1_2 shapes (patch-staged, wave = phase group); else returns 1
int gssd_try_conv_thin_wgrad(const gssd_conv_desc& d, const float* dy, float* dw, gssd_conv_ctx& c);
// conv_patch_wgrad.hip: conv2_1 .. conv3_3 shapes (patch-staged, one phase group per workgroup); else returns 1
int gssd_try_conv_patch_wgrad(const gssd_conv_desc& d, const float* dy, float* dw, gssd_conv_ctx& c);
// gemm_slot.hip: large plain 1x1 convs / GEMMs as a slot-scheduled 128 x 256 MFMA stream; returns 1 for every other shape
int gssd_try_gemm_slot(const gssd_conv_desc& d, gssd_conv_ctx& c);
// wgrad_slot.hip: weight gradient of large plain 1x1 convs (and the DCN contraction) as a slot-scheduled TN GEMM; else returns 1
int gssd_try_wgrad_slot(const gssd_conv_desc& d, const float* dy, float* dw, gssd_conv_ctx& c);
// conv_thin_bf16.hip: bf16 thin trunk layers (conv1_1 .. conv2_2); returns 1 when the descriptor is not one of them
int gssd_try_conv_thin_bf16(const gssd_conv_desc& d, gssd_conv_ctx& c);
// conv_flat_bf16.hip: bf16 grouped 3x3 trunk layers with 32 .. 128 channels per group (conv3_1 .. conv6); returns 1 when not one of them
int gssd_try_conv_flat_bf16(const gssd_conv_desc& d, gssd_conv_ctx& c);
