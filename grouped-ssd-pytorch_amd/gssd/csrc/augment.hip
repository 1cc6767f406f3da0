// Device SSDAugmentation for gfx950: the pixel half of utils/augmentations.py:548-589 (use_normalize; optional p_only) for a
// whole batch of 4-phase, 3-slice uint8 studies in three launches.  The host planner (gssd/augment.py) draws every random
// number in the reference's order and reduces a study's chain -- ConvertFromInts, PhotometricDistort, Expand, RandomSampleCrop,
// RandomMirror, SubtractMeans, [POnly], Normalize, ResizeFast -- to one gssd_aug_desc.  What is left is per pixel:
//   v = fl32(fl32(fl32(u8 + delta) * alpha) - mean[c])  inside the placed image, 0 on Expand's fill (mean - mean),
//   q = (uint8) fl32(fl32(fl32(v - min) / fl32(max - min)) * 255),   Pillow's 8-bit bicubic resize of q,   fl32(k / 255).
// Pass 1 finds the extrema, pass 2 quantises the window's rows straight from the raw bytes (mirrored index) into LDS and runs the
// horizontal resampling pass, pass 3 the vertical one and the finish.  Every launch covers the batch with per-study geometry.
// Compiled with -ffp-contract=off: each fp32 operation rounds on its own, like the reference's numpy expressions.
#include <math.h>

#include "common.h"
#include "resample8.h"

namespace {

using gssd_resample8::taps8;

constexpr int MM_ROWS = 8;      // source rows per workgroup of the extrema pass
constexpr int H_ROWS = 4;       // crop rows per workgroup of the horizontal pass
constexpr int V_ROWS = 8;       // output rows per workgroup of the vertical pass
constexpr int MAX_LDS = 48 * 1024;

// The window's intersection with the placed image, in source coordinates (empty when y0 >= y1 or x0 >= x1).
struct Extent {
    int y0, y1, x0, x1;
};
__device__ __forceinline__ Extent inside(const gssd_aug_desc& d) {
    Extent e;
    e.y0 = max(d.cy, d.top) - d.top;
    e.y1 = min(d.cy + d.ch, d.top + d.H) - d.top;
    e.x0 = max(d.cx, d.left) - d.left;
    e.x1 = min(d.cx + d.cw, d.left + d.W) - d.left;
    return e;
}

__device__ __forceinline__ float pick3(int c, float a, float b, float d) { return c == 0 ? a : (c == 1 ? b : d); }

// PhotometricDistort then SubtractMeans: three float32 roundings (delta = 0 / alpha = 1 when a branch was not taken: exact no-ops)
__device__ __forceinline__ float pix(int u, float delta, float alpha, float mean) {
    return __fsub_rn(__fmul_rn(__fadd_rn((float)u, delta), alpha), mean);
}

// Normalize + ResizeFast's (v * 255).astype(uint8): the correctly rounded divide, truncation.  A flat study (the reference asserts)
// quantises to 0 here; DeviceSSDAugmentation.check_not_flat() reports it.
__device__ __forceinline__ int quant(float v, float mn, float den) {
    if (!(den > 0.f)) return 0;
    return (int)__fmul_rn(__fdiv_rn(__fsub_rn(v, mn), den), 255.f);
}

// Byte offset of element i of a window row of n columns: interleaved sources (slice stride 1) walk (column, slice), planar ones
// (slice, column), so that consecutive lanes read neighbouring bytes either way.
__device__ __forceinline__ void split(const gssd_aug_desc& d, int i, int n, int& x, int& c) {
    if (d.s_chan == 1) {
        x = i / 3;
        c = i - 3 * x;
    } else {
        c = i / n;
        x = i - c * n;
    }
}

// Pass 1: per-slice byte extrema of the window inside the placed image.  v is a non-decreasing function of the byte for a fixed
// slice (alpha > 0; every rounding is monotone), so the extrema of v are those of the bytes mapped through it -- exact, integer
// atomics.  mm[b][3][2] = (255 - min, max), zeroed by the launcher.
__global__ __launch_bounds__(256) void aug_minmax_kernel(const gssd_aug_desc* __restrict__ desc, int p_only, int* __restrict__ mm) {
    const gssd_aug_desc d = desc[blockIdx.z];
    const Extent e = inside(d);
    const int phase = p_only ? 2 : (int)blockIdx.y;
    const int nx = e.x1 - e.x0, y0 = e.y0 + (int)blockIdx.x * MM_ROWS;
    int lo[3] = {255, 255, 255}, hi[3] = {0, 0, 0};
    if (nx > 0 && y0 < e.y1) {
        const uint8_t* base = reinterpret_cast<const uint8_t*>(d.src) + (long long)phase * d.s_phase;
        const int y1 = min(e.y1, y0 + MM_ROWS), n = 3 * nx;
        for (int y = y0; y < y1; ++y)
            for (int i = threadIdx.x; i < n; i += blockDim.x) {
                int x, c;
                split(d, i, nx, x, c);
                const int u = base[(long long)c * d.s_chan + (long long)y * d.s_y + (long long)(e.x0 + x) * d.s_x];
#pragma unroll
                for (int q = 0; q < 3; ++q)
                    if (q == c) {
                        lo[q] = min(lo[q], u);
                        hi[q] = max(hi[q], u);
                    }
            }
    }
    __shared__ int red[4][6];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        int l = lo[q], h = hi[q];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            l = min(l, __shfl_xor(l, o, 64));
            h = max(h, __shfl_xor(h, o, 64));
        }
        if ((threadIdx.x & 63) == 0) {
            red[threadIdx.x >> 6][2 * q] = h >= l ? 255 - l : 0;
            red[threadIdx.x >> 6][2 * q + 1] = h >= l ? h : 0;
        }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int v = max(max(red[0][threadIdx.x], red[1][threadIdx.x]), max(red[2][threadIdx.x], red[3][threadIdx.x]));
        int* m = mm + blockIdx.z * 6 + threadIdx.x;
        if (v > __atomic_load_n(m, __ATOMIC_RELAXED)) atomicMax(m, v);      // (a stale read is fine, the atomic decides)
    }
}

// Pass 2: a workgroup quantises H_ROWS rows of its study's crop window into LDS (mirrored position, fill outside the placed image)
// and writes their horizontal pass (or the rows themselves when the window is already `size` wide) to work[phase][row][size][3].
__global__ __launch_bounds__(256) void aug_horizontal_kernel(const gssd_aug_desc* __restrict__ desc, const int* __restrict__ mm,
                                                             const int* __restrict__ table, float m0, float m1, float m2,
                                                             uint8_t* __restrict__ work, int ldsrow, int size, int p_only) {
    extern __shared__ __attribute__((aligned(16))) uint8_t qrow[];
    const gssd_aug_desc d = desc[blockIdx.z];
    const int tph = blockIdx.y, phase = p_only ? 2 : tph;
    const int r0 = (int)blockIdx.x * H_ROWS;
    if (r0 >= d.nrows) return;
    const int nr = min(H_ROWS, d.nrows - r0);
    // the study's extrema of v (pass 1 + the fill)
    const Extent e = inside(d);
    float lo = INFINITY, hi = -INFINITY;
    if (e.y0 < e.y1 && e.x0 < e.x1) {
        const int* m = mm + blockIdx.z * 6;
        for (int c = 0; c < 3; ++c) {
            const float mc = pick3(c, m0, m1, m2);
            lo = fminf(lo, pix(255 - m[2 * c], d.delta, d.alpha, mc));
            hi = fmaxf(hi, pix(m[2 * c + 1], d.delta, d.alpha, mc));
        }
    }
    if (d.fill) {
        lo = fminf(lo, 0.f);
        hi = fmaxf(hi, 0.f);
    }
    const float den = __fsub_rn(hi, lo);
    const int qfill = quant(0.f, lo, den);

    const uint8_t* base = reinterpret_cast<const uint8_t*>(d.src) + (long long)phase * d.s_phase;
    const int n = 3 * d.cw;
    for (int i = threadIdx.x; i < nr * n; i += blockDim.x) {
        const int r = i / n;
        int x, c;
        split(d, i - r * n, d.cw, x, c);
        const int Y = d.cy + d.row0 + r0 + r - d.top, X = d.cx + x - d.left;
        int q = qfill;
        if (Y >= 0 && Y < d.H && X >= 0 && X < d.W)
            q = quant(pix(base[(long long)c * d.s_chan + (long long)Y * d.s_y + (long long)X * d.s_x], d.delta, d.alpha,
                          pick3(c, m0, m1, m2)),
                      lo, den);
        const int xm = d.mirror ? d.cw - 1 - x : x;
        qrow[r * ldsrow + 3 * xm + c] = (uint8_t)q;
    }
    __syncthreads();
    const int m = 3 * size;
    uint8_t* out = work + d.work + ((long long)tph * d.nrows + r0) * m;
    for (int i = threadIdx.x; i < nr * m; i += blockDim.x) {
        const int r = i / m, j = i - r * m;
        uint8_t b;
        if (d.hks == 0) {
            b = qrow[r * ldsrow + j];
        } else {
            const int xo = j / 3, c = j - 3 * xo;
            const int x0 = table[d.hb + 2 * xo], nt = table[d.hb + 2 * xo + 1];
            b = taps8(qrow + r * ldsrow + 3 * x0 + c, 3, table + d.hk + xo * d.hks, nt);
        }
        out[(long long)r * m + j] = b;
    }
}

// Pass 3: the vertical pass of V_ROWS output rows and fl32(k / 255) into the network's NCHW input, channel = phase * 3 + slice.
__global__ __launch_bounds__(256) void aug_vertical_kernel(const gssd_aug_desc* __restrict__ desc, const int* __restrict__ table,
                                                           const uint8_t* __restrict__ work, float* __restrict__ out, int size,
                                                           int p_only) {
    const gssd_aug_desc d = desc[blockIdx.z];
    const int phase = blockIdx.y, tph = p_only ? 0 : phase;
    const int m = 3 * size;
    const uint8_t* in = work + d.work + (long long)tph * d.nrows * m;
    float* o = out + ((long long)blockIdx.z * 12 + phase * 3) * size * size;
    const int yend = min(size, ((int)blockIdx.x + 1) * V_ROWS);
    for (int yo = blockIdx.x * V_ROWS; yo < yend; ++yo) {
        int y0 = yo, nt = 0;
        const int* k = nullptr;
        if (d.vks != 0) {
            y0 = table[d.vb + 2 * yo];
            nt = table[d.vb + 2 * yo + 1];
            k = table + d.vk + yo * d.vks;
        }
        const uint8_t* row = in + (long long)(y0 - d.row0) * m;
        for (int i = threadIdx.x; i < m; i += blockDim.x) {
            const int c = i / size, x = i - c * size;
            const uint8_t b = d.vks == 0 ? row[3 * x + c] : taps8(row + 3 * x + c, m, k, nt);
            o[(long long)c * size * size + (long long)yo * size + x] = __fdiv_rn((float)b, 255.f);
        }
    }
}

}  // namespace

extern "C" int gssd_aug_desc_size(void) { return (int)sizeof(gssd_aug_desc); }

extern "C" int gssd_augment_minmax(const gssd_aug_desc* desc, int B, int max_rows, int p_only, int32_t* minmax, gssd_stream_t stream) {
    GSSD_CHECK_ARG(desc && minmax && B > 0 && B <= 65535 && max_rows > 0);
    if (hipMemsetAsync(minmax, 0, (size_t)B * 6 * sizeof(int32_t), as_stream(stream)) != hipSuccess) {
        gssd_set_error("%s:%d: hipMemsetAsync of the extrema failed", __FILE__, __LINE__);
        return GSSD_ELAUNCH;
    }
    hipLaunchKernelGGL(aug_minmax_kernel, dim3((max_rows + MM_ROWS - 1) / MM_ROWS, p_only ? 1 : 4, B), dim3(256), 0, as_stream(stream),
                       desc, p_only, minmax);
    GSSD_CHECK_LAUNCH();
    return GSSD_OK;
}

extern "C" int gssd_augment_horizontal(const gssd_aug_desc* desc, const int32_t* minmax, const int32_t* table, float mean0, float mean1,
                                       float mean2, uint8_t* work, int B, int max_rows, int max_cw, int size, int p_only,
                                       gssd_stream_t stream) {
    GSSD_CHECK_ARG(desc && minmax && table && work && B > 0 && B <= 65535 && max_rows > 0 && max_cw > 0 && size > 0);
    const int ldsrow = (3 * max_cw + 3) & ~3;
    GSSD_CHECK_ARG((size_t)H_ROWS * ldsrow <= (size_t)MAX_LDS);
    hipLaunchKernelGGL(aug_horizontal_kernel, dim3((max_rows + H_ROWS - 1) / H_ROWS, p_only ? 1 : 4, B), dim3(256),
                       (size_t)H_ROWS * ldsrow, as_stream(stream), desc, minmax, table, mean0, mean1, mean2, work, ldsrow, size, p_only);
    GSSD_CHECK_LAUNCH();
    return GSSD_OK;
}

extern "C" int gssd_augment_vertical(const gssd_aug_desc* desc, const int32_t* table, const uint8_t* work, float* out_nchw, int B,
                                     int size, int p_only, gssd_stream_t stream) {
    GSSD_CHECK_ARG(desc && table && work && out_nchw && B > 0 && B <= 65535 && size > 0);
    hipLaunchKernelGGL(aug_vertical_kernel, dim3((size + V_ROWS - 1) / V_ROWS, 4, B), dim3(256), 0, as_stream(stream), desc, table, work,
                       out_nchw, size, p_only);
    GSSD_CHECK_LAUNCH();
    return GSSD_OK;
}
