// DCNv2 sampling for ANY geometry (the standalone operator gssd/dcn_op.py: layers/dcn_v2_custom.py's DCNv2 / DCN / dcn_v2_conv with any
// kernel, stride, padding, dilation and deformable group count).  The engine's 3x3 / stride 1 / pad 1 path keeps csrc/dcn.hip and the
// fused forwards; these two kernels only serve the op.
//
// A unit is one (output pixel, tap, deformable group).  A wave takes 64 consecutive units: lane l computes unit l's sampling geometry
// once (offset / mask loads, optional sigmoid, floor, gate and corner tests), then the wave walks the 64 units with that geometry
// broadcast by v_readlane and the lanes running over the group's channels, so every global access of the channel loop (x corners,
// columns, d(cols), the d(x) atomics) is one contiguous run of up to 64 floats.  Units are ordered (row, tap, group) with the group
// fastest: consecutive units write consecutive pieces of a column row.
//
// Sampling rules (oracle/gssd_oracle.py::dcn_v2_conv): tap k = i*kw + j samples at (ho*sh - ph + i*dh + dy, wo*sw - pw + j*dw + dx),
// dy = offset[d*2K + 2k], dx = offset[d*2K + 2k + 1], m = mask[d*K + k] (or sigmoid of it); zero unless -1 < y < H and -1 < x < W;
// bilinear with the corners outside the map contributing 0.  floor() and the gates are constants of the differentiation.
//
// All element offsets are 64-bit.
#include "common.h"

namespace {

struct GeoArgs {
    gssd_dcn_geom g;
    int b0, rows, K, Cp, cpg, HoWo;
    long long units;
};

// one unit's sampling geometry; xo = element offset of the (y0, x0) corner's first channel of the group (only dereferenced for a
// corner whose bit is set in `ok`)
struct UnitGeo {
    float ly, lx, m;
    int ok;
    long long xo, dst, oo, mo;
};

__device__ __forceinline__ UnitGeo unit_geo(const GeoArgs& a, const float* __restrict__ off, const float* __restrict__ msk,
                                            long long u) {
    const gssd_dcn_geom& g = a.g;
    const int d = (int)(u % g.dg);
    const long long t = u / g.dg;
    const int k = (int)(t % a.K);
    const long long row = t / a.K;                                // pixel row of the chunk's column matrix
    const int p = (int)(row % a.HoWo);
    const int b = a.b0 + (int)(row / a.HoWo);
    const int ho = p / g.Wo, wo = p - ho * g.Wo;
    const int i = k / g.kw, j = k - i * g.kw;
    const long long pix = (long long)b * a.HoWo + p;
    UnitGeo r;
    r.oo = pix * g.off_stride + (long long)d * 2 * a.K + 2 * k;
    r.mo = pix * g.mask_stride + (long long)d * a.K + k;
    r.dst = row * ((long long)a.K * a.Cp) + (long long)k * a.Cp + (long long)d * a.cpg;
    const float oy = off[r.oo], ox = off[r.oo + 1];
    const float mv = msk[r.mo];
    r.m = g.mask_logit ? 1.f / (1.f + expf(-mv)) : mv;
    const float py = (float)(ho * g.sh - g.ph + i * g.dh) + oy;
    const float px = (float)(wo * g.sw - g.pw + j * g.dw) + ox;
    r.ly = 0.f;
    r.lx = 0.f;
    r.ok = 0;
    r.xo = 0;
    if (py > -1.f && px > -1.f && py < (float)g.H && px < (float)g.W) {   // (false for NaN offsets too)
        const float y0f = floorf(py), x0f = floorf(px);
        const int y0 = (int)y0f, x0 = (int)x0f;
        r.ly = py - y0f;
        r.lx = px - x0f;
        const bool y0ok = y0 >= 0, y1ok = y0 + 1 <= g.H - 1, x0ok = x0 >= 0, x1ok = x0 + 1 <= g.W - 1;
        r.ok = ((y0ok && x0ok) ? 1 : 0) | ((y0ok && x1ok) ? 2 : 0) | ((y1ok && x0ok) ? 4 : 0) | ((y1ok && x1ok) ? 8 : 0);
        r.xo = (((long long)b * g.H + y0) * g.W + x0) * g.x_stride + (long long)d * a.cpg;
    }
    return r;
}

__device__ __forceinline__ float rlf(float v, int j) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), j));
}
__device__ __forceinline__ long long rl64(long long v, int j) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v & 0xffffffffll), j);
    const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)((unsigned long long)v >> 32), j);
    return (long long)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ float wave_sum(float v) {
    // xor butterfly: both partners of every step add the same two values, so all 64 lanes end with the same, order-fixed sum
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(256) void dcn_geo_im2col_kernel(const float* __restrict__ x, const float* __restrict__ off,
                                                             const float* __restrict__ msk, float* __restrict__ cols, GeoArgs a) {
    const int lane = threadIdx.x & 63;
    const long long wave0 = (blockIdx.x * (long long)blockDim.x + threadIdx.x) >> 6;
    const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    const long long xs = a.g.x_stride, rs = (long long)a.g.W * a.g.x_stride;
    const int cpg = a.cpg, pad = a.Cp - a.g.C, dlast = a.g.dg - 1;
    for (long long base = wave0 * 64; base < a.units; base += nwaves * 64) {
        const long long u = base + lane;
        const UnitGeo q = unit_geo(a, off, msk, u < a.units ? u : a.units - 1);
        const float hy = 1.f - q.ly, hx = 1.f - q.lx;
        const float q00 = hy * hx * q.m, q01 = hy * q.lx * q.m, q10 = q.ly * hx * q.m, q11 = q.ly * q.lx * q.m;
        const int nj = (int)((a.units - base) < 64 ? (a.units - base) : 64);
        for (int j = 0; j < nj; ++j) {
            const int ok = __builtin_amdgcn_readlane(q.ok, j);
            const float w00 = (ok & 1) ? rlf(q00, j) : 0.f, w01 = (ok & 2) ? rlf(q01, j) : 0.f;
            const float w10 = (ok & 4) ? rlf(q10, j) : 0.f, w11 = (ok & 8) ? rlf(q11, j) : 0.f;
            const float* p00 = x + rl64(q.xo, j);
            float* dst = cols + rl64(q.dst, j);
            for (int c = lane; c < cpg; c += 64) {
                float v = 0.f;
                if (ok & 1) v += w00 * p00[c];
                if (ok & 2) v += w01 * p00[xs + c];
                if (ok & 4) v += w10 * p00[rs + c];
                if (ok & 8) v += w11 * p00[rs + xs + c];
                dst[c] = v;
            }
            // zero pad columns [C, Cp) of the tap: written by the last group's unit
            if (pad && lane < pad && (int)((base + j) % a.g.dg) == dlast) dst[cpg + lane] = 0.f;
        }
    }
}

__global__ __launch_bounds__(256) void dcn_geo_col2im_kernel(const float* __restrict__ x, const float* __restrict__ off,
                                                             const float* __restrict__ msk, const float* __restrict__ dcols,
                                                             float* __restrict__ dx, float* __restrict__ doff, float* __restrict__ dmsk,
                                                             GeoArgs a) {
    const int lane = threadIdx.x & 63;
    const long long wave0 = (blockIdx.x * (long long)blockDim.x + threadIdx.x) >> 6;
    const long long nwaves = ((long long)gridDim.x * blockDim.x) >> 6;
    const long long xs = a.g.x_stride, rs = (long long)a.g.W * a.g.x_stride;
    const int cpg = a.cpg;
    const bool want_om = doff != nullptr;
    for (long long base = wave0 * 64; base < a.units; base += nwaves * 64) {
        const long long u = base + lane;
        const UnitGeo q = unit_geo(a, off, msk, u < a.units ? u : a.units - 1);
        const int nj = (int)((a.units - base) < 64 ? (a.units - base) : 64);
        float ry = 0.f, rx = 0.f, rm = 0.f;                       // this lane's unit: d(offset_y), d(offset_x) / m, d(mask)
        for (int j = 0; j < nj; ++j) {
            const int ok = __builtin_amdgcn_readlane(q.ok, j);
            const float ly = rlf(q.ly, j), lx = rlf(q.lx, j), m = rlf(q.m, j);
            const float hy = 1.f - ly, hx = 1.f - lx;
            const long long xo = rl64(q.xo, j);
            const float* g = dcols + rl64(q.dst, j);
            float sy = 0.f, sx = 0.f, sm = 0.f;
            if (ok) {                                             // (a gated sample has zero value and zero derivatives)
                for (int c = lane; c < cpg; c += 64) {
                    const float gc = g[c];
                    const float* p = x + xo + c;
                    const float v00 = (ok & 1) ? p[0] : 0.f, v01 = (ok & 2) ? p[xs] : 0.f;
                    const float v10 = (ok & 4) ? p[rs] : 0.f, v11 = (ok & 8) ? p[rs + xs] : 0.f;
                    sm += gc * (hy * (hx * v00 + lx * v01) + ly * (hx * v10 + lx * v11));
                    sy += gc * (hx * (v10 - v00) + lx * (v11 - v01));
                    sx += gc * (hy * (v01 - v00) + ly * (v11 - v10));
                    if (dx) {
                        const float gm = gc * m;
                        float* t = dx + xo + c;
                        if (ok & 1) unsafeAtomicAdd(t, gm * (hy * hx));
                        if (ok & 2) unsafeAtomicAdd(t + xs, gm * (hy * lx));
                        if (ok & 4) unsafeAtomicAdd(t + rs, gm * (ly * hx));
                        if (ok & 8) unsafeAtomicAdd(t + rs + xs, gm * (ly * lx));
                    }
                }
            }
            if (want_om) {
                sy = wave_sum(sy);
                sx = wave_sum(sx);
                sm = wave_sum(sm);
                if (lane == j) {
                    ry = sy;
                    rx = sx;
                    rm = sm;
                }
            }
        }
        if (want_om && u < a.units) {
            doff[q.oo] = ry * q.m;
            doff[q.oo + 1] = rx * q.m;
            dmsk[q.mo] = a.g.mask_logit ? rm * q.m * (1.f - q.m) : rm;
        }
    }
}

int geo_args(GeoArgs& a, const gssd_dcn_geom* gp, int b0, int b1) {
    GSSD_CHECK_ARG(gp != nullptr);
    const gssd_dcn_geom& g = *gp;
    GSSD_CHECK_ARG(g.B > 0 && g.H > 0 && g.W > 0 && g.C > 0 && g.dg > 0 && g.C % g.dg == 0 && g.x_stride >= g.C);
    GSSD_CHECK_ARG(g.kh > 0 && g.kw > 0 && g.sh > 0 && g.sw > 0 && g.dh > 0 && g.dw > 0 && g.ph >= 0 && g.pw >= 0);
    GSSD_CHECK_ARG(g.Ho > 0 && g.Wo > 0 && (g.H + 2 * g.ph - g.dh * (g.kh - 1) - 1) / g.sh + 1 == g.Ho &&
                   (g.W + 2 * g.pw - g.dw * (g.kw - 1) - 1) / g.sw + 1 == g.Wo);
    GSSD_CHECK_ARG(g.mask_logit == 0 || g.mask_logit == 1);
    GSSD_CHECK_ARG(0 <= b0 && b0 < b1 && b1 <= g.B);
    // 32-bit products inside the kernels: pixel counts per image, the sampling coordinates, the column row length
    const long long K = (long long)g.kh * g.kw, Cp = (g.C + 3) / 4 * 4;
    GSSD_CHECK_ARG((long long)g.H * g.W < (1ll << 31) && (long long)g.Ho * g.Wo < (1ll << 31) && K * Cp < (1ll << 31));
    GSSD_CHECK_ARG((long long)g.Ho * g.sh + (long long)g.kh * g.dh + g.H < (1ll << 24) &&
                   (long long)g.Wo * g.sw + (long long)g.kw * g.dw + g.W < (1ll << 24));   // integer positions exact in fp32
    GSSD_CHECK_ARG((long long)g.off_stride >= 2 * g.dg * K && (long long)g.mask_stride >= g.dg * K);
    a.g = g;
    a.b0 = b0;
    a.rows = b1 - b0;
    a.K = (int)K;
    a.Cp = (int)Cp;
    a.cpg = g.C / g.dg;
    a.HoWo = g.Ho * g.Wo;
    a.units = (long long)a.rows * a.HoWo * K * g.dg;
    return GSSD_OK;
}

dim3 geo_grid(long long units) {
    long long blocks = (units + 255) / 256;                      // a wave per 64 units
    if (blocks > 16384) blocks = 16384;
    return dim3((unsigned)blocks);
}

}  // namespace

extern "C" int gssd_dcn_geo_im2col_f32(const float* x, const float* offset, const float* mask, float* cols, const gssd_dcn_geom* geom,
                                       int b0, int b1, gssd_stream_t stream) {
    GSSD_CHECK_ARG(x && offset && mask && cols);
    GeoArgs a;
    const int rc = geo_args(a, geom, b0, b1);
    if (rc != GSSD_OK) return rc;
    hipLaunchKernelGGL(dcn_geo_im2col_kernel, geo_grid(a.units), dim3(256), 0, as_stream(stream), x, offset, mask, cols, a);
    GSSD_CHECK_LAUNCH();
    return GSSD_OK;
}

extern "C" int gssd_dcn_geo_col2im_f32(const float* x, const float* offset, const float* mask, const float* dcols, float* dx,
                                       float* doffset, float* dmask, const gssd_dcn_geom* geom, int b0, int b1, gssd_stream_t stream) {
    GSSD_CHECK_ARG(x && offset && mask && dcols && (doffset == nullptr) == (dmask == nullptr) && (dx || doffset));
    GeoArgs a;
    const int rc = geo_args(a, geom, b0, b1);
    if (rc != GSSD_OK) return rc;
    hipLaunchKernelGGL(dcn_geo_col2im_kernel, geo_grid(a.units), dim3(256), 0, as_stream(stream), x, offset, mask, dcols, dx, doffset,
                       dmask, a);
    GSSD_CHECK_LAUNCH();
    return GSSD_OK;
}
