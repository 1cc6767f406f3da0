// The box tail of PixelLink's mask_to_box on the device (ssd_liverdet/pixel_link/postprocess.py:124-160 as pixel_link/box_geometry.py defines
// it): label map [h][w] + pixel logits -> per image the rows (score, min x, min y, max x, max y) of the components the reference's filters keep.
//
// One workgroup of 16 waves per image, everything in LDS, the arithmetic of box_geometry.py operation for operation (this file is compiled with
// -ffp-contract=off: every product and sum below rounds on its own, like numpy's):
//   0. index tables of the nearest up-scaling, built once per workgroup: ys[Y] = min(int(Y * (h / Hd)), h - 1) in float64 (xs alike) and their
//      inverses (the destination rows / columns that read one source row / column: a contiguous, possibly empty range since ys is monotone);
//      the positive-class probability float32(1 / (1 + exp(float64(l0 - l1)))) of every source pixel; the source bounding box of every label.
//   1. one pass over the Hd x Wd destination pixels: upscale_bilinear of the probability in fp32 (half-pixel centres, border replicated, the
//      i0 < 0 branch), added in float64 to its label's sum.  Waves whose 64 pixels carry one label add once; the sums are LDS float64
//      atomics, so their last bit may depend on arrival order -- 1e-16 of a value that is then rounded to fp32.  The host definition takes
//      numpy's float32 `.mean()` (pairwise float32 sums) here: the two scores agree to a few fp32 ulps, not bit for bit.
//   2. one wave per component: per source row of its box the leftmost / rightmost destination column of the component, at the first and
//      last destination row of that source row -- at most four hull candidates per (component, source row).  Candidates arrive sorted by
//      row, so the right and the left hull chain are two monotone-chain stacks (exact integer cross products, collinear points dropped);
//      right chain downwards + left chain upwards is convex_hull's orientation, rotated to start at the lowest-x-then-lowest-y vertex.
//      Rotating calipers in float64: 64 edges' rectangles at a time over the lanes, the choice among them the definition's sequential scan
//      (area < best - 1e-9 * max(1, best), first edge wins); filters, corners trunc(rint(c * 1e6) / 1e6) clamped into the image.
//   3. kept components squeezed together in label order (component_boxes' order), or with by_score in descending score order, equal scores
//      in label order (a rank count over the <= 1024 kept scores): the order gssd_eval_match expects of an image's rows.  Rows ndet ..
//      max_det - 1 zeroed.
// Limits (the launcher returns GSSD_EINVAL before any launch, nothing written): h, w, Hd, Wd, B > 0; h * w <= 26624 (the decode's limit);
// Hd, Wd <= 65536 and Hd * Wd <= 2^22 (step 1 is Hd * Wd / 1024 iterations per thread: a bound on the kernel's running time); 1 <= max_det <= 1024 (the decode's statistics table); det_stride >= 5 * max_det; the tables (4 h w bytes of probabilities,
// 2 (Hd + Wd) + 8 (h + w) bytes of index tables, 44 KB per-component state) within the CU's 160 KB of LDS -- 150 x 150 -> 300 x 300 takes 139 KB.
// Labels above max_det (or above ncomp[b] when ncomp is given) are ignored: the caller decides what more components than that mean.
#include <limits.h>
#include <math.h>
#include "common.h"

namespace {

constexpr int PB_THREADS = 1024, PB_WAVES = PB_THREADS / 64;
constexpr int PB_MAX_DET = 1024;         // = PL_STAT_COMPS of pixellink.hip
constexpr int PB_MAXPIX = 26624;         // = PL_MAXPIX_LDS of pixellink.hip
constexpr size_t PB_LDS_MAX = 160 * 1024;
constexpr long long PB_MAX_DST = 1ll << 22;      // destination pixels per image

struct PbLayout {                        // byte offsets into dynamic LDS
    unsigned dsum, cnt, bbox, score, box, pre, ylo, yhi, xlo, xhi, ys, xs, uni, misc, total;
    int cap;                             // points per hull chain: min(2 h, Hd)
};

inline PbLayout pb_layout(int h, int w, int Hd, int Wd) {
    PbLayout L;
    size_t o = 0;
    auto take = [&o](size_t bytes) {
        const size_t at = o;
        o += (bytes + 15) / 16 * 16;
        return (unsigned)at;
    };
    L.dsum = take(PB_MAX_DET * 8);
    L.cnt = take(PB_MAX_DET * 4);
    L.bbox = take(PB_MAX_DET * 16);
    L.score = take(PB_MAX_DET * 4);
    L.box = take(PB_MAX_DET * 8);
    L.pre = take(PB_MAX_DET * 4);
    L.ylo = take((size_t)h * 4);
    L.yhi = take((size_t)h * 4);
    L.xlo = take((size_t)w * 4);
    L.xhi = take((size_t)w * 4);
    L.ys = take((size_t)Hd * 2);
    L.xs = take((size_t)Wd * 2);
    L.misc = take(16);
    L.cap = 2 * h < Hd ? 2 * h : Hd;
    const size_t prob = (size_t)h * w * 4, stacks = (size_t)PB_WAVES * 2 * L.cap * 4;
    L.uni = take(prob > stacks ? prob : stacks);       // probabilities (steps 0, 1), then the hull stacks (step 2)
    L.total = o > 0xffffffffu ? 0xffffffffu : (unsigned)o;
    return L;
}

// one axis of upscale_bilinear: s = (i + 0.5) * float32(n_in / n_out) - 0.5 in fp32, f = float32(s - floor(s)), 0 where floor(s) < 0
__device__ __forceinline__ void pb_axis(int idx, float scale, int n_in, int& lo, int& hi, float& f) {
    const float s = ((float)idx + 0.5f) * scale - 0.5f;
    const float fl = floorf(s);
    const int i0 = (int)fl;
    f = i0 < 0 ? 0.f : (float)((double)s - (double)fl);
    lo = i0 < 0 ? 0 : i0 > n_in - 1 ? n_in - 1 : i0;
    hi = i0 + 1 < 0 ? 0 : i0 + 1 > n_in - 1 ? n_in - 1 : i0 + 1;
}

__device__ __forceinline__ int pb_wave_min(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int pb_wave_max(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}

// Monotone-chain push (every lane of the wave runs it with the same values).  sign = +1: the right chain keeps cross > 0, -1: the left chain
// keeps cross < 0, both walking down the rows.  Points are packed x << 16 | y.
__device__ __forceinline__ void pb_push(unsigned* chain, int& n, int cap, int px, int py, int sign) {
    while (n >= 2) {
        const unsigned a = chain[n - 2], b = chain[n - 1];
        const long long ax = a >> 16, ay = a & 0xffffu, bx = b >> 16, by = b & 0xffffu;
        const long long cr = (bx - ax) * (py - ay) - (by - ay) * (px - ax);
        if (sign * cr <= 0) --n;
        else break;
    }
    if (n < cap) chain[n++] = ((unsigned)px << 16) | (unsigned)py;
}

struct PbHull {                          // the cyclic vertex sequence: right chain downwards, then the left chain upwards, from `start`
    const unsigned* R;
    const unsigned* Lc;
    int nR, nL, dup_bot, nv, start;
    __device__ __forceinline__ unsigned seq(int j) const { return j < nR ? R[j] : Lc[nL - 1 - dup_bot - (j - nR)]; }
    __device__ __forceinline__ unsigned at(int i) const {
        int j = start + i;
        if (j >= nv) j -= nv;
        return seq(j);
    }
};

struct PbRect {
    double u0, u1, a0, a1, b0, b1, area;
};

// the candidate rectangle of hull edge i (min_area_rect's loop body)
__device__ __forceinline__ PbRect pb_rect(const PbHull& H, int i) {
    const unsigned p = H.at(i), q = H.at(i + 1 == H.nv ? 0 : i + 1);
    const int ex = (int)(q >> 16) - (int)(p >> 16), ey = (int)(q & 0xffffu) - (int)(p & 0xffffu);
    const double len = __dsqrt_rn((double)((long long)ex * ex + (long long)ey * ey));      // correctly rounded: the exact integer's root
    PbRect r;
    r.u0 = (double)ex / len;
    r.u1 = (double)ey / len;
    const double v0 = -r.u1, v1 = r.u0;
    r.a0 = r.b0 = INFINITY;
    r.a1 = r.b1 = -INFINITY;
    for (int k = 0; k < H.nv; ++k) {
        const unsigned t = H.at(k);
        const double x = (double)(t >> 16), y = (double)(t & 0xffffu);
        const double a = x * r.u0 + y * r.u1, b = x * v0 + y * v1;
        r.a0 = fmin(r.a0, a);
        r.a1 = fmax(r.a1, a);
        r.b0 = fmin(r.b0, b);
        r.b1 = fmax(r.b1, b);
    }
    r.area = (r.a1 - r.a0) * (r.b1 - r.b0);
    return r;
}

// rect_corners_int for one coordinate: trunc(np.round(c, 6)) clamped to [0, n - 1]
__device__ __forceinline__ int pb_corner(double c, int n) {
    const double t = trunc(rint(c * 1e6) / 1e6);
    return t < 0.0 ? 0 : t > (double)(n - 1) ? n - 1 : (int)t;
}

__global__ __launch_bounds__(PB_THREADS) void pl_boxes_kernel(const int* __restrict__ labels, const float* __restrict__ out1,
                                                              const int* __restrict__ ncomp, float* __restrict__ det, long long det_stride,
                                                              int* __restrict__ ndet, int h, int w, int Hd, int Wd, double min_height,
                                                              double min_area, int max_det, int by_score, PbLayout L) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* dsum = reinterpret_cast<double*>(smem + L.dsum);
    int* cnt = reinterpret_cast<int*>(smem + L.cnt);
    int* bbox = reinterpret_cast<int*>(smem + L.bbox);                  // [k][4] = min row, max row, min column, max column (source)
    float* score = reinterpret_cast<float*>(smem + L.score);
    unsigned short* box = reinterpret_cast<unsigned short*>(smem + L.box);
    int* pre = reinterpret_cast<int*>(smem + L.pre);                    // kept flag, then the output row (-1: dropped)
    int* ylo = reinterpret_cast<int*>(smem + L.ylo);
    int* yhi = reinterpret_cast<int*>(smem + L.yhi);
    int* xlo = reinterpret_cast<int*>(smem + L.xlo);
    int* xhi = reinterpret_cast<int*>(smem + L.xhi);
    unsigned short* ys = reinterpret_cast<unsigned short*>(smem + L.ys);
    unsigned short* xs = reinterpret_cast<unsigned short*>(smem + L.xs);
    int* misc = reinterpret_cast<int*>(smem + L.misc);                  // [0] largest label seen, [1] ndet
    float* prob = reinterpret_cast<float*>(smem + L.uni);
    unsigned* stacks = reinterpret_cast<unsigned*>(smem + L.uni);

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hw = h * w;
    const int* lab = labels + (size_t)b * hw;
    const float* l0 = out1 + (size_t)b * 2 * hw;
    const float* l1 = l0 + hw;

    // ---- 0. tables ----------------------------------------------------------------------------------------------------------------------
    if (tid < 2) misc[tid] = 0;
    for (int k = tid; k < PB_MAX_DET; k += PB_THREADS) {
        dsum[k] = 0.0;
        cnt[k] = 0;
        bbox[4 * k + 0] = INT_MAX;
        bbox[4 * k + 1] = -1;
        bbox[4 * k + 2] = INT_MAX;
        bbox[4 * k + 3] = -1;
        pre[k] = 0;
    }
    const double sy = (double)h / (double)Hd, sx = (double)w / (double)Wd;
    for (int Y = tid; Y < Hd; Y += PB_THREADS) {
        const int r = (int)((double)Y * sy);
        ys[Y] = (unsigned short)(r < h - 1 ? r : h - 1);
    }
    for (int X = tid; X < Wd; X += PB_THREADS) {
        const int c = (int)((double)X * sx);
        xs[X] = (unsigned short)(c < w - 1 ? c : w - 1);
    }
    for (int r = tid; r < h; r += PB_THREADS) {                          // empty range until a destination row claims it
        ylo[r] = 1;
        yhi[r] = 0;
    }
    for (int c = tid; c < w; c += PB_THREADS) {
        xlo[c] = 1;
        xhi[c] = 0;
    }
    __syncthreads();
    for (int Y = tid; Y < Hd; Y += PB_THREADS) {
        const int r = ys[Y];
        if (Y == 0 || ys[Y - 1] != r) ylo[r] = Y;
        if (Y == Hd - 1 || ys[Y + 1] != r) yhi[r] = Y;
    }
    for (int X = tid; X < Wd; X += PB_THREADS) {
        const int c = xs[X];
        if (X == 0 || xs[X - 1] != c) xlo[c] = X;
        if (X == Wd - 1 || xs[X + 1] != c) xhi[c] = X;
    }
    int seen = 0;
    for (int i0 = 0; i0 < hw; i0 += PB_THREADS) {
        const int i = i0 + tid;
        int id = -1, r = 0, c = 0;
        if (i < hw) {
            prob[i] = (float)(1.0 / (1.0 + exp((double)(l0[i] - l1[i]))));
            const int l = lab[i];
            seen = l > seen ? l : seen;
            if (l >= 1 && l <= max_det) id = l - 1;
            r = i / w;
            c = i - r * w;
        }
        // a wave whose labelled pixels all belong to one component (64 consecutive pixels inside a large one) reduces first
        const unsigned long long act = __ballot(id >= 0);
        if (act == 0ull) continue;
        const int id0 = __builtin_amdgcn_readlane(id, __builtin_ctzll(act));
        if (__ballot(id >= 0 && id != id0) == 0ull) {
            const int r0 = pb_wave_min(id >= 0 ? r : INT_MAX), r1 = pb_wave_max(id >= 0 ? r : -1);
            const int c0 = pb_wave_min(id >= 0 ? c : INT_MAX), c1 = pb_wave_max(id >= 0 ? c : -1);
            if (lane == 0) {
                atomicMin(&bbox[4 * id0 + 0], r0);
                atomicMax(&bbox[4 * id0 + 1], r1);
                atomicMin(&bbox[4 * id0 + 2], c0);
                atomicMax(&bbox[4 * id0 + 3], c1);
            }
        } else if (id >= 0) {
            atomicMin(&bbox[4 * id + 0], r);
            atomicMax(&bbox[4 * id + 1], r);
            atomicMin(&bbox[4 * id + 2], c);
            atomicMax(&bbox[4 * id + 3], c);
        }
    }
    if (!ncomp) {
        seen = pb_wave_max(seen);
        if (lane == 0) atomicMax(&misc[0], seen);
    }
    __syncthreads();
    int n = ncomp ? ncomp[b] : misc[0];
    n = n < 0 ? 0 : n > max_det ? max_det : n;

    // ---- 1. score sums over the destination pixels ---------------------------------------------------------------------------------------
    const float fsy = (float)sy, fsx = (float)sx;
    const long long dtotal = (long long)Hd * Wd;
    for (long long i0 = 0; i0 < dtotal; i0 += PB_THREADS) {
        const long long i = i0 + tid;
        int id = -1;
        float val = 0.f;
        if (i < dtotal) {
            const int Y = (int)(i / Wd), X = (int)(i - (long long)Y * Wd);
            const int l = lab[(int)ys[Y] * w + (int)xs[X]];
            if (l >= 1 && l <= n) {
                id = l - 1;
                int y0, y1, x0, x1;
                float fy, fx;
                pb_axis(Y, fsy, h, y0, y1, fy);
                pb_axis(X, fsx, w, x0, x1, fx);
                const float top = prob[y0 * w + x0] * (1.f - fx) + prob[y0 * w + x1] * fx;
                const float bot = prob[y1 * w + x0] * (1.f - fx) + prob[y1 * w + x1] * fx;
                val = top * (1.f - fy) + bot * fy;
            }
        }
        const unsigned long long act = __ballot(id >= 0);
        if (act == 0ull) continue;
        const int id0 = __builtin_amdgcn_readlane(id, __builtin_ctzll(act));
        if (__ballot(id >= 0 && id != id0) == 0ull) {
            const double s = wave_sum(id >= 0 ? (double)val : 0.0);
            if (lane == 0) {
                atomicAdd(&dsum[id0], s);
                atomicAdd(&cnt[id0], (int)__builtin_popcountll(act));
            }
        } else if (id >= 0) {
            atomicAdd(&dsum[id], (double)val);
            atomicAdd(&cnt[id], 1);
        }
    }
    __syncthreads();                                                     // the probabilities are dead: their LDS becomes the hull stacks

    // ---- 2. one wave per component: hull, calipers, filters, corners ----------------------------------------------------------------------
    const int cap = L.cap;
    unsigned* R = stacks + (size_t)wave * 2 * cap;
    unsigned* Lc = R + cap;
    for (int k = wave; k < n; k += PB_WAVES) {
        const int rmin = bbox[4 * k + 0], rmax = bbox[4 * k + 1], cmin = bbox[4 * k + 2], cmax = bbox[4 * k + 3];
        const int pixels = cnt[k];
        if (pixels <= 0 || rmax < rmin) continue;                        // no destination pixel (len(ys) == 0): skipped
        int nR = 0, nL = 0;
        for (int r = rmin; r <= rmax; ++r) {
            const int ya = ylo[r], yb = yhi[r];
            if (ya > yb) continue;                                       // no destination row reads this source row
            int xl = INT_MAX, xr = -1;
            for (int c0 = cmin; c0 <= cmax; c0 += 256) {
                int v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {                            // four loads in flight per lane
                    const int c = c0 + lane + 64 * j;
                    v[j] = c <= cmax ? lab[r * w + c] : 0;
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = c0 + lane + 64 * j;
                    if (v[j] == k + 1 && xlo[c] <= xhi[c]) {
                        xl = min(xl, xlo[c]);
                        xr = max(xr, xhi[c]);
                    }
                }
            }
            xl = pb_wave_min(xl);
            xr = pb_wave_max(xr);
            if (xr < 0) continue;
            pb_push(R, nR, cap, xr, ya, 1);
            pb_push(Lc, nL, cap, xl, ya, -1);
            if (yb != ya) {
                pb_push(R, nR, cap, xr, yb, 1);
                pb_push(Lc, nL, cap, xl, yb, -1);
            }
        }
        if (nR == 0) continue;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        PbHull H;
        H.R = R;
        H.Lc = Lc;
        H.nR = nR;
        H.nL = nL;
        const int dup_top = R[0] == Lc[0], dup_bot = R[nR - 1] == Lc[nL - 1];
        H.dup_bot = dup_bot;
        H.nv = (nR == 1 && nL == 1 && dup_top) ? 1 : nR + nL - dup_top - dup_bot;
        H.start = 0;
        unsigned long long lowest = ~0ull;                               // packed point << 32 | index: the lowest x, then the lowest y
        for (int j = lane; j < H.nv; j += 64) {
            const unsigned long long key = ((unsigned long long)H.seq(j) << 32) | (unsigned)j;
            lowest = key < lowest ? key : lowest;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(lowest, o, 64);
            lowest = other < lowest ? other : lowest;
        }
        H.start = (int)(lowest & 0xffffffffu);

        double w_ = 0.0, h_ = 0.0, area = 0.0, cx[4], cy[4];
        if (H.nv == 1) {
            const unsigned p = H.at(0);
            for (int q = 0; q < 4; ++q) {
                cx[q] = (double)(p >> 16);
                cy[q] = (double)(p & 0xffffu);
            }
        } else {
            const int ne = H.nv > 2 ? H.nv : 1;
            bool have = false;
            double best = 0.0;
            int ib = 0;
            for (int base = 0; base < ne; base += 64) {
                const int i = base + lane;
                const double mine = i < ne ? pb_rect(H, i).area : 0.0;
                const int m = ne - base < 64 ? ne - base : 64;
                for (int j = 0; j < m; ++j) {                            // the definition's sequential scan, the same in every lane
                    const double aj = __shfl(mine, j, 64);
                    if (!have || aj < best - 1e-9 * fmax(1.0, best)) {
                        best = aj;
                        ib = base + j;
                        have = true;
                    }
                }
            }
            const PbRect rc = pb_rect(H, ib);
            w_ = rc.a1 - rc.a0;
            h_ = rc.b1 - rc.b0;
            area = rc.area;
            const double v0 = -rc.u1, v1 = rc.u0;
            const double ca[4] = {rc.a0, rc.a1, rc.a1, rc.a0}, cb[4] = {rc.b0, rc.b0, rc.b1, rc.b1};
            for (int q = 0; q < 4; ++q) {
                cx[q] = ca[q] * rc.u0 + cb[q] * v0;
                cy[q] = ca[q] * rc.u1 + cb[q] * v1;
            }
        }
        if (fmin(w_, h_) < min_height || area < min_area) continue;
        int x0 = INT_MAX, y0 = INT_MAX, x1 = -1, y1 = -1;
        for (int q = 0; q < 4; ++q) {
            const int ix = pb_corner(cx[q], Wd), iy = pb_corner(cy[q], Hd);
            x0 = min(x0, ix);
            x1 = max(x1, ix);
            y0 = min(y0, iy);
            y1 = max(y1, iy);
        }
        if (lane == 0) {
            box[4 * k + 0] = (unsigned short)x0;
            box[4 * k + 1] = (unsigned short)y0;
            box[4 * k + 2] = (unsigned short)x1;
            box[4 * k + 3] = (unsigned short)y1;
            score[k] = (float)(dsum[k] / (double)pixels);
            pre[k] = 1;
        }
    }
    __syncthreads();

    // ---- 3. label order, dropped components squeezed out ----------------------------------------------------------------------------------
    if (tid < 64) {                                                      // wave 0: 16 flags per lane, then a 64-lane scan
        int loc[16], run = 0;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            loc[t] = run;
            run += pre[tid * 16 + t];
        }
        int inc = run;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(inc, o, 64);
            if (tid >= o) inc += v;
        }
        const int excl = inc - run;
#pragma unroll
        for (int t = 0; t < 16; ++t) pre[tid * 16 + t] = pre[tid * 16 + t] ? excl + loc[t] : -1;
        if (tid == 63) misc[1] = inc;
    }
    __syncthreads();
    const int kept = misc[1];
    float* out = det + (size_t)b * det_stride;
    for (int k = tid; k < n; k += PB_THREADS) {
        int row = pre[k];
        if (row < 0) continue;
        if (by_score) {                                                  // rank among the kept scores
            const float s = score[k];
            row = 0;
            for (int j = 0; j < n; ++j) row += pre[j] >= 0 && (score[j] > s || (score[j] == s && j < k));
        }
        out[row * 5 + 0] = score[k];
#pragma unroll
        for (int q = 0; q < 4; ++q) out[row * 5 + 1 + q] = (float)box[4 * k + q];
    }
    for (int i = kept * 5 + tid; i < max_det * 5; i += PB_THREADS) out[i] = 0.f;
    if (tid == 0) ndet[b] = kept;
}

}  // namespace

extern "C" int gssd_pixellink_boxes_f32(const int* labels, const float* out1, const int* ncomp, float* det, long long det_stride, int* ndet,
                                        int B, int h, int w, int Hd, int Wd, double min_height, double min_area, int max_det, int by_score,
                                        gssd_stream_t stream) {
    GSSD_CHECK_ARG(labels && out1 && det && ndet && B > 0 && h > 0 && w > 0 && Hd > 0 && Wd > 0);
    GSSD_CHECK_ARG((long long)h * w <= PB_MAXPIX && Hd <= 65536 && Wd <= 65536 && (long long)Hd * Wd <= PB_MAX_DST && max_det >= 1 && max_det <= PB_MAX_DET);
    GSSD_CHECK_ARG(det_stride >= 5ll * max_det);
    const PbLayout L = pb_layout(h, w, Hd, Wd);
    GSSD_CHECK_ARG(L.total <= PB_LDS_MAX);
    static unsigned attr_mask = 0;
    if (const int rc = gssd_max_dynamic_lds(&attr_mask, pl_boxes_kernel, PB_LDS_MAX)) return rc;
    hipLaunchKernelGGL(pl_boxes_kernel, dim3(B), dim3(PB_THREADS), L.total, as_stream(stream), labels, out1, ncomp, det, det_stride, ndet, h,
                       w, Hd, Wd, min_height, min_area, max_det, by_score, L);
    GSSD_CHECK_LAUNCH();
    return GSSD_OK;
}
