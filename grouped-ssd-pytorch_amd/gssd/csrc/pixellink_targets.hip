// PixelLink training targets for gfx950: utils/augmentations.py:527-545 (PreparePixelLinkTargets) and
// pixel_link/pixellink_data.py:15-99 (label_to_mask_and_pixel_pos_weight) for a whole batch in one launch, with the dtypes that
// data/data_custom_v2.py:399-434 (detection_collate_v2_pixel_link) gives them.  Per image, from its float32 percent boxes:
//   corners c = trunc(fl32(b * size)) / factor (C division), box i = the rectangle between them, both ends inclusive, clipped to
//   the M x M map (M = size / factor); cnt(q) = boxes covering q; owner(q) = the box when cnt(q) == 1; P_i = pixels i owns.
//   pixel_mask = (cnt == 1), neg_pixel_mask = (cnt == 0), pixel_pos_weight = fl32(fl64(fl64(A / R) / |P_i|)) on P_i (A = sum of
//   |P_i|, R = boxes with |P_i| > 0), link_mask[j][q] = q in P_i and some p in P_i with clip(p + d_j) == q (the reference's
//   scatter, border clipping included).  The rectangle restates cv2.drawContours(thickness=-1) of the reference's axis-aligned
//   4-vertex polygon; it has not been checked against OpenCV itself (cv2 is not a dependency here).
// A workgroup builds its image's owner map in LDS (one byte per pixel: the box index, or NONE), a coverage bit per pixel, the per-box areas with LDS
// atomics and the weights, then writes its slice of rows of every output: each element once, so nothing needs a memset.
// Compiled with -ffp-contract=off; the two fp64 divisions are IEEE (correctly rounded), as numpy's.
#include "common.h"

namespace {

constexpr int MAX_M = 256;        // mask side: the owner map is MAX_M^2 bytes of LDS (size 512 with "2s")
constexpr int MAX_BOXES = 255;    // owner indices 0..254 and the sentinel fit a byte
constexpr uint8_t NONE = 255;     // cnt(q) != 1
constexpr int THREADS = 512;

// link direction j: (dh, dw), pixellink_data.py:89-96
__constant__ int8_t c_dh[8] = {1, 1, 1, 0, -1, -1, -1, 0};
__constant__ int8_t c_dw[8] = {1, 0, -1, -1, -1, 0, 1, 1};

// The p in [0, M) with clip(p + d, 0, M - 1) == q, on one axis: at most two.
__device__ __forceinline__ int preimage(int q, int d, int M, int* p) {
    int n = 0;
    const int a = q - d;
    if (a >= 0 && a < M) p[n++] = a;
    if (d != 0 && q == (d > 0 ? M - 1 : 0)) p[n++] = q;      // p + d leaves the map and is clipped back onto q
    return n;
}

// Truncated integer corner divided by the factor, as (int64)(b * size) then (label / factor).astype(int).  The clamp keeps the
// float -> integer conversion defined; it cannot change a clipped rectangle (|value| >= 2^30 lies far outside any map).
__device__ __forceinline__ int corner(float b, float size, int factor) {
    float v = __fmul_rn(b, size);
    v = fminf(fmaxf(v, -1073741824.f), 1073741824.f);
    return (int)((long long)v / factor);
}

__global__ __launch_bounds__(THREADS) void pixellink_targets_kernel(const float* __restrict__ boxes, const int32_t* __restrict__ offsets,
                                                                    int size, int factor, int M, int rows_per_wg,
                                                                    int64_t* __restrict__ pixel_mask, int64_t* __restrict__ neg_mask,
                                                                    float* __restrict__ weight, int64_t* __restrict__ link_mask) {
    __shared__ uint8_t own[MAX_M * MAX_M];
    __shared__ uint32_t cov[MAX_M * MAX_M / 32];    // bit q: cnt(q) >= 1 (one 64-pixel pair of words per wave and step)
    __shared__ int rect[MAX_BOXES][4];      // r0, r1, c0, c1 after clipping (empty: r0 > r1 or c0 > c1)
    __shared__ int area[MAX_BOXES];
    __shared__ float wgt[MAX_BOXES];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int beg = offsets[b];
    const int n = min(max(offsets[b + 1] - beg, 0), MAX_BOXES);           // the host refuses more than MAX_BOXES
    const int MM = M * M;
    for (int i = tid; i < n; i += blockDim.x) {
        const float* bx = boxes + 4 * ((long long)beg + i);
        const float s = (float)size;
        const int x0 = corner(bx[0], s, factor), y0 = corner(bx[1], s, factor);
        const int x1 = corner(bx[2], s, factor), y1 = corner(bx[3], s, factor);
        rect[i][0] = max(min(y0, y1), 0);
        rect[i][1] = min(max(y0, y1), M - 1);
        rect[i][2] = max(min(x0, x1), 0);
        rect[i][3] = min(max(x0, x1), M - 1);
        area[i] = 0;
    }
    __syncthreads();
    // owner map, coverage bits and areas over the whole image (every workgroup of the image needs all of it).  A thread's pixels lie
    // blockDim.x apart, mostly in one box: it adds a run of equal owners to the area at once (few same-address LDS atomics).
    int run_o = NONE, run_n = 0;
    for (int base = 0; base < MM; base += blockDim.x) {
        const int q = base + tid;
        int cnt = 0, o = NONE;
        if (q < MM) {
            const int h = q / M, w = q - h * M;
            for (int i = 0; i < n && cnt < 2; ++i)
                if (h >= rect[i][0] && h <= rect[i][1] && w >= rect[i][2] && w <= rect[i][3]) {
                    ++cnt;
                    o = i;
                }
            own[q] = cnt == 1 ? (uint8_t)o : NONE;
        }
        const unsigned long long bits = __ballot(cnt > 0);           // the wave's 64 pixels start at a multiple of 64
        if ((tid & 63) == 0 && q < MM) {
            cov[q >> 5] = (uint32_t)bits;
            if ((q >> 5) + 1 < (MM + 31) >> 5) cov[(q >> 5) + 1] = (uint32_t)(bits >> 32);
        }
        if (cnt == 1) {
            if (o != run_o && run_n) atomicAdd(&area[run_o], run_n), run_n = 0;
            run_o = o;
            ++run_n;
        }
    }
    if (run_n) atomicAdd(&area[run_o], run_n);
    __syncthreads();
    if (tid < 64) {
        int A = 0, R = 0;
        for (int i = tid; i < n; i += 64) {
            A += area[i];
            R += area[i] > 0;
        }
        A = wave_sum(A);
        R = wave_sum(R);
        // avg_weight_per_box = A / R (Python true division), then pixel_weight_tmp /= area: two IEEE fp64 divisions; float32 last
        for (int i = tid; i < n; i += 64)
            wgt[i] = area[i] > 0 ? (float)(((double)A / (double)R) / (double)area[i]) : 0.f;
    }
    __syncthreads();
    const int y0 = blockIdx.y * rows_per_wg, y1 = min(M, y0 + rows_per_wg);
    const long long img = (long long)b * MM;
    for (int q = y0 * M + tid; q < y1 * M; q += blockDim.x) {
        const int h = q / M, w = q - h * M;
        const int o = own[q];
        pixel_mask[img + q] = o != NONE;
        neg_mask[img + q] = ((cov[q >> 5] >> (q & 31)) & 1u) ^ 1u;
        weight[img + q] = o != NONE ? wgt[o] : 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            int hit = 0;
            if (o != NONE) {
                int ph[2], pw[2];
                const int nh = preimage(h, c_dh[j], M, ph), nw = preimage(w, c_dw[j], M, pw);
                for (int u = 0; u < nh; ++u)
                    for (int v = 0; v < nw; ++v) hit |= own[ph[u] * M + pw[v]] == o;
            }
            link_mask[(img * 8 + (long long)j * MM) + q] = hit;
        }
    }
}

}  // namespace

extern "C" int gssd_pixellink_targets(const float* boxes, const int32_t* offsets, int B, int size, int factor, int64_t* pixel_mask,
                                      int64_t* neg_pixel_mask, float* pixel_pos_weight, int64_t* link_mask, gssd_stream_t stream) {
    GSSD_CHECK_ARG(boxes && offsets && pixel_mask && neg_pixel_mask && pixel_pos_weight && link_mask);
    GSSD_CHECK_ARG(B > 0 && B <= 65535 && size > 0 && factor > 0);
    const int M = size / factor;
    GSSD_CHECK_ARG(M >= 1 && M <= MAX_M);
    // a workgroup per slice of rows: enough workgroups to spread a small batch over the CUs (each rebuilds its image's map)
    const int slices = min(M, max(1, 256 / B));
    const int rows = (M + slices - 1) / slices;
    hipLaunchKernelGGL(pixellink_targets_kernel, dim3(B, (M + rows - 1) / rows), dim3(THREADS), 0, as_stream(stream), boxes, offsets, size,
                       factor, M, rows, pixel_mask, neg_pixel_mask, pixel_pos_weight, link_mask);
    GSSD_CHECK_LAUNCH();
    return GSSD_OK;
}
