// MultiBoxLoss on gfx950: batched prior matching, hard-negative mining and the two loss sums.
// Compiled with -ffp-contract=off: the IoU / encode arithmetic must round exactly like the
// reference's separate fp32 torch ops (layers/box_utils.py:28-67,114-135) so that every integer
// output (conf_t, positive / negative masks) is bit-identical.
//
//   gssd_match_batch : one 1024-thread workgroup per image (box_utils.py:70-111)
//   gssd_hnm_loss    : one workgroup per image; mining scores live in LDS, the per-row
//                      "rank < num_neg" of the reference's double sort (multibox_loss.py:101-106) is an
//                      8-bit x 4-pass radix select of the num_neg-th largest score, ties by lower index
//   gssd_loss_finalize / gssd_loss_backward
//   gssd_multibox_loss_forward_f32 : the forward in two launches (match + conf maximum over B x 8 prior slices; mining + sums +
//                      finalize, one workgroup per image) -- the same bits as the four entry points above, which stay
#include "common.h"

namespace {

constexpr int MAX_GT = 64;
constexpr int LT = 1024;     // one workgroup per image: 16 waves hide the fp64 exp / log chains and quarter the per-thread loops

__device__ __forceinline__ float iou_pf(float ax1, float ay1, float ax2, float ay2, float area_a, float bx1, float by1,
                                        float bx2, float by2) {
    // intersect(): clamp(min(max_xy) - max(min_xy), 0) ; jaccard(): inter / (area_a + area_b - inter)
    const float w = fmaxf(fminf(ax2, bx2) - fmaxf(ax1, bx1), 0.f);
    const float h = fmaxf(fminf(ay2, by2) - fmaxf(ay1, by1), 0.f);
    const float inter = w * h;
    const float area_b = (bx2 - bx1) * (by2 - by1);
    const float uni = (area_a + area_b) - inter;
    return __fdiv_rn(inter, uni);
}

__global__ __launch_bounds__(LT) void match_kernel(const float* __restrict__ targets, const int* __restrict__ gt_off,
                                                   const float* __restrict__ priors, int P, float thr,
                                                   float var0, float var1, float* __restrict__ loc_t,
                                                   int64_t* __restrict__ conf_t) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];
    __shared__ float gt[MAX_GT][5];
    __shared__ float gt_area[MAX_GT];
    __shared__ int best_prior[MAX_GT];
    __shared__ float red_v[LT / 64];
    __shared__ int red_i[LT / 64];
    short* forced = reinterpret_cast<short*>(smraw);  // [P]: gt index forced onto this prior, -1 none

    const int b = blockIdx.x, tid = threadIdx.x;
    const int g0 = gt_off[b];
    int n = gt_off[b + 1] - g0;
    if (n > MAX_GT) n = MAX_GT;
    if (tid < 5) gt[0][tid] = 0.f;
    __syncthreads();
    for (int i = tid; i < n * 5; i += LT) gt[i / 5][i % 5] = targets[(size_t)g0 * 5 + i];
    for (int p = tid; p < P; p += LT) forced[p] = -1;
    __syncthreads();
    if (tid < n) gt_area[tid] = (gt[tid][2] - gt[tid][0]) * (gt[tid][3] - gt[tid][1]);
    __syncthreads();

    // best prior for each ground truth (overlaps.max(1)): max value, lowest index on ties
    for (int j = 0; j < n; ++j) {
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        bool any_nan = false;
        for (int p = tid; p < P; p += LT) {
            const float4 pr = reinterpret_cast<const float4*>(priors)[p];
            const float hx = pr.z / 2.f, hy = pr.w / 2.f;
            const float v = iou_pf(gt[j][0], gt[j][1], gt[j][2], gt[j][3], gt_area[j], pr.x - hx, pr.y - hy, pr.x + hx,
                                   pr.y + hy);
            if (v > bv) {
                bv = v;
                bi = p;
            }
        }
        (void)any_nan;
        // wave then block reduce on (value desc, index asc)
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (ov > bv || (ov == bv && oi < bi)) {
                bv = ov;
                bi = oi;
            }
        }
        if ((tid & 63) == 0) {
            red_v[tid >> 6] = bv;
            red_i[tid >> 6] = bi;
        }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < LT / 64; ++w)
                if (red_v[w] > bv || (red_v[w] == bv && red_i[w] < bi)) {
                    bv = red_v[w];
                    bi = red_i[w];
                }
            best_prior[j] = (bi == 0x7fffffff) ? 0 : bi;
        }
        __syncthreads();
    }
    // "for j: best_truth_idx[best_prior_idx[j]] = j" -- sequential, later ground truth wins
    if (tid == 0)
        for (int j = 0; j < n; ++j) forced[best_prior[j]] = (short)j;
    __syncthreads();

    for (int p = tid; p < P; p += LT) {
        const float4 pr = reinterpret_cast<const float4*>(priors)[p];
        const float hx = pr.z / 2.f, hy = pr.w / 2.f;
        const float px1 = pr.x - hx, py1 = pr.y - hy, px2 = pr.x + hx, py2 = pr.y + hy;
        float bv = -INFINITY;
        int bj = 0;
        for (int j = 0; j < n; ++j) {
            const float v = iou_pf(gt[j][0], gt[j][1], gt[j][2], gt[j][3], gt_area[j], px1, py1, px2, py2);
            if (v > bv) {   // overlaps.max(0): first maximum wins
                bv = v;
                bj = j;
            }
        }
        const int f = forced[p];
        if (f >= 0) {       // index_fill_(0, best_prior_idx, 2)
            bv = 2.f;
            bj = f;
        }
        int64_t conf = (int64_t)(gt[bj][4] + 1.f);
        if (bv < thr) conf = 0;
        conf_t[(size_t)b * P + p] = conf;
        // encode(): ((g_min + g_max)/2 - p_c) / (var0 * p_wh) ; log((g_max - g_min) / p_wh) / var1
        const float gx1 = gt[bj][0], gy1 = gt[bj][1], gx2 = gt[bj][2], gy2 = gt[bj][3];
        float4 o;
        o.x = __fdiv_rn(((gx1 + gx2) / 2.f) - pr.x, var0 * pr.z);
        o.y = __fdiv_rn(((gy1 + gy2) / 2.f) - pr.y, var0 * pr.w);
        o.z = __fdiv_rn((float)log((double)__fdiv_rn(gx2 - gx1, pr.z)), var1);
        o.w = __fdiv_rn((float)log((double)__fdiv_rn(gy2 - gy1, pr.w)), var1);
        reinterpret_cast<float4*>(loc_t)[(size_t)b * P + p] = o;
    }
}

// k-th largest (1-based) of n non-negative floats in LDS via 4 x 8-bit radix passes on the bit pattern.
// Returns the value's bits; *n_greater = how many are strictly greater.
__device__ unsigned radix_select_desc(const float* vals, int n, int k, unsigned* hist /*[256]*/, int* bcast /*[2]*/,
                                      int* n_greater) {
    unsigned prefix = 0, mask = 0;
    int greater = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int i = threadIdx.x; i < 256; i += blockDim.x) hist[i] = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            const unsigned u = __float_as_uint(vals[i]);
            if ((u & mask) == prefix) atomicAdd(&hist[(u >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int acc = greater, bin = 255;
            for (; bin > 0; --bin) {
                if (acc + (int)hist[bin] >= k) break;
                acc += (int)hist[bin];
            }
            bcast[0] = bin;
            bcast[1] = acc;
        }
        __syncthreads();
        prefix |= ((unsigned)bcast[0]) << shift;
        mask |= 255u << shift;
        greater = bcast[1];
        __syncthreads();
    }
    *n_greater = greater;
    return prefix;
}

__global__ __launch_bounds__(LT) void hnm_loss_kernel(const float* __restrict__ loc, const float* __restrict__ conf,
                                                      const float* __restrict__ loc_t,
                                                      const int64_t* __restrict__ conf_t,
                                                      const float* __restrict__ xmax_p, int xmax_n, int P, int C, int negpos_ratio,
                                                      uint8_t* __restrict__ sel, double* __restrict__ partial,
                                                      float* __restrict__ lca_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];
    float* lca = reinterpret_cast<float*>(smraw);  // [P]
    __shared__ unsigned hist[256];
    __shared__ int bcast[2];
    __shared__ int s_cnt[LT / 64];
    __shared__ double s_red[LT / 64][2];
    __shared__ int s_tie_base;

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float xmax = xmax_p[0];
    for (int i = 1; i < xmax_n; ++i) xmax = fmaxf(xmax, xmax_p[i]);
    const float* cb = conf + (size_t)b * P * C;
    const int64_t* tb = conf_t + (size_t)b * P;

    // loss_c = log_sum_exp(conf) - conf[target], positives zeroed (multibox_loss.py:93-98)
    int npos = 0;
    for (int p = tid; p < P; p += LT) {
        const int t = (int)tb[p];
        float s = 0.f;
        for (int c = 0; c < C; ++c) s += (float)exp((double)(cb[(size_t)p * C + c] - xmax));
        float v = ((float)log((double)s) + xmax) - cb[(size_t)p * C + t];
        if (t > 0) {
            v = 0.f;
            ++npos;
        }
        if (!(v > 0.f)) v = 0.f;   // -0 / tiny negative rounding -> +0 keeps the uint ordering monotone
        lca[p] = v;
    }
    npos = wave_sum(npos);
    if (lane == 0) s_cnt[wave] = npos;
    __syncthreads();
    npos = 0;
    for (int w = 0; w < LT / 64; ++w) npos += s_cnt[w];
    int num_neg = negpos_ratio * npos;
    if (num_neg > P - 1) num_neg = P - 1;
    if (lca_out)
        for (int p = tid; p < P; p += LT) lca_out[(size_t)b * P + p] = lca[p];

    unsigned kth_bits = 0xffffffffu;
    int n_greater = 0;
    if (num_neg > 0) kth_bits = radix_select_desc(lca, P, num_neg, hist, bcast, &n_greater);
    const int ties_needed = num_neg - n_greater;   // how many values == kth to take, lowest index first

    // neg = rank < num_neg ; stable descending order => among equal scores the lower index ranks first
    double sum_l = 0.0, sum_c = 0.0;
    if (tid == 0) s_tie_base = 0;
    __syncthreads();
    for (int p0 = 0; p0 < P; p0 += LT) {
        const int p = p0 + tid;
        bool is_tie = false, take = false, pos = false;
        if (p < P) {
            const unsigned u = __float_as_uint(lca[p]);
            pos = tb[p] > 0;
            if (num_neg > 0) {
                if (u > kth_bits) take = true;
                else if (u == kth_bits) is_tie = true;
            }
        }
        // ordered compaction of ties across the block (index order)
        const unsigned long long bal = __ballot(is_tie);
        const int before = __popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) s_cnt[wave] = __popcll(bal);
        __syncthreads();
        int base = s_tie_base;
        for (int w = 0; w < wave; ++w) base += s_cnt[w];
        if (is_tie && base + before < ties_needed) take = true;
        __syncthreads();
        if (tid == 0) {
            int t = 0;
            for (int w = 0; w < LT / 64; ++w) t += s_cnt[w];
            s_tie_base += t;
        }
        if (p < P) {
            // a positive can never be mined: its score is 0 and ranks after every positive-loss prior; if the
            // cut reaches the zeros the reference would mark it too (rank < num_neg) -- keep that behaviour
            const uint8_t code = pos ? 1 : (take ? 2 : 0);
            const bool neg_flag = take;
            sel[(size_t)b * P + p] = pos ? (uint8_t)(neg_flag ? 3 : 1) : code;
            if (pos) {
                const float4 a = reinterpret_cast<const float4*>(loc)[(size_t)b * P + p];
                const float4 t4 = reinterpret_cast<const float4*>(loc_t)[(size_t)b * P + p];
                const float d[4] = {a.x - t4.x, a.y - t4.y, a.z - t4.z, a.w - t4.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float ad = fabsf(d[e]);
                    sum_l += (double)(ad < 1.f ? 0.5f * d[e] * d[e] : ad - 0.5f);
                }
            }
            if (pos || take) {   // cross_entropy(sum) over pos | neg (multibox_loss.py:109-113)
                const int t = (int)tb[p];
                float m = cb[(size_t)p * C];
                for (int c = 1; c < C; ++c) m = fmaxf(m, cb[(size_t)p * C + c]);
                double s = 0.0;
                for (int c = 0; c < C; ++c) s += exp((double)(cb[(size_t)p * C + c] - m));
                sum_c += (log(s) + (double)m) - (double)cb[(size_t)p * C + t];
            }
        }
        __syncthreads();
    }
    sum_l = wave_sum(sum_l);
    sum_c = wave_sum(sum_c);
    if (lane == 0) {
        s_red[wave][0] = sum_l;
        s_red[wave][1] = sum_c;
    }
    __syncthreads();
    if (tid == 0) {
        double l = 0.0, c = 0.0;
        for (int w = 0; w < LT / 64; ++w) {
            l += s_red[w][0];
            c += s_red[w][1];
        }
        partial[(size_t)b * 4 + 0] = l;
        partial[(size_t)b * 4 + 1] = c;
        partial[(size_t)b * 4 + 2] = (double)npos;
        partial[(size_t)b * 4 + 3] = (double)num_neg;
    }
}

__global__ void loss_finalize_kernel(const double* __restrict__ partial, int B, float* __restrict__ losses,
                                     double* __restrict__ n_total) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double l = 0.0, c = 0.0, n = 0.0;
        for (int b = 0; b < B; ++b) {
            l += partial[b * 4 + 0];
            c += partial[b * 4 + 1];
            n += partial[b * 4 + 2];
        }
        losses[0] = (float)(l / n);   // N == 0 -> inf/nan, like the reference (multibox_loss.py:117-119)
        losses[1] = (float)(c / n);
        if (n_total) *n_total = n;
    }
}

// the normaliser of multibox_loss.py:117 taken over ALL ranks' images ("for exact equivalence to a single 256-image batch,
// all-reduce N (one int) and scale"): n_global = sum over ranks of the local N (the caller's all-reduce).  The rank's losses come out as
// world * local sum / n_global and *n_total as n_global / world, so that the data-parallel MEAN over ranks of the losses / of the gradients
// gssd_loss_backward forms with this n_total is exactly the loss / gradient of the one big batch.
__global__ void loss_finalize_global_kernel(const double* __restrict__ partial, int B, const double* __restrict__ n_global, int world,
                                            float* __restrict__ losses, double* __restrict__ n_total) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        double l = 0.0, c = 0.0;
        for (int b = 0; b < B; ++b) {
            l += partial[b * 4 + 0];
            c += partial[b * 4 + 1];
        }
        const double n = *n_global / (double)world;
        losses[0] = (float)(l / n);
        losses[1] = (float)(c / n);
        *n_total = n;
    }
}

// ------------------------------------------------------------------------------------------------------------------------------
// gssd_multibox_loss_forward_f32: the four launches above in two.  Every float and double expression, and the order of every sum, is the
// one of match_kernel / hnm_loss_kernel / loss_finalize_kernel; what changes is who computes it and how the integer searches are organised.
// ------------------------------------------------------------------------------------------------------------------------------
constexpr int MS = GSSD_MULTIBOX_SLICES;   // prior slices per image in launch 1: B x MS workgroups (256 at the driver's batch 32)
constexpr int MT = 512;
constexpr int MK = 6;                   // priors per thread and register tile in launch 1 (three tiles at P = 8732)
constexpr int MAX_CH = 36;                 // ceil(36000 / LT): the prior chunks of one thread in launch 2

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long t = __shfl_xor(k, o, 64);
        k = t > k ? t : k;
    }
    return k;
}

// (IoU, prior) -> a key whose unsigned maximum is "largest IoU, lowest prior on ties": the float's bits made monotone (-0 counts as +0,
// as in match_kernel's ov == bv) above the complemented index.  Never called for a NaN or -inf (neither passes v > bv); 0 = no candidate.
__device__ __forceinline__ unsigned long long match_key(float v, int p) {
    unsigned u = (v == 0.f) ? 0u : __float_as_uint(v);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((unsigned long long)u << 32) | (unsigned)~p;
}

// Launch 1, grid (MS, B): workgroup (s, b) writes loc_t / conf_t of priors [p0, p1) of image b and the maximum of that slice of conf.
// The best prior of a box needs all P priors: every slice workgroup of the image repeats that search (float-only, n <= 3 boxes on real
// data) instead of a second pass that patches the forced priors -- no cross-workgroup hand-over in this launch.  Each IoU is computed
// once per workgroup: the box loop feeds both the box's best prior (a wave shuffle reduction, then one LDS atomicMax per wave and box: no
// barrier per box) and, for the slice's priors, the prior's best box (kept in LDS by the thread that owns the prior).
__global__ __launch_bounds__(MT) void match_slice_kernel(const float* __restrict__ targets, const int* __restrict__ gt_off,
                                                         const float* __restrict__ priors, const float* __restrict__ conf, int P, int C,
                                                         float thr, float var0, float var1, float* __restrict__ loc_t,
                                                         int64_t* __restrict__ conf_t, float* __restrict__ pmax) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];
    __shared__ float gt[MAX_GT][5];
    __shared__ float gt_area[MAX_GT];
    __shared__ unsigned long long best_key[MAX_GT];
    __shared__ int best_prior[MAX_GT];
    __shared__ float red_m[MT / 64];

    const int s = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
    const int chunk = (P + MS - 1) / MS;
    const int p0 = min(s * chunk, P), p1 = min(p0 + chunk, P);
    float* s_bv = reinterpret_cast<float*>(smraw);          // [chunk]: best IoU of the slice's prior over the boxes so far
    int* s_bj = reinterpret_cast<int*>(s_bv + chunk);       // [chunk]: ... and its box

    const int g0 = gt_off[b];
    int n = gt_off[b + 1] - g0;
    if (n > MAX_GT) n = MAX_GT;
    if (tid < 5) gt[0][tid] = 0.f;
    if (tid < MAX_GT) best_key[tid] = 0ull;
    for (int q = p0 + tid; q < p1; q += MT) {
        s_bv[q - p0] = -INFINITY;
        s_bj[q - p0] = 0;
    }
    __syncthreads();
    for (int i = tid; i < n * 5; i += MT) gt[i / 5][i % 5] = targets[(size_t)g0 * 5 + i];
    __syncthreads();
    if (tid < n) gt_area[tid] = (gt[tid][2] - gt[tid][0]) * (gt[tid][3] - gt[tid][1]);
    __syncthreads();

    // thread tid owns priors tid, tid + MT, ... in both roles, so s_bv / s_bj need no barrier.  A tile of MK priors per thread stays in
    // registers in corner form while the boxes go by: one prior load per prior, not one per (prior, box).
    for (int base = 0; base < P; base += MT * MK) {
        float px1[MK], py1[MK], px2[MK], py2[MK];
#pragma unroll
        for (int k = 0; k < MK; ++k) {
            const int p = base + k * MT + tid;
            const float4 pr = p < P ? reinterpret_cast<const float4*>(priors)[p] : make_float4(0.f, 0.f, 0.f, 0.f);
            const float hx = pr.z / 2.f, hy = pr.w / 2.f;
            px1[k] = pr.x - hx;
            py1[k] = pr.y - hy;
            px2[k] = pr.x + hx;
            py2[k] = pr.y + hy;
        }
        for (int j = 0; j < n; ++j) {
            const float gx1 = gt[j][0], gy1 = gt[j][1], gx2 = gt[j][2], gy2 = gt[j][3], ga = gt_area[j];
            float bv = -INFINITY;
            int bi = 0x7fffffff;
#pragma unroll
            for (int k = 0; k < MK; ++k) {
                const int p = base + k * MT + tid;
                if (p < P) {
                    const float v = iou_pf(gx1, gy1, gx2, gy2, ga, px1[k], py1[k], px2[k], py2[k]);
                    if (v > bv) {       // overlaps.max(1): lowest index of the maximum (p ascends); a NaN never wins
                        bv = v;
                        bi = p;
                    }
                    if (p >= p0 && p < p1 && v > s_bv[p - p0]) {   // overlaps.max(0): first maximum wins (j ascends)
                        s_bv[p - p0] = v;
                        s_bj[p - p0] = j;
                    }
                }
            }
            unsigned long long key = (bi == 0x7fffffff) ? 0ull : match_key(bv, bi);
            key = wave_max_u64(key);
            if (lane == 0 && key) atomicMax(&best_key[j], key);
        }
    }
    __syncthreads();
    if (tid < n) best_prior[tid] = best_key[tid] ? (int)~(unsigned)best_key[tid] : 0;
    __syncthreads();

    for (int p = p0 + tid; p < p1; p += MT) {
        const float4 pr = reinterpret_cast<const float4*>(priors)[p];
        float bv = s_bv[p - p0];
        int bj = s_bj[p - p0];
        // "for j: best_truth_idx[best_prior_idx[j]] = j" -- sequential, later ground truth wins
        int f = -1;
        for (int j = 0; j < n; ++j)
            if (best_prior[j] == p) f = j;
        if (f >= 0) {       // index_fill_(0, best_prior_idx, 2)
            bv = 2.f;
            bj = f;
        }
        int64_t cf = (int64_t)(gt[bj][4] + 1.f);
        if (bv < thr) cf = 0;
        conf_t[(size_t)b * P + p] = cf;
        // encode(): ((g_min + g_max)/2 - p_c) / (var0 * p_wh) ; log((g_max - g_min) / p_wh) / var1
        const float gx1 = gt[bj][0], gy1 = gt[bj][1], gx2 = gt[bj][2], gy2 = gt[bj][3];
        float4 o;
        o.x = __fdiv_rn(((gx1 + gx2) / 2.f) - pr.x, var0 * pr.z);
        o.y = __fdiv_rn(((gy1 + gy2) / 2.f) - pr.y, var0 * pr.w);
        o.z = __fdiv_rn((float)log((double)__fdiv_rn(gx2 - gx1, pr.z)), var1);
        o.w = __fdiv_rn((float)log((double)__fdiv_rn(gy2 - gy1, pr.w)), var1);
        reinterpret_cast<float4*>(loc_t)[(size_t)b * P + p] = o;
    }

    // log_sum_exp's x_max: this slice's share (a maximum of maxima is the same float whatever the partition)
    const float* cs = conf + ((size_t)b * P + p0) * C;
    const int len = (p1 - p0) * C;
    int head = (int)(((16u - (unsigned)((uintptr_t)cs & 15u)) & 15u) >> 2);
    if (head > len) head = len;
    float m = -INFINITY;
    if (tid < head) m = cs[tid];
    const int n4 = (len - head) >> 2;
    for (int i = tid; i < n4; i += MT) {
        const float4 v = reinterpret_cast<const float4*>(cs + head)[i];
        m = fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w));
    }
    for (int i = head + (n4 << 2) + tid; i < len; i += MT) m = fmaxf(m, cs[i]);
    m = wave_max(m);
    if (lane == 0) red_m[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < MT / 64; ++w) m = fmaxf(m, red_m[w]);
        pmax[b * MS + s] = m;
    }
}

// k-th largest (1-based) of n non-negative floats in LDS, as radix_select_desc, without its serial parts: the digits of a wave are
// counted by ballots (one LDS add per distinct digit and wave, however the scores cluster), every wave finds the bin itself by a suffix
// scan (256 bins, four per lane: no thread-0 walk, no broadcast), and each pass has a histogram of its own, so one barrier per pass.
// hist [4][256] is zero on entry (a barrier behind the zeroing included).
__device__ unsigned radix_select_desc_scan(const float* vals, int n, int k, unsigned (*hist)[256], int* n_greater) {
    const int tid = threadIdx.x, lane = tid & 63;
    unsigned prefix = 0, mask = 0;
    int greater = 0;
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        unsigned* h = hist[pass];
        for (int base = 0; base < n; base += LT) {
            const int i = base + tid;
            bool act = false;
            unsigned d = 0;
            if (i < n) {
                const unsigned u = __float_as_uint(vals[i]);
                act = (u & mask) == prefix;
                d = (u >> shift) & 255u;
            }
            unsigned long long peers = __ballot(act);
            if (peers == 0ull) continue;
#pragma unroll
            for (int bit = 0; bit < 8; ++bit) {
                const bool on = (d >> bit) & 1u;
                const unsigned long long bb = __ballot(act && on);
                peers &= on ? bb : ~bb;
            }
            if (act && lane == __ffsll((long long)peers) - 1) atomicAdd(&h[d], (unsigned)__popcll(peers));
        }
        __syncthreads();
        // lane l holds bins 4l .. 4l+3; `above` = values ranked before bin 4l+3 (those of higher bins and of the earlier passes)
        const uint4 c = reinterpret_cast<const uint4*>(h)[lane];
        const int sum4 = (int)(c.x + c.y + c.z + c.w);
        int incl = sum4;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_down(incl, o, 64);
            if (lane + o < 64) incl += t;
        }
        const int above = greater + incl - sum4;
        const int cum3 = above + (int)c.w, cum2 = cum3 + (int)c.z, cum1 = cum2 + (int)c.y, cum0 = cum1 + (int)c.x;
        // the walk "from bin 255 down, stop at the first bin whose cumulative count reaches k, or at bin 0": the cumulative count only
        // grows downwards, so the bins that reach k are 0 .. bin
        const int reach = wave_sum((int)(cum3 >= k) + (int)(cum2 >= k) + (int)(cum1 >= k) + (int)(cum0 >= k));
        const int bin = reach > 0 ? reach - 1 : 0;
        const int r = bin & 3;
        const int before = r == 3 ? above : (r == 2 ? cum3 : (r == 1 ? cum2 : cum1));
        greater = __shfl(before, bin >> 2, 64);
        prefix |= ((unsigned)bin) << shift;
        mask |= 255u << shift;
    }
    *n_greater = greater;
    return prefix;
}

// Launch 2, grid B: hnm_loss_kernel with the x_max reduction in front and the finalize behind.  The sums keep their association: thread
// tid adds priors tid, tid + 1024, ... in fp64, then wave_sum, then the 16 waves in order, then the images in order.
__global__ __launch_bounds__(LT) void hnm_fused_kernel(const float* __restrict__ loc, const float* __restrict__ conf,
                                                       const float* __restrict__ loc_t, const int64_t* __restrict__ conf_t,
                                                       const float* __restrict__ pmax, int pmax_n, int P, int C, int negpos_ratio,
                                                       uint8_t* __restrict__ sel, double* partial, float* __restrict__ lca_out,
                                                       unsigned* ticket, int B, float* __restrict__ losses,
                                                       double* __restrict__ n_total) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];
    float* lca = reinterpret_cast<float*>(smraw);  // [P]
    __shared__ __attribute__((aligned(16))) unsigned hist[4][256];
    __shared__ int s_cnt[LT / 64];
    __shared__ float s_max[LT / 64];
    __shared__ double s_red[LT / 64][2];
    __shared__ int s_tie[MAX_CH * (LT / 64)];
    __shared__ int s_last;

    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float xmax = -INFINITY;
    for (int i = tid; i < pmax_n; i += LT) xmax = fmaxf(xmax, pmax[i]);
    xmax = wave_max(xmax);
    if (lane == 0) s_max[wave] = xmax;
    reinterpret_cast<unsigned*>(hist)[tid] = 0u;   // LT == 4 * 256
    __syncthreads();
    xmax = s_max[0];
    for (int w = 1; w < LT / 64; ++w) xmax = fmaxf(xmax, s_max[w]);
    const float* cb = conf + (size_t)b * P * C;
    const int64_t* tb = conf_t + (size_t)b * P;

    // loss_c = log_sum_exp(conf) - conf[target], positives zeroed (multibox_loss.py:93-98)
    // (the target and the first four logits of the NEXT prior are fetched before this prior's exp / log chain: the loads of the up to
    // 36 trips are independent, the chain is not short)
    int npos = 0;
    int t_n = 0;
    float c_n[4] = {0.f, 0.f, 0.f, 0.f};
    auto fetch = [&](int q) {
        if (q < P) {
            t_n = (int)tb[q];
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (c < C) c_n[c] = cb[(size_t)q * C + c];
        }
    };
    fetch(tid);
    for (int p = tid; p < P; p += LT) {
        const int t = t_n;
        const float cv[4] = {c_n[0], c_n[1], c_n[2], c_n[3]};
        fetch(p + LT);
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (c < C) s += (float)exp((double)(cv[c] - xmax));
        for (int c = 4; c < C; ++c) s += (float)exp((double)(cb[(size_t)p * C + c] - xmax));
        const float xt = t == 0 ? cv[0] : (t == 1 ? cv[1] : (t == 2 ? cv[2] : (t == 3 ? cv[3] : cb[(size_t)p * C + t])));
        float v = ((float)log((double)s) + xmax) - xt;
        if (t > 0) {
            v = 0.f;
            ++npos;
        }
        if (!(v > 0.f)) v = 0.f;   // -0 / tiny negative rounding -> +0 keeps the uint ordering monotone
        lca[p] = v;
    }
    npos = wave_sum(npos);
    if (lane == 0) s_cnt[wave] = npos;
    __syncthreads();
    npos = 0;
    for (int w = 0; w < LT / 64; ++w) npos += s_cnt[w];
    int num_neg = negpos_ratio * npos;
    if (num_neg > P - 1) num_neg = P - 1;
    if (lca_out)
        for (int p = tid; p < P; p += LT) lca_out[(size_t)b * P + p] = lca[p];

    unsigned kth_bits = 0xffffffffu;
    int n_greater = 0;
    const int nch = (P + LT - 1) / LT;
    if (num_neg > 0) {   // (uniform over the workgroup)
        kth_bits = radix_select_desc_scan(lca, P, num_neg, hist, &n_greater);
        // ties at the cut are taken lowest index first: one exclusive scan over the (chunk, wave) tie counts, which are in index order
        for (int k = 0; k < nch; ++k) {
            const int p = k * LT + tid;
            const unsigned long long bal = __ballot(p < P && __float_as_uint(lca[p < P ? p : 0]) == kth_bits);
            if (lane == 0) s_tie[k * (LT / 64) + wave] = __popcll(bal);
        }
        __syncthreads();
        if (wave == 0) {
            const int ntot = nch * (LT / 64), per = (ntot + 63) / 64;
            int sum = 0;
            for (int e = 0; e < per; ++e) {
                const int idx = lane * per + e;
                if (idx < ntot) sum += s_tie[idx];
            }
            int incl = sum;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int t = __shfl_up(incl, o, 64);
                if (lane >= o) incl += t;
            }
            int run = incl - sum;
            for (int e = 0; e < per; ++e) {
                const int idx = lane * per + e;
                if (idx < ntot) {
                    const int v = s_tie[idx];
                    s_tie[idx] = run;
                    run += v;
                }
            }
        }
        __syncthreads();
    }
    const int ties_needed = num_neg - n_greater;   // how many values == kth to take, lowest index first

    // neg = rank < num_neg ; stable descending order => among equal scores the lower index ranks first
    double sum_l = 0.0, sum_c = 0.0;
    for (int k = 0; k < nch; ++k) {
        const int p = k * LT + tid;
        bool is_tie = false, take = false, pos = false;
        if (p < P) {
            const unsigned u = __float_as_uint(lca[p]);
            pos = tb[p] > 0;
            if (num_neg > 0) {
                if (u > kth_bits) take = true;
                else if (u == kth_bits) is_tie = true;
            }
        }
        const unsigned long long bal = __ballot(is_tie);
        if (is_tie && s_tie[k * (LT / 64) + wave] + __popcll(bal & ((1ull << lane) - 1ull)) < ties_needed) take = true;
        if (p < P) {
            // a positive can never be mined: its score is 0 and ranks after every positive-loss prior; if the
            // cut reaches the zeros the reference would mark it too (rank < num_neg) -- keep that behaviour
            const uint8_t code = pos ? 1 : (take ? 2 : 0);
            const bool neg_flag = take;
            sel[(size_t)b * P + p] = pos ? (uint8_t)(neg_flag ? 3 : 1) : code;
            if (pos) {
                const float4 a = reinterpret_cast<const float4*>(loc)[(size_t)b * P + p];
                const float4 t4 = reinterpret_cast<const float4*>(loc_t)[(size_t)b * P + p];
                const float d[4] = {a.x - t4.x, a.y - t4.y, a.z - t4.z, a.w - t4.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float ad = fabsf(d[e]);
                    sum_l += (double)(ad < 1.f ? 0.5f * d[e] * d[e] : ad - 0.5f);
                }
            }
            if (pos || take) {   // cross_entropy(sum) over pos | neg (multibox_loss.py:109-113)
                const int t = (int)tb[p];
                float m = cb[(size_t)p * C];
                for (int c = 1; c < C; ++c) m = fmaxf(m, cb[(size_t)p * C + c]);
                double s = 0.0;
                for (int c = 0; c < C; ++c) s += exp((double)(cb[(size_t)p * C + c] - m));
                sum_c += (log(s) + (double)m) - (double)cb[(size_t)p * C + t];
            }
        }
    }
    sum_l = wave_sum(sum_l);
    sum_c = wave_sum(sum_c);
    if (lane == 0) {
        s_red[wave][0] = sum_l;
        s_red[wave][1] = sum_c;
    }
    __syncthreads();
    // The rows of `partial` are handed to the workgroup that finishes last: 8-byte agent-scope atomic stores (write-through), drained,
    // then ONE agent-scope add by the same lane; the workgroup whose add returned B - 1 reads them with agent-scope atomic loads (past
    // this CU's L1), after the barrier its adding wave joins.  No plain access to another workgroup's stores on either side.
    unsigned long long* part = reinterpret_cast<unsigned long long*>(partial);
    if (tid == 0) {
        double l = 0.0, c = 0.0;
        for (int w = 0; w < LT / 64; ++w) {
            l += s_red[w][0];
            c += s_red[w][1];
        }
        __hip_atomic_store(part + (size_t)b * 4 + 0, (unsigned long long)__double_as_longlong(l), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(part + (size_t)b * 4 + 1, (unsigned long long)__double_as_longlong(c), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(part + (size_t)b * 4 + 2, (unsigned long long)__double_as_longlong((double)npos), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(part + (size_t)b * 4 + 3, (unsigned long long)__double_as_longlong((double)num_neg), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_last = (t == (unsigned)(B - 1)) ? 1 : 0;
    }
    __syncthreads();
    if (s_last && wave == 0) {
        double l = 0.0, c = 0.0, n = 0.0;
        for (int base = 0; base < B; base += 64) {
            const int bb = base + lane < B ? base + lane : B - 1;
            const double vl = __longlong_as_double((long long)__hip_atomic_load(part + (size_t)bb * 4 + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            const double vc = __longlong_as_double((long long)__hip_atomic_load(part + (size_t)bb * 4 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            const double vn = __longlong_as_double((long long)__hip_atomic_load(part + (size_t)bb * 4 + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
            const int cnt = B - base < 64 ? B - base : 64;
            for (int i = 0; i < cnt; ++i) {   // image order, as loss_finalize_kernel
                l += __shfl(vl, i, 64);
                c += __shfl(vc, i, 64);
                n += __shfl(vn, i, 64);
            }
        }
        if (lane == 0) {
            losses[0] = (float)(l / n);   // N == 0 -> inf/nan, like the reference (multibox_loss.py:117-119)
            losses[1] = (float)(c / n);
            if (n_total) *n_total = n;
            __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // zero again for the next call
        }
    }
}

__global__ void loss_backward_kernel(const float* __restrict__ loc, const float* __restrict__ conf,
                                     const float* __restrict__ loc_t, const int64_t* __restrict__ conf_t,
                                     const uint8_t* __restrict__ sel, const double* __restrict__ n_total,
                                     const float* __restrict__ gl_p, const float* __restrict__ gc_p, long long BP, int C,
                                     float* __restrict__ dloc, float* __restrict__ dconf) {
    const float invN = (float)(1.0 / *n_total);
    const float gl = (gl_p ? *gl_p : 1.f) * invN, gc = (gc_p ? *gc_p : 1.f) * invN;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < BP;
         i += (long long)gridDim.x * blockDim.x) {
        const uint8_t s = sel[i];
        float4 g = {0.f, 0.f, 0.f, 0.f};
        if (s & 1) {
            const float4 a = reinterpret_cast<const float4*>(loc)[i];
            const float4 t = reinterpret_cast<const float4*>(loc_t)[i];
            const float d[4] = {a.x - t.x, a.y - t.y, a.z - t.z, a.w - t.w};
            float o[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (fabsf(d[e]) < 1.f ? d[e] : (d[e] > 0.f ? 1.f : -1.f)) * gl;
            g = {o[0], o[1], o[2], o[3]};
        }
        reinterpret_cast<float4*>(dloc)[i] = g;
        if (s) {
            const int t = (int)conf_t[i];
            float m = conf[i * C];
            for (int c = 1; c < C; ++c) m = fmaxf(m, conf[i * C + c]);
            float z = 0.f;
            for (int c = 0; c < C; ++c) z += __expf(conf[i * C + c] - m);
            for (int c = 0; c < C; ++c) dconf[i * C + c] = (__expf(conf[i * C + c] - m) / z - (c == t ? 1.f : 0.f)) * gc;
        } else {
            for (int c = 0; c < C; ++c) dconf[i * C + c] = 0.f;
        }
    }
}

}  // namespace

extern "C" int gssd_match_batch(const float* targets, const int* gt_off, const float* priors, int B, int P,
                                float threshold, float var0, float var1, float* loc_t, int64_t* conf_t,
                                gssd_stream_t stream) {
    GSSD_CHECK_ARG(targets && gt_off && priors && loc_t && conf_t);
    GSSD_CHECK_ARG(B > 0 && P > 0 && P < 32768);
    GSSD_CHECK_ARG(((uintptr_t)priors % 16) == 0 && ((uintptr_t)loc_t % 16) == 0);
    hipLaunchKernelGGL(match_kernel, dim3(B), dim3(LT), (size_t)P * sizeof(short), as_stream(stream), targets, gt_off,
                       priors, P, threshold, var0, var1, loc_t, conf_t);
    GSSD_CHECK_LAUNCH();
    return GSSD_OK;
}

extern "C" int gssd_hnm_loss(const float* loc, const float* conf, const float* loc_t, const int64_t* conf_t,
                             const float* xmax, int xmax_n, int B, int P, int C, int negpos_ratio, uint8_t* sel,
                             double* partial, float* loss_c_all, gssd_stream_t stream) {
    GSSD_CHECK_ARG(loc && conf && loc_t && conf_t && xmax && xmax_n > 0 && sel && partial);
    GSSD_CHECK_ARG(B > 0 && P > 0 && P <= 36000 && C >= 2 && negpos_ratio >= 0);
    GSSD_CHECK_ARG(((uintptr_t)loc % 16) == 0 && ((uintptr_t)loc_t % 16) == 0);
    static unsigned attr_mask = 0;     // one bit per device (the attribute is per device)
    const size_t smem = (size_t)P * sizeof(float);
    if (smem > 48 * 1024)
        if (const int rc = gssd_max_dynamic_lds(&attr_mask, hnm_loss_kernel, 150 * 1024)) return rc;
    hipLaunchKernelGGL(hnm_loss_kernel, dim3(B), dim3(LT), smem, as_stream(stream), loc, conf, loc_t, conf_t, xmax, xmax_n, P,
                       C, negpos_ratio, sel, partial, loss_c_all);
    GSSD_CHECK_LAUNCH();
    return GSSD_OK;
}

extern "C" int gssd_loss_finalize(const double* partial, int B, float* losses, double* n_total, gssd_stream_t stream) {
    GSSD_CHECK_ARG(partial && losses && B > 0);
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(64), 0, as_stream(stream), partial, B, losses, n_total);
    GSSD_CHECK_LAUNCH();
    return GSSD_OK;
}

// workspace: [0, 16) the ticket of launch 2 (zero between calls), then B * MS partial maxima of conf
extern "C" long long gssd_multibox_loss_workspace_bytes(int B) { return B > 0 ? 16 + (long long)B * MS * (long long)sizeof(float) : 0; }

extern "C" int gssd_multibox_loss_forward_f32(const float* loc, const float* conf, const float* priors, const float* targets,
                                              const int* gt_off, int B, int P, int C, float threshold, float var0, float var1,
                                              int negpos_ratio, float* loc_t, int64_t* conf_t, uint8_t* sel, double* partial,
                                              float* losses, double* n_total, float* loss_c_all, void* workspace,
                                              long long workspace_bytes, gssd_stream_t stream) {
    GSSD_CHECK_ARG(loc && conf && priors && targets && gt_off && loc_t && conf_t && sel && partial && losses && workspace);
    GSSD_CHECK_ARG(B > 0 && B <= 65535 && P > 0 && P < 32768 && C >= 2 && negpos_ratio >= 0);
    GSSD_CHECK_ARG(workspace_bytes >= gssd_multibox_loss_workspace_bytes(B));
    GSSD_CHECK_ARG(((uintptr_t)priors % 16) == 0 && ((uintptr_t)loc % 16) == 0 && ((uintptr_t)loc_t % 16) == 0);
    GSSD_CHECK_ARG(((uintptr_t)workspace % 16) == 0 && ((uintptr_t)partial % 8) == 0 && ((uintptr_t)conf % 4) == 0);
    unsigned* ticket = static_cast<unsigned*>(workspace);
    float* pmax = reinterpret_cast<float*>(static_cast<unsigned char*>(workspace) + 16);
    const int chunk = (P + MS - 1) / MS;
    hipLaunchKernelGGL(match_slice_kernel, dim3(MS, B), dim3(MT), (size_t)chunk * (sizeof(float) + sizeof(int)), as_stream(stream),
                       targets, gt_off, priors, conf, P, C, threshold, var0, var1, loc_t, conf_t, pmax);
    GSSD_CHECK_LAUNCH();
    static unsigned attr_mask = 0;     // one bit per device (the attribute is per device)
    const size_t smem = (size_t)P * sizeof(float);
    if (smem > 48 * 1024)
        if (const int rc = gssd_max_dynamic_lds(&attr_mask, hnm_fused_kernel, 150 * 1024)) return rc;
    hipLaunchKernelGGL(hnm_fused_kernel, dim3(B), dim3(LT), smem, as_stream(stream), loc, conf, loc_t, conf_t, pmax, B * MS, P, C,
                       negpos_ratio, sel, partial, loss_c_all, ticket, B, losses, n_total);
    GSSD_CHECK_LAUNCH();
    return GSSD_OK;
}

extern "C" int gssd_loss_finalize_global(const double* partial, int B, const double* n_global, int world, float* losses, double* n_total,
                                         gssd_stream_t stream) {
    GSSD_CHECK_ARG(partial && losses && n_global && n_total && B > 0 && world > 0);
    hipLaunchKernelGGL(loss_finalize_global_kernel, dim3(1), dim3(64), 0, as_stream(stream), partial, B, n_global, world, losses, n_total);
    GSSD_CHECK_LAUNCH();
    return GSSD_OK;
}

extern "C" int gssd_loss_backward(const float* loc, const float* conf, const float* loc_t, const int64_t* conf_t,
                                  const uint8_t* sel, const double* n_total, const float* grad_l, const float* grad_c,
                                  int B, int P, int C, float* dloc, float* dconf, gssd_stream_t stream) {
    GSSD_CHECK_ARG(loc && conf && loc_t && conf_t && sel && n_total && dloc && dconf && B > 0 && P > 0 && C >= 2);
    const long long BP = (long long)B * P;
    int blocks = (int)((BP + 255) / 256);
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(loss_backward_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), loc, conf, loc_t, conf_t, sel,
                       n_total, grad_l, grad_c, BP, C, dloc, dconf);
    GSSD_CHECK_LAUNCH();
    return GSSD_OK;
}
