// Per-tensor statistics of the gradients (and weights) of a model -- what the reference drivers' check_grad_norm(net) reads back one
// tensor at a time (train_lesion_multiphase_v2.py:250), and what tells WHICH tensor went non-finite -- on the item / chunk tables of
// optim.hip, in two launches, without atomics and without a host read:
//
//   tensor_stats_chunk_kernel   one workgroup per chunk: sum of squares (fp64), largest finite |x| and the count of non-finite elements
//                               of the chunk of g and of p, left as one 32-byte record per chunk;
//   tensor_stats_fold_kernel    workgroup i folds the records of item i into row i of the fp64 table, one more workgroup folds ALL
//                               records into the totals row.  It runs stream-ordered behind the first: no grid-wide wait.
//
// Squares are formed in fp64 from the converted element: every fp32 square is exact there, a subnormal gradient and one of 1e30
// contribute alike (in fp32 the first square is 0 and the second inf).  Sums are IEEE: an inf makes them inf, a NaN makes them NaN; the
// maximum and the count are what say how much of the tensor is still finite.  Every reduction runs in a fixed order, so a table is the
// same to the bit from run to run.  The totals row is folded from the chunk records, not from the rows: the fold kernel then needs no
// second pass (or a third launch) behind its own rows, and the total does not inherit the rows' rounding.
#include "optim_util.h"

namespace {

struct StatsRec {                       // 32 bytes per chunk
    double sumsq_g, sumsq_p;
    float amax_g, amax_p;
    uint32_t nf_g, nf_p;
};
static_assert(sizeof(StatsRec) == 32, "gssd_tensor_stats_workspace_bytes");

constexpr int OUT_COLS = 8;             // g: sumsq, norm, absmax, nonfinite; then the same of p
constexpr uint32_t ABS_MASK = 0x7fffffffu, EXP_MASK = 0x7f800000u;

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t w = (uint32_t)__shfl_xor((int)v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}

// block_sum's shape for the two other reductions: xor butterfly inside the waves, then the four waves in order
__device__ __forceinline__ uint32_t block_max_u32(uint32_t v, uint32_t* red) {
    v = wave_max_u32(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const uint32_t a = red[0] > red[1] ? red[0] : red[1], b = red[2] > red[3] ? red[2] : red[3];
    return a > b ? a : b;
}
__device__ __forceinline__ uint32_t block_sum_u32(uint32_t v, uint32_t* red) {
    v = (uint32_t)wave_sum((int)v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

struct Acc {
    double ss = 0.0;
    uint32_t amax = 0;                  // bits of the largest finite |x|: for non-negative floats the order of the bits is the order of
    uint32_t nf = 0;                    // the values, subnormals included, and no NaN ever enters a floating-point max
};

__device__ __forceinline__ void take(Acc& a, const float (&x)[NE + 1]) {
#pragma unroll
    for (int k = 0; k <= NE; ++k) {
        const double d = (double)x[k];
        a.ss += d * d;
        const uint32_t mag = __builtin_bit_cast(uint32_t, x[k]) & ABS_MASK;
        if (mag < EXP_MASK)
            a.amax = mag > a.amax ? mag : a.amax;
        else
            ++a.nf;
    }
}

__global__ __launch_bounds__(THREADS) void tensor_stats_chunk_kernel(const gssd_sgd_item* items, const gssd_sgd_chunk* chunks,
                                                                     StatsRec* recs) {
    __shared__ double red_d[2][4];
    __shared__ uint32_t red_u[4][4];
    const gssd_sgd_chunk ch = chunks[blockIdx.x];
    const gssd_sgd_item it = items[ch.item];
    const int len = chunk_len(it, ch);
    const gfloat* g = it.g ? as_global(it.g) + ch.off : nullptr;
    const gfloat* p = it.p ? as_global(it.p) + ch.off : nullptr;
    float gx[NE + 1], px[NE + 1];
    load_share(g, len, gx);             // all loads of the thread issue here ...
    load_share(p, len, px);
    Acc ag, ap;
    take(ag, gx);                       // ... before the first use
    take(ap, px);
    StatsRec r;
    r.sumsq_g = block_sum(ag.ss, red_d[0]);
    r.sumsq_p = block_sum(ap.ss, red_d[1]);
    r.amax_g = __builtin_bit_cast(float, block_max_u32(ag.amax, red_u[0]));
    r.amax_p = __builtin_bit_cast(float, block_max_u32(ap.amax, red_u[1]));
    r.nf_g = block_sum_u32(ag.nf, red_u[2]);
    r.nf_p = block_sum_u32(ap.nf, red_u[3]);
    if (threadIdx.x == 0) recs[blockIdx.x] = r;
}

__global__ __launch_bounds__(THREADS) void tensor_stats_fold_kernel(const StatsRec* recs, const int* item_chunk0, const int n_items,
                                                                    const int n_chunks, double* out) {
    __shared__ double red_d[4][4];
    __shared__ uint32_t red_u[2][4];
    const int row = blockIdx.x;
    int c0 = row < n_items ? item_chunk0[row] : 0;
    int c1 = row < n_items ? item_chunk0[row + 1] : n_chunks;
    c0 = c0 < 0 ? 0 : c0, c1 = c1 > n_chunks ? n_chunks : c1;      // (a bad prefix reads no record that is not there)
    double ss_g = 0.0, ss_p = 0.0, nf_g = 0.0, nf_p = 0.0;        // (counts of up to 4096 per record: their fp64 sums are exact)
    uint32_t am_g = 0, am_p = 0;
    for (int c = c0 + (int)threadIdx.x; c < c1; c += THREADS) {
        const StatsRec r = recs[c];
        ss_g += r.sumsq_g, ss_p += r.sumsq_p;
        nf_g += (double)r.nf_g, nf_p += (double)r.nf_p;
        const uint32_t mg = __builtin_bit_cast(uint32_t, r.amax_g), mp = __builtin_bit_cast(uint32_t, r.amax_p);
        am_g = mg > am_g ? mg : am_g, am_p = mp > am_p ? mp : am_p;
    }
    ss_g = block_sum(ss_g, red_d[0]);
    ss_p = block_sum(ss_p, red_d[1]);
    nf_g = block_sum(nf_g, red_d[2]);
    nf_p = block_sum(nf_p, red_d[3]);
    am_g = block_max_u32(am_g, red_u[0]);
    am_p = block_max_u32(am_p, red_u[1]);
    if (threadIdx.x == 0) {
        double* o = out + (size_t)row * OUT_COLS;
        o[0] = ss_g, o[1] = sqrt(ss_g), o[2] = (double)__builtin_bit_cast(float, am_g), o[3] = nf_g;
        o[4] = ss_p, o[5] = sqrt(ss_p), o[6] = (double)__builtin_bit_cast(float, am_p), o[7] = nf_p;
    }
}

}  // namespace

extern "C" long long gssd_tensor_stats_workspace_bytes(int n_chunks) { return n_chunks > 0 ? (long long)sizeof(StatsRec) * n_chunks : 0; }

extern "C" int gssd_tensor_stats_f32(const gssd_sgd_item* items, int n_items, const gssd_sgd_chunk* chunks, int n_chunks,
                                     const int* item_chunk0, void* workspace, double* out, gssd_stream_t stream) {
    GSSD_CHECK_ARG(items && n_items > 0 && n_chunks >= 0 && item_chunk0 && out);
    GSSD_CHECK_ARG(n_chunks == 0 || (chunks && workspace));
    GSSD_CHECK_ARG(((uintptr_t)workspace & 7) == 0);
    if (n_chunks > 0) {
        hipLaunchKernelGGL(tensor_stats_chunk_kernel, dim3(n_chunks), dim3(THREADS), 0, as_stream(stream), items, chunks,
                           (StatsRec*)workspace);
        GSSD_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(tensor_stats_fold_kernel, dim3(n_items + 1), dim3(THREADS), 0, as_stream(stream), (const StatsRec*)workspace,
                       item_chunk0, n_items, n_chunks, out);
    GSSD_CHECK_LAUNCH();
    return GSSD_OK;
}
