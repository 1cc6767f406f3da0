// Device-side helpers shared by the MFMA kernels of libgssd_hip.so: vector types, the LDS-DMA and barrier wrappers, the plane splits
// of the fp32-equivalent ("x6") family and the LDS layout functions that the weight packers and the kernels must agree on.
// Every helper is defined here once; a file-specific variant (another swizzle, another row order) lives in its file under its own name.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16;          // storage type of bf16 / fp16 tensors and LDS planes

// compile-time loop: f(std::integral_constant<int, I>{}) for I in [I, N), for bodies that need the index as a constant expression
template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// ---- memory ----

// LDS-DMA (global_load_lds_dwordx4): every lane fetches 16 bytes from its own `src`; the wave's 64 pieces land contiguously (1 KiB, lane
// order) at `lds_wave_base`, which is wave-uniform.  Counted by vmcnt.
__device__ __forceinline__ void dma16(const void* src, void* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// wait until at most N of this wave's vector-memory operations (LDS-DMA pieces) are outstanding and this wave's fragment reads have
// RETURNED (lgkmcnt(0): hipcc sinks their MFMAs below the barrier, so the DMA another wave issues right behind the barrier may overwrite
// that ring stage), then the workgroup barrier -- NO fence: a __syncthreads() waits vmcnt(0) and would drain the younger pieces of a ring
template <int N>
__device__ __forceinline__ void wait_vm_barrier() {
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(N) : "memory");
}

// ds_read_b64_tr_b16: the transposing LDS read that turns a row-major 16-bit tile into the k-major MFMA operand (four 16-bit elements)
__device__ __forceinline__ s16x4 tr_read(const u16* lds_ptr) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)lds_ptr);
}

__device__ __forceinline__ float bf2f(u16 h) { return __builtin_bit_cast(float, (unsigned)h << 16); }
__device__ __forceinline__ u16 f2bf(float f) { return __builtin_bit_cast(u16, (__bf16)f); }          // round to nearest even

// ---- LDS layout of 64-byte rows (32 16-bit elements = four 16-byte units); the host-side packers write the same image ----

// unit u of row `row` sits at u ^ swz64(row): conflict-free ds_read_b128 of the MFMA fragments (a four-way swizzle (row >> 2) & 3
// measured 1.5 % slower in dcn_x6)
__device__ __host__ __forceinline__ int swz64(int row) { return (row & 8) ? 3 : 0; }

// LDS row of the weight tile -> output channel inside the BN tile: the 16-row MFMA tiles j = row / 16 are paired (2 j', 2 j' + 1) so
// that the lane holding accumulator rows 4 kq .. 4 kq + 3 of both owns EIGHT consecutive channels (32-byte epilogue accesses)
__device__ __host__ __forceinline__ int chan_of_row(int row) {
    const int j = row >> 4, rho = row & 15;
    return 32 * (j >> 1) + 8 * (rho >> 2) + 4 * (j & 1) + (rho & 3);
}

// ---- plane splits of the fp32-equivalent ("x6") kernels ----
// The fp32 MFMA runs at 1/16 of the 16-bit matrix rate on gfx950, so these kernels write an fp32 operand as a short sum of 16-bit planes
// and rebuild the product from the plane products that lie above 2^-24 |x y|, accumulated in fp32.

// Three bf16 planes: x = h + m + l, each rounded to nearest even from what the planes before it left; exact to 2^-25 |x| (3 x 8
// significand bits + the signs of the residuals).  bf16 has fp32's exponent range, so the residuals need no scaling and any operand
// (activations, weights, gradients) may be split this way.
// Product: h h' + (h m' + m h') + (h l' + l h' + m m') -- six bf16 MFMAs, the rest is below 2^-24 |x y|.
__device__ __forceinline__ void split3(float v, __bf16& h, __bf16& m, __bf16& l) {
    h = (__bf16)v;
    const float r1 = v - (float)h;
    m = (__bf16)r1;
    l = (__bf16)(r1 - (float)m);
}

// the same split of TWO values at once, planes as packed bf16 pairs (a in the low half): one v_cvt_pk_bf16_f32 per plane and PAIR, and
// the packed result IS the operand dword (the element-wise form converts every element alone and then once more to pack: 7 converts per
// pair -- the compiler does not pair the converts of two chains)
__device__ __forceinline__ void split3_pair(const float a, const float b, unsigned& ph, unsigned& pm, unsigned& pl) {
    ph = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{a, b}, bf16x2));
    const float ra = a - __builtin_bit_cast(float, ph << 16), rb = b - __builtin_bit_cast(float, ph & 0xffff0000u);
    pm = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{ra, rb}, bf16x2));
    const float sa = ra - __builtin_bit_cast(float, pm << 16), sb = rb - __builtin_bit_cast(float, pm & 0xffff0000u);
    pl = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{sa, sb}, bf16x2));
}

// Two fp16 planes (round 6), for operands that are bounded activations -- launches with the fused producer BatchNorm + ReLU, or that the
// caller marks GSSD_CONV_F16_OK; data gradients keep the bf16 planes (fp16 has no exponent range for them):
//   x = h + l' / 2048,  h = fp16(x),  l' = fp16((x - h) * 2048) -- round to nearest twice, |x - h - l' / 2048| <= 2^-24 |x|: what fp32
// itself keeps -- and THREE v_mfma_f32_16x16x32_f16 per product: h h' into one accumulator, h l' + l' h' into a second one that enters
// with the factor 1 / 2048 (the l' l'' term is below 2^-24).  Half the matrix instructions and LDS fragment reads of the bf16 form, a
// split of 3 instead of 5.5 vector instructions per value.
// Why 2048: the residual is at most half an ulp of h, 2^-11 |x|; fp16 has no exponent range to spare (unscaled the residual would be a
// subnormal for |x| < 0.25), and 2^11 lifts it to the magnitude of x itself.  Valid operand range: h overflows above 65 504, which a
// BatchNorm + ReLU output does not reach; values below 6e-5 (fp16's smallest normal) lose relative, not absolute, accuracy.  Accuracy
// against float64: that of an fp32 FMA chain (4e-7 of the output scale; the three-plane bf16 form: 1.5e-7).
__device__ __forceinline__ void split2_pair(const float a, const float b, unsigned& ph, unsigned& pl) {
    const f16x2 h = __builtin_convertvector(f32x2{a, b}, f16x2);
    const f32x2 r = (f32x2{a, b} - __builtin_convertvector(h, f32x2)) * 2048.f;
    ph = __builtin_bit_cast(unsigned, h);
    pl = __builtin_bit_cast(unsigned, __builtin_convertvector(r, f16x2));
}

// Three fp16 planes (round 6), for a kernel whose accumulator count leaves no room for the second set that split2_pair's cross terms
// need: h = fp16(x), h6 = h / 64 (exact), l6 = fp16((x - h) * 64): x = h + l6 / 64 to 2^-24 |x| -- and the three products
// h h' + l6 h6' + h6 l6' into ONE accumulator.  Same plane count, LDS images and DMA pieces as the bf16 form, half the matrix instructions.
// Why 64: with one accumulator the cross terms cannot enter with a factor afterwards, so the scale cancels inside each of them,
// l6 h6' = (x - h) h'.  The residual (<= 2^-11 |x|) needs lifting, and 2^6 on it against 2^-6 on the leading plane puts half of the
// shift on either operand of the two cross terms, so that neither a residual nor a down-scaled leading plane leaves fp16's normal range
// for operands between 4e-3 and 1e3; below that the ABSOLUTE error stays under 5e-10.
__device__ __forceinline__ void split3h_pair(const float a, const float b, unsigned& ph, unsigned& p6, unsigned& pl) {
    const f16x2 h = __builtin_convertvector(f32x2{a, b}, f16x2);
    const f32x2 r = (f32x2{a, b} - __builtin_convertvector(h, f32x2)) * 64.f;
    ph = __builtin_bit_cast(unsigned, h);
    p6 = __builtin_bit_cast(unsigned, h * f16x2{(_Float16)0.015625f, (_Float16)0.015625f});
    pl = __builtin_bit_cast(unsigned, __builtin_convertvector(r, f16x2));
}
