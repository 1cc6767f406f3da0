// Pillow's 8-bit resampling arithmetic (src/libImaging/Resample.c, 8bpc path), shared by the input stage (input_stage.hip) and
// the training augmentation (augment.hip): the coefficients are 22-bit fixed point (gssd_resample_coeffs), the accumulator starts
// at 1 << 21, the sum is shifted arithmetically and clipped to [0, 255].
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gssd_resample8 {

constexpr int PRECISION_BITS = 32 - 8 - 2;

__device__ __forceinline__ uint8_t clip8(int acc) {
    const int v = acc >> PRECISION_BITS;                    // arithmetic shift, like the C reference
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// One output byte: n taps of bytes `stride` apart starting at p, coefficients k[0 .. n).
__device__ __forceinline__ uint8_t taps8(const uint8_t* p, int stride, const int* k, int n) {
    int acc = 1 << (PRECISION_BITS - 1);
    for (int t = 0; t < n; ++t) acc += __mul24((int)p[t * stride], k[t]);      // 8-bit x 23-bit: exact in the 24-bit multiplier
    return clip8(acc);
}

}  // namespace gssd_resample8
