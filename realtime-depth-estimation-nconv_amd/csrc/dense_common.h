// dense_common.h — what the dense-convolution translation units share (dense_conv.hip: forward,
// dense_pack.hip: weight packing, dense_wgrad.hip: weight gradients).
#pragma once
#include "nconv_internal.h"

namespace nconv {

constexpr int kDT = 256;
constexpr int kCK = 8;  // input channels per staged chunk

__host__ __device__ constexpr int dense_taps(int kind) {
    return kind == NCONV_DENSE_3X3 ? 9 : kind == NCONV_DENSE_1X1 ? 1 : kind == NCONV_DENSE_TRANSPOSED_4X4 ? 4 : 16;
}

typedef float f16v __attribute__((ext_vector_type(16)));
typedef __bf16 dbf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned du4 __attribute__((ext_vector_type(4)));

// v (8 lanes) -> three bf16x8 parts summing to v exactly
__device__ __forceinline__ void dsplit3(const float (&v)[8], dbf16x8 (&o)[3]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const __bf16 h0 = (__bf16)v[j];
        const float r1 = v[j] - (float)h0;
        const __bf16 h1 = (__bf16)r1;
        o[0][j] = h0;
        o[1][j] = h1;
        o[2][j] = (__bf16)(r1 - (float)h1);
    }
}

}  // namespace nconv
