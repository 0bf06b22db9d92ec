// wave_ops.h — the sums and scans over a wave and over a workgroup, defined once. The project's rule
// is "the same bits on every run, in a stated order"; this is where the order is stated, and the
// tests' error bounds and tests/reduce_tree.py restate it from here.
//
//   wave_sum        the xor butterfly over the 64 lanes: v += v of lane ^ 32, then ^ 16, 8, 4, 2, 1.
//                   Every lane ends with the same total.
//   waves_in_order  the per-wave totals that lane 0 of each wave left in LDS, added in wave order:
//                   ((w0 + w1) + w2) + w3.
//   block_sum4      a workgroup of four waves: wave_sum, red[wave] by lane 0, a barrier,
//                   waves_in_order. block_sum4_again is the same with a barrier before the write, for
//                   a caller that passes the same red to consecutive calls.
//   image_tile_sums the finalize stage of the per-tile partial sums (conf_loss.hip, metrics.hip,
//                   view_warp.hip, smooth_loss.hip): by one wave, lane l adds its image's tiles l, l + 64, .. in that
//                   order in double, then wave_sum. The caller adds the images in order.
//   wave_incl_scan  the inclusive prefix over the lanes of a wave by __shfl_up 1, 2, .., 32.
//   block_excl_scan the exclusive prefix over the threads of NWAVES waves in thread order, and the
//                   total: the wave totals through LDS, those of the lower waves added in wave order,
//                   base + inclusive - v.
//
// A kernel that needs another shape (several sums behind one barrier, a sum only some threads read)
// composes wave_sum and waves_in_order itself; the order stays the one above. Trees over fewer than
// 64 lanes and the min / max trees are not sums in this order and stay where they are.
#pragma once
#include <hip/hip_runtime.h>

namespace nconv {

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// red[w * stride] holds wave w's total
template <typename T>
__device__ __forceinline__ T waves_in_order(const T* red, int stride = 1) {
    return ((red[0] + red[stride]) + red[2 * stride]) + red[3 * stride];
}

template <bool AGAIN, typename T>
__device__ __forceinline__ T block_sum4_impl(T v, T* red) {
    v = wave_sum(v);
    if (AGAIN) __syncthreads();  // red of the call before has been read
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return waves_in_order(red);
}
template <typename T>
__device__ __forceinline__ T block_sum4(T v, T* red) {
    return block_sum4_impl<false>(v, red);
}
template <typename T>
__device__ __forceinline__ T block_sum4_again(T v, T* red) {
    return block_sum4_impl<true>(v, red);
}

// part: the image's tiles, K fp32 sums each; s[k] = sum k of the image, in every lane
template <int K>
__device__ __forceinline__ void image_tile_sums(const float* part, int tiles, int lane, double (&s)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = 0.0;
    for (int t = lane; t < tiles; t += 64) {
#pragma unroll
        for (int k = 0; k < K; ++k) s[k] += (double)part[(size_t)t * K + k];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = wave_sum(s[k]);
}

template <typename T>
__device__ __forceinline__ T wave_incl_scan(T v) {
    const int lane = (int)threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    return v;
}

// s_wave: NWAVES words of LDS. AGAIN: a barrier before they are written, for a caller that passes
// the same s_wave to consecutive calls; a caller in a loop places its own.
template <int NWAVES, typename T, bool AGAIN = false>
__device__ __forceinline__ T block_excl_scan(T v, T* s_wave, T& total) {
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const T inc = wave_incl_scan(v);
    if (AGAIN) __syncthreads();
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    T base = 0;
    total = 0;
#pragma unroll
    for (int i = 0; i < NWAVES; ++i) {
        if (i < wave) base += s_wave[i];
        total += s_wave[i];
    }
    return base + inc - v;
}

}  // namespace nconv
