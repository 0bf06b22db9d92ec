// metrics.hip — the depth-completion evaluation figures (KITTI: MAE, RMSE, iMAE, iRMSE; NYU: REL,
// squared REL, RMSE(log), delta < 1.25^k) as twelve raw sums per image, in two kernels.
//
//   valid   g > 0, g >= gt_min, g <= gt_max (a bound of 0 is absent)
//   p       the prediction clamped into [clamp_lo, clamp_hi] (a bound of 0 is absent; a NaN stays NaN)
//   e       p - g;  positive = valid and p > 0 (the inverse, log and delta terms)
//   sums    0 n_valid  1 n_pos  2 sum|e|  3 sum e^2  4 sum|e|/g  5 sum e^2/g  6 sum|1/p - 1/g|
//           7 sum(1/p - 1/g)^2  8 sum(ln p - ln g)^2  9-11 #{max(p/g, g/p) < 1.25, 1.25^2, 1.25^3}
//
// In PyTorch these are ~40 elementwise / reduction launches per frame; here, on the loss's 16 x 64
// pixel tiles (four consecutive pixels of a row per thread: plane_io.h's loss_quad):
//   metrics_partials  one workgroup per tile of one image: the per-pixel terms in fp32 (IEEE division,
//                     logf, no contraction), twelve fp32 tile partials (counts <= 1024 are exact) in
//                     wave_ops.h's order
//   metrics_finalize  one block of sixteen waves: a wave per image sums its tiles (image_tile_sums)
//                     -> sums[b][0..11]; then accum[k] += image 0, 1, .. B-1 in that order
// Deterministic (no atomics), no host synchronisation, 2 x 4 bytes read per pixel.
#include "nconv_internal.h"

namespace nconv {

constexpr int kMT = 256;
constexpr int kFT = 1024;  // finalize: sixteen waves, one image each at a time
constexpr int kNS = NCONV_DEPTH_METRICS_SUMS;

// one pixel's terms added to the thread's twelve sums
__device__ __forceinline__ void metrics_pixel(float pr, float g, const MetricsArgs& a, float (&s)[kNS]) {
#pragma clang fp contract(off)
    const bool valid = g > 0.f && g >= a.g_lo && g <= a.g_hi;
    float p = pr;  // comparisons, not fminf / fmaxf: a NaN prediction stays NaN
    p = p < a.c_lo ? a.c_lo : p;
    p = p > a.c_hi ? a.c_hi : p;
    const bool pos = valid && p > 0.f;
    const float e = p - g, ae = fabsf(e), e2 = e * e;
    const float d = 1.f / p - 1.f / g;
    const float l = logf(p) - logf(g);
    const float ratio = fmaxf(p / g, g / p);
    s[0] += valid ? 1.f : 0.f;
    s[1] += pos ? 1.f : 0.f;
    s[2] += valid ? ae : 0.f;
    s[3] += valid ? e2 : 0.f;
    s[4] += valid ? ae / g : 0.f;
    s[5] += valid ? e2 / g : 0.f;
    s[6] += pos ? fabsf(d) : 0.f;
    s[7] += pos ? d * d : 0.f;
    s[8] += pos ? l * l : 0.f;
    s[9] += pos && ratio < 1.25f ? 1.f : 0.f;
    s[10] += pos && ratio < 1.5625f ? 1.f : 0.f;
    s[11] += pos && ratio < 1.953125f ? 1.f : 0.f;
}

// one workgroup per tile; part[tile][0..11], tiles of image b at b * tiles-per-image (a fixed order)
__global__ __launch_bounds__(kMT) void metrics_partials(MetricsArgs a, float* __restrict__ part) {
    __shared__ float red[kMT / 64][kNS];
    const Quad q = loss_quad(a.H, a.W);  // pixels outside the plane read 0 (an invalid target)
    const f4 pv = load4_f32(a.p, a.H, a.W, q), gv = load4_f32(a.g, a.H, a.W, q);
    float s[kNS];
#pragma unroll
    for (int k = 0; k < kNS; ++k) s[k] = 0.f;
    metrics_pixel(pv.x, gv.x, a, s);
    metrics_pixel(pv.y, gv.y, a, s);
    metrics_pixel(pv.z, gv.z, a, s);
    metrics_pixel(pv.w, gv.w, a, s);
#pragma unroll
    for (int k = 0; k < kNS; ++k) s[k] = wave_sum(s[k]);
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < kNS; ++k) red[w][k] = s[k];
    }
    __syncthreads();
    if (threadIdx.x < kNS) part[(size_t)blockIdx.x * kNS + threadIdx.x] = waves_in_order(&red[0][threadIdx.x], kNS);
}

// One block. Wave w reduces images w, w + 16, .. (image_tile_sums); the image's row goes to img
// (workspace) and to sums. After the barrier thread k adds img[0..B)[k] in order into accum[k].
__global__ __launch_bounds__(kFT) void metrics_finalize(const float* __restrict__ part, int B, int tiles,
                                                         double* __restrict__ img, double* __restrict__ sums,
                                                         double* __restrict__ accum) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int b = w; b < B; b += kFT / 64) {
        double s[kNS];
        image_tile_sums(part + (size_t)b * tiles * kNS, tiles, lane, s);
        double mine = 0.0;  // lane k keeps sum k
#pragma unroll
        for (int k = 0; k < kNS; ++k) mine = lane == k ? s[k] : mine;
        if (lane < kNS) {
            img[(size_t)b * kNS + lane] = mine;
            if (sums) sums[(size_t)b * kNS + lane] = mine;
        }
    }
    if (!accum) return;
    __syncthreads();  // img rows written by this block's waves
    if (threadIdx.x < kNS) {
        double acc = accum[threadIdx.x];
        for (int b = 0; b < B; ++b) acc += img[(size_t)b * kNS + threadIdx.x];
        accum[threadIdx.x] = acc;
    }
}

size_t metrics_workspace_bytes(int B, int H, int W) {
    return (size_t)B * kNS * sizeof(double) + (size_t)B * loss_tiles_per_image(H, W) * kNS * sizeof(float);
}

int launch_metrics(const MetricsArgs& a, double* sums, double* accum, void* ws, hipStream_t st, const char** why) {
    const int tiles = loss_tiles_per_image(a.H, a.W);
    double* img = (double*)ws;
    float* part = (float*)(img + (size_t)a.B * kNS);
    hipLaunchKernelGGL(metrics_partials, dim3(a.B * tiles), dim3(kMT), 0, st, a, part);
    hipLaunchKernelGGL(metrics_finalize, dim3(1), dim3(kFT), 0, st, part, a.B, tiles, img, sums, accum);
    return launch_status(why);
}

}  // namespace nconv
