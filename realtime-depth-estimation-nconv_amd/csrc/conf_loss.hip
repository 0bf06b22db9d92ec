// conf_loss.hip — the confidence loss of the NConv authors (Eldesokey, Felsberg, Khan, "Confidence
// Propagation through CNNs for Guided Sparse Depth Regression", TPAMI 2019; ConfLossDecay in their
// code) on the prediction r, the output confidence c and the target t, forward and backward fused.
//
//   v    = t != 0
//   d    = r - t,  a = |d|
//   e    = smooth_l1: a < beta ? ((0.5 a) a) / beta : a - 0.5 beta        l2: d d
//   de   = smooth_l1: a < beta ? d / beta : (d > 0 ? 1 : -1)              l2: 2 d
//   term = v ? e - (lam c) (1 - e) : 0         (the published err - lam (c v - err c v), lam = 1 / p)
//   L    = (sum term) / n,  n = B H W: the mean over all pixels
//   k    = gloss (1 / n);  g_r = v ? (k de) (1 + lam c) : 0;  g_c = v ? -((k lam) (1 - e)) : 0
//
// Every operation in fp32 in the order written (include/nconv.h), no contraction. lam is a device
// scalar, so a captured training step decays it per epoch without another capture. On the loss's
// 16 x 64 pixel tiles, four consecutive pixels of a row per thread (plane_io.h's loss_quad):
//   conf_loss_partials  one workgroup per tile of one image: the tile's 1024 terms summed in fp32
//                       (a thread's four in order, then wave_ops.h's block_sum4)
//   conf_loss_finalize  one block: a wave per image sums its tiles (image_tile_sums), then thread 0
//                       adds the images in order and writes L
//   conf_loss_grad      one workgroup per tile: g_r, g_c (contiguous B x H x W), overwritten
// Deterministic (no atomics), no host synchronisation.
#include "nconv_internal.h"

namespace nconv {

constexpr int kCT = 256;
constexpr int kCF = 1024;            // finalize: sixteen waves, one image each at a time

// e and de of one pixel (KIND: enum nconv_conf_loss_err)
template <int KIND>
__device__ __forceinline__ void conf_err(float r, float t, float beta, float& e, float& de) {
#pragma clang fp contract(off)
    const float d = r - t;
    if constexpr (KIND == NCONV_CONF_LOSS_SMOOTH_L1) {
        const float a = fabsf(d);
        e = a < beta ? ((0.5f * a) * a) / beta : a - 0.5f * beta;
        de = a < beta ? d / beta : (d > 0.f ? 1.f : -1.f);
    } else {
        e = d * d;
        de = 2.f * d;
    }
}

template <int KIND>
__device__ __forceinline__ float conf_term(float r, float c, float t, float beta, float lam) {
#pragma clang fp contract(off)
    float e, de;
    conf_err<KIND>(r, t, beta, e, de);
    return t != 0.f ? e - (lam * c) * (1.0f - e) : 0.f;
}

// one workgroup per tile; part[tile], tiles of image b at b * tiles-per-image (a fixed order)
template <int KIND>
__global__ __launch_bounds__(kCT) void conf_loss_partials(ConfLossArgs a, float* __restrict__ part) {
#pragma clang fp contract(off)
    __shared__ float red[kCT / 64];
    const Quad q = loss_quad(a.H, a.W);
    // pixels outside the plane read 0 (t = 0: no term, no gradient)
    const f4 rv = load4_f32(a.r, a.H, a.W, q), cv = load4_f32(a.c, a.H, a.W, q), tv = load4_f32(a.t, a.H, a.W, q);
    const float lam = a.lam[0], beta = a.beta;
    float s = conf_term<KIND>(rv.x, cv.x, tv.x, beta, lam);
    s += conf_term<KIND>(rv.y, cv.y, tv.y, beta, lam);
    s += conf_term<KIND>(rv.z, cv.z, tv.z, beta, lam);
    s += conf_term<KIND>(rv.w, cv.w, tv.w, beta, lam);
    s = block_sum4(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// One block. Wave w reduces images w, w + 16, .. (image_tile_sums) -> img[b]. After the barrier
// thread 0 adds img[0..B) in order.
__global__ __launch_bounds__(kCF) void conf_loss_finalize(const float* __restrict__ part, int B, int tiles, double n,
                                                           double* __restrict__ img, float* __restrict__ loss) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int b = w; b < B; b += kCF / 64) {
        double s[1];
        image_tile_sums(part + (size_t)b * tiles, tiles, lane, s);
        if (lane == 0) img[b] = s[0];
    }
    __syncthreads();  // img written by this block's waves
    if (threadIdx.x == 0) {
        double acc = 0.0;
        for (int b = 0; b < B; ++b) acc += img[b];
        loss[0] = (float)(acc / n);
    }
}

template <int KIND>
__global__ __launch_bounds__(kCT) void conf_loss_grad(ConfLossArgs a, const float* __restrict__ gloss,
                                                       float* __restrict__ g_r, float* __restrict__ g_c) {
#pragma clang fp contract(off)
    const Quad q = loss_quad(a.H, a.W);
    // pixels outside the plane read 0 (t = 0: no term, no gradient)
    const f4 rv = load4_f32(a.r, a.H, a.W, q), cv = load4_f32(a.c, a.H, a.W, q), tv = load4_f32(a.t, a.H, a.W, q);
    const float lam = a.lam[0], beta = a.beta;
    const float n = (float)((long long)a.B * a.H * a.W);
    const float k = (gloss ? gloss[0] : 1.f) * (1.0f / n);
    if (!q.row_in) return;
    const size_t o = ((size_t)q.b * a.H + q.i) * a.W + q.j;
    const float r4[4] = {rv.x, rv.y, rv.z, rv.w}, c4[4] = {cv.x, cv.y, cv.z, cv.w}, t4[4] = {tv.x, tv.y, tv.z, tv.w};
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        if (m >= q.n) break;
        float e, de;
        conf_err<KIND>(r4[m], t4[m], beta, e, de);
        const bool v = t4[m] != 0.f;
        if (g_r) g_r[o + m] = v ? (k * de) * (1.0f + lam * c4[m]) : 0.f;
        if (g_c) g_c[o + m] = v ? -((k * lam) * (1.0f - e)) : 0.f;
    }
}

size_t conf_loss_workspace_bytes(int B, int H, int W) {
    return (size_t)B * sizeof(double) + (size_t)B * loss_tiles_per_image(H, W) * sizeof(float);
}

int launch_conf_loss_fwd(const ConfLossArgs& a, float* loss, void* ws, hipStream_t st, const char** why) {
    const int tiles = loss_tiles_per_image(a.H, a.W);
    double* img = (double*)ws;
    float* part = (float*)(img + a.B);
    const dim3 g(a.B * tiles), t(kCT);
    if (a.kind == NCONV_CONF_LOSS_SMOOTH_L1)
        hipLaunchKernelGGL(conf_loss_partials<NCONV_CONF_LOSS_SMOOTH_L1>, g, t, 0, st, a, part);
    else
        hipLaunchKernelGGL(conf_loss_partials<NCONV_CONF_LOSS_L2>, g, t, 0, st, a, part);
    hipLaunchKernelGGL(conf_loss_finalize, dim3(1), dim3(kCF), 0, st, part, a.B, tiles, (double)a.B * a.H * a.W, img,
                       loss);
    return launch_status(why);
}

int launch_conf_loss_bwd(const ConfLossArgs& a, const float* gloss, float* g_r, float* g_c, hipStream_t st,
                         const char** why) {
    const dim3 g(a.B * loss_tiles_per_image(a.H, a.W)), t(kCT);
    if (a.kind == NCONV_CONF_LOSS_SMOOTH_L1)
        hipLaunchKernelGGL(conf_loss_grad<NCONV_CONF_LOSS_SMOOTH_L1>, g, t, 0, st, a, gloss, g_r, g_c);
    else
        hipLaunchKernelGGL(conf_loss_grad<NCONV_CONF_LOSS_L2>, g, t, 0, st, a, gloss, g_r, g_c);
    return launch_status(why);
}

}  // namespace nconv
