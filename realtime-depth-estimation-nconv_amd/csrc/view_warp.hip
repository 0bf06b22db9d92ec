// view_warp.hip — a neighbouring camera frame warped into the current view by the predicted depth and a
// known relative pose, the gradient of that with respect to the depth, and the photometric (L1) loss
// on top of it with the warp fused in: the self-supervised term of Ma, Cavalheiro and Karaman (ICRA 2019)
// and the monodepth family. The rule is stated operation by operation in include/nconv.h
// (nconv_view_warp_*, nconv_photo_loss_*); every operation here is fp32 in that order, no contraction.
//
// Per target pixel (b, i, j), z = depth[b][i][j]:
//   P = (x, y, z)          backproject_common.h's project(): x = ((float)j - cx) * z / fx, likewise y
//   a, b, c = dot(m[0..2], P), dot(r, P) = ((r0 x + r1 y) + r2 z) + r3 (lidar_project.hip's), u = a / c, v = b / c
//   valid                  z > z_min && z <= z_max && c > 0 && 0 <= u <= Ws - 1 && 0 <= v <= Hs - 1 && mask
//   taps                   j0 = floor(u), j1 = min(j0 + 1, Ws - 1), wu = u - floor(u), w0u = 1 - wu; likewise i, v
//   s[ch]                  w0v (w0u a00 + wu a01) + wv (w0u a10 + wu a11)
//   g_depth                sum_ch g_s[ch] (dIu[ch] du + dIv[ch] dv): each target pixel owns its four taps, so
//                          the gradient with respect to the depth is a gather, not a scatter
//
// One workgroup of 256 threads per 16 x 64 tile of one image (the loss's tile): a wave's 64 lanes lie
// along a row, so depth, mask, tgt, warped, valid and g_depth move 256 contiguous bytes per wave and
// row; a thread takes rows w, w + 4, w + 8, w + 12 of the tile (w its wave). The image comes from
// blockIdx alone, so its K and m are read from wave-uniform addresses (scalar loads, scalar registers)
// and the buffer resources of its planes are scalar too. The four taps are a gather: under the small
// inter-frame motion this is used with, neighbouring lanes read neighbouring addresses, and the cache
// line a wave's row touches is shared by its four loads. The backward recomputes the projection from
// the depth (one 4-byte read per pixel) instead of reading stored u, v and a validity byte (9 bytes).
//
//   view_warp_fwd        warped (B, C, H, W) and / or valid (B, H, W)
//   view_warp_bwd        g_depth from g_warped
//   photo_partials       per tile: the fp32 sum of its 1024 terms sum_ch |s - tgt| (a thread's four in row
//                        order, then wave_ops.h's wave_sum and waves_in_order) and its valid count
//   photo_finalize       one block: a wave per image sums its tiles (image_tile_sums; the counts in
//                        integers), thread 0 adds the images in order and writes n_v and L
//   photo_grad           g_depth with g_s = kk sign(s - tgt), kk from the device's n_v: neither warped
//                        nor g_s reaches memory
//
// An invalid pixel loads no tap (its loads are aimed at plane_io.h's kOOB); a valid one reads taps
// inside [0, Hs - 1] x [0, Ws - 1] by the clamps, so no byte outside a view's extent is read. No
// atomics, no host synchronisation, no allocation: capturable, and the same bits on every run.
//
// The per-pixel pieces (Geo, warp_geometry, warp_sample, warp_duv, warp_gterm, tgt_load, Proj,
// warp_camera, the tile's thread map) are warp_common.h's, shared with photo_ssim.hip.
#include "warp_common.h"

namespace nconv {

namespace {

constexpr int kWF = 1024;              // finalize: sixteen waves, one image each at a time

// the photometric loss's workspace: n_v first (the backward and the caller read it there)
struct PhotoWs {
    int* n_v;       // [2]: the count and padding
    double* img;    // [B]
    int* icnt;      // [B rounded up to even]
    float* part;    // [B * tiles]
    int* cnt;       // [B * tiles]
};
__host__ __device__ PhotoWs photo_ws(void* ws, int B, int tiles) {
    PhotoWs p;
    p.n_v = (int*)ws;
    p.img = (double*)(p.n_v + 2);
    p.icnt = (int*)(p.img + B);
    p.part = (float*)(p.icnt + B + (B & 1));
    p.cnt = (int*)(p.part + (size_t)B * tiles);
    return p;
}

template <int C>
__global__ __launch_bounds__(kWT) void view_warp_fwd(WarpArgs a, float* __restrict__ warped,
                                                     unsigned char* __restrict__ valid) {
    const WarpTile t = warp_tile(a);
    const Camera cam = warp_camera(a, t.b);
    const Proj q = proj_of(a, t.b);
    const size_t plane = (size_t)a.H * a.W;
#pragma unroll
    for (int r = 0; r < kWRows; ++r) {
        const int i = t.i0 + r * (kWT / 64);
        const bool inside = i < a.H && t.j < a.W;
        const Geo g = warp_geometry(a, cam, q, t.b, i, t.j, inside);
        if (!inside) continue;
        const size_t o = (size_t)i * a.W + t.j;
        if (valid) valid[(size_t)t.b * plane + o] = g.ok ? 1 : 0;
        if (warped) {
#pragma unroll
            for (int ch = 0; ch < C; ++ch) {
                const Sample p = warp_sample(a, g, t.b, ch);
                warped[((size_t)t.b * C + ch) * plane + o] = g.ok ? p.s : 0.f;
            }
        }
    }
}

template <int C>
__global__ __launch_bounds__(kWT) void view_warp_bwd(WarpArgs a, const float* __restrict__ g_warped,
                                                     float* __restrict__ g_depth) {
#pragma clang fp contract(off)
    const WarpTile t = warp_tile(a);
    const Camera cam = warp_camera(a, t.b);
    const Proj q = proj_of(a, t.b);
    const size_t plane = (size_t)a.H * a.W;
#pragma unroll
    for (int r = 0; r < kWRows; ++r) {
        const int i = t.i0 + r * (kWT / 64);
        const bool inside = i < a.H && t.j < a.W;
        const Geo g = warp_geometry(a, cam, q, t.b, i, t.j, inside);
        if (!inside) continue;
        const size_t o = (size_t)i * a.W + t.j;
        float du, dv;
        warp_duv(cam, q, g, i, t.j, du, dv);
        float acc = 0.f;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            const Sample p = warp_sample(a, g, t.b, ch);
            const float gs = g_warped[((size_t)t.b * C + ch) * plane + o];
            const float term = warp_gterm(g, p, gs, du, dv);
            acc = ch == 0 ? term : acc + term;
        }
        g_depth[(size_t)t.b * plane + o] = g.ok ? acc : 0.f;
    }
}

// one workgroup per tile; part[tile] and cnt[tile], the tiles of image b at b * tiles-per-image
template <int C>
__global__ __launch_bounds__(kWT) void photo_partials(WarpArgs a, float* __restrict__ part, int* __restrict__ cnt) {
#pragma clang fp contract(off)
    __shared__ float red[kWT / 64];
    __shared__ int redc[kWT / 64];
    const WarpTile t = warp_tile(a);
    const Camera cam = warp_camera(a, t.b);
    const Proj q = proj_of(a, t.b);
    float s = 0.f;
    int n = 0;
#pragma unroll
    for (int r = 0; r < kWRows; ++r) {
        const int i = t.i0 + r * (kWT / 64);
        const bool inside = i < a.H && t.j < a.W;
        const Geo g = warp_geometry(a, cam, q, t.b, i, t.j, inside);
        float term = 0.f;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            const Sample p = warp_sample(a, g, t.b, ch);
            const float e = fabsf(p.s - tgt_load(a, t.b, ch, i, t.j, inside && g.ok));
            term = ch == 0 ? e : term + e;
        }
        s += g.ok ? term : 0.f;
        n += g.ok ? 1 : 0;
    }
    s = wave_sum(s), n = wave_sum(n);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s, redc[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = waves_in_order(red), cnt[blockIdx.x] = waves_in_order(redc);
}

// One block. Wave w reduces images w, w + 16, .. (image_tile_sums; the counts likewise in integers).
// After the barrier thread 0 adds the images in order and writes n_v and
// L = (sum) / ((float)C * (float)max(n_v, 1)).
__global__ __launch_bounds__(kWF) void photo_finalize(const float* __restrict__ part, const int* __restrict__ cnt,
                                                      int B, int tiles, int C, double* __restrict__ img,
                                                      int* __restrict__ icnt, int* __restrict__ n_v,
                                                      float* __restrict__ loss) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int b = w; b < B; b += kWF / 64) {
        const int* cb = cnt + (size_t)b * tiles;
        double s[1];
        image_tile_sums(part + (size_t)b * tiles, tiles, lane, s);
        int n = 0;
        for (int t = lane; t < tiles; t += 64) n += cb[t];
        n = wave_sum(n);
        if (lane == 0) img[b] = s[0], icnt[b] = n;
    }
    __syncthreads();  // img and icnt written by this block's waves
    if (threadIdx.x == 0) {
        double acc = 0.0;
        int n = 0;
        for (int b = 0; b < B; ++b) acc += img[b], n += icnt[b];
        n_v[0] = n;
        const float den = (float)C * (float)max(n, 1);
        loss[0] = (float)(acc / (double)den);
    }
}

template <int C>
__global__ __launch_bounds__(kWT) void photo_grad(WarpArgs a, const float* __restrict__ gloss,
                                                  const int* __restrict__ n_v, float* __restrict__ g_depth) {
#pragma clang fp contract(off)
    const WarpTile t = warp_tile(a);
    const Camera cam = warp_camera(a, t.b);
    const Proj q = proj_of(a, t.b);
    const float den = (float)C * (float)max(n_v[0], 1);
    const float inv = 1.0f / den;
    const float kk = (gloss ? gloss[0] : 1.f) * inv;
    const size_t plane = (size_t)a.H * a.W;
#pragma unroll
    for (int r = 0; r < kWRows; ++r) {
        const int i = t.i0 + r * (kWT / 64);
        const bool inside = i < a.H && t.j < a.W;
        const Geo g = warp_geometry(a, cam, q, t.b, i, t.j, inside);
        if (!inside) continue;
        float du, dv;
        warp_duv(cam, q, g, i, t.j, du, dv);
        float acc = 0.f;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            const Sample p = warp_sample(a, g, t.b, ch);
            const float d = p.s - tgt_load(a, t.b, ch, i, t.j, g.ok);
            const float sg = d > 0.f ? 1.f : d < 0.f ? -1.f : 0.f;
            const float gs = kk * sg;
            const float term = warp_gterm(g, p, gs, du, dv);
            acc = ch == 0 ? term : acc + term;
        }
        g_depth[(size_t)t.b * plane + (size_t)i * a.W + t.j] = g.ok ? acc : 0.f;
    }
}

}  // namespace

size_t photo_loss_workspace_bytes(int B, int H, int W) {
    // photo_ws: n_v and padding, img, icnt (an even number of ints), part, cnt
    return 8 + (size_t)B * 8 + (size_t)(B + (B & 1)) * 4 + (size_t)B * loss_tiles_per_image(H, W) * 8;
}

int launch_view_warp_fwd(const WarpArgs& a, float* warped, unsigned char* valid, hipStream_t st, const char** why) {
    const dim3 g(a.B * loss_tiles_per_image(a.H, a.W)), t(kWT);
    if (a.C == 1)
        hipLaunchKernelGGL(view_warp_fwd<1>, g, t, 0, st, a, warped, valid);
    else
        hipLaunchKernelGGL(view_warp_fwd<3>, g, t, 0, st, a, warped, valid);
    return launch_status(why);
}

int launch_view_warp_bwd(const WarpArgs& a, const float* g_warped, float* g_depth, hipStream_t st, const char** why) {
    const dim3 g(a.B * loss_tiles_per_image(a.H, a.W)), t(kWT);
    if (a.C == 1)
        hipLaunchKernelGGL(view_warp_bwd<1>, g, t, 0, st, a, g_warped, g_depth);
    else
        hipLaunchKernelGGL(view_warp_bwd<3>, g, t, 0, st, a, g_warped, g_depth);
    return launch_status(why);
}

int launch_photo_loss_fwd(const WarpArgs& a, float* loss, void* ws, hipStream_t st, const char** why) {
    const int tiles = loss_tiles_per_image(a.H, a.W);
    const PhotoWs p = photo_ws(ws, a.B, tiles);
    const dim3 g(a.B * tiles), t(kWT);
    if (a.C == 1)
        hipLaunchKernelGGL(photo_partials<1>, g, t, 0, st, a, p.part, p.cnt);
    else
        hipLaunchKernelGGL(photo_partials<3>, g, t, 0, st, a, p.part, p.cnt);
    hipLaunchKernelGGL(photo_finalize, dim3(1), dim3(kWF), 0, st, p.part, p.cnt, a.B, tiles, a.C, p.img, p.icnt, p.n_v,
                       loss);
    return launch_status(why);
}

int launch_photo_loss_bwd(const WarpArgs& a, const float* gloss, const void* ws, float* g_depth, hipStream_t st,
                          const char** why) {
    const dim3 g(a.B * loss_tiles_per_image(a.H, a.W)), t(kWT);
    const int* n_v = (const int*)ws;
    if (a.C == 1)
        hipLaunchKernelGGL(photo_grad<1>, g, t, 0, st, a, gloss, n_v, g_depth);
    else
        hipLaunchKernelGGL(photo_grad<3>, g, t, 0, st, a, gloss, n_v, g_depth);
    return launch_status(why);
}

}  // namespace nconv
