// photo_ssim.hip — the photometric loss of the monodepth family with its structural term,
//   L = alpha Lw + (1 - alpha) Lv,   Lw = mean over windows and channels of clamp((1 - SSIM) / 2, 0, 1),
//                                    Lv = view_warp.hip's L1 mean over the valid pixels,
// with the warp fused in, and its gradient with respect to the depth. SSIM is taken over the 3 x 3 window
// of a pixel whose nine pixels are all valid (no reflection padding: a one-pixel frame and the
// neighbourhood of every invalid pixel have no window). The rule is stated operation by operation in
// include/nconv.h (nconv_photo_ssim_loss_*); every operation here is fp32 in that order, no contraction.
//
// One workgroup of 256 threads per 16 x 64 tile of one image (view_warp.hip's tile and thread map: lane =
// column, wave w owns rows w, w + 4, w + 8, w + 12). Unlike the L1 kernels these are not per-pixel: a
// window needs its neighbours' warped values, so a workgroup warps its tile and a halo into LDS first.
//
//   ssim_partials   stages x = warp(src), y = tgt and a validity byte of the tile and a one-pixel halo
//                   (18 x 66 pixels, every channel; the halo is re-projected from the depth, a pixel
//                   outside the image is not valid), one barrier, then every thread forms the windows of its
//                   four pixels from LDS. Per tile: the fp32 sums of its 1024 L1 terms (photo_partials' order
//                   and bits) and of its 1024 SSIM terms, and the counts of valid pixels and of windows
//   ssim_finalize   one block: a wave per image sums its tiles (image_tile_sums<2>; the counts in integers),
//                   thread 0 adds the images in order and writes n_v, n_w and L
//   ssim_grad       d ssim_p / d x_q = a_p + b_p x_q + c_p y_q is affine in the pixel q of the window p, so
//                   g_x(q) needs only the sums of a, b, c over the up to nine windows that hold q: a box sum, a
//                   gather. Stages x, y and validity of the tile and a two-pixel halo (20 x 68, every channel),
//                   then per channel a, b, c of the 18 x 66 windows around the tile (LDS reused by the
//                   channels), and gathers; g_depth by warp_gterm. The forward saves no planes: nothing
//                   per-pixel but g_depth reaches memory
//
// Static LDS: ssim_partials<3> 29.8 KB, ssim_grad<3> 48.3 KB (x and y of all channels 32.6 KB, validity
// 1.4 KB, one channel's a, b, c 14.3 KB), both below 64 KB. The image comes from blockIdx alone, so K, m and
// the planes' buffer resources stay wave-uniform; an invalid pixel loads no tap and no tgt; no byte outside
// a view is read. No atomics, no host synchronisation, no allocation: capturable, the same bits on every run.
//
// The window pieces (the regions, stage_pixel, window_valid, ssim_window, ssim_term, ssim_coef) are
// ssim_common.h's, shared with photo_min.hip.
#include "ssim_common.h"

namespace nconv {

namespace {

constexpr int kSsimF = 1024;                             // finalize: sixteen waves, one image each at a time
// the workspace: n_v, n_w first (the backward and the caller read them there); [.][0] L1, [.][1] SSIM
struct SsimWs {
    int* n;        // [2]: n_v, n_w
    double* img;   // [B][2]
    int* icnt;     // [B][2]
    float* part;   // [B * tiles][2]
    int* cnt;      // [B * tiles][2]
};
__host__ __device__ SsimWs ssim_ws(void* ws, int B, int tiles) {
    SsimWs p;
    p.n = (int*)ws;
    p.img = (double*)(p.n + 2);
    p.icnt = (int*)(p.img + 2 * (size_t)B);
    p.part = (float*)(p.icnt + 2 * (size_t)B);
    p.cnt = (int*)(p.part + 2 * (size_t)B * tiles);
    return p;
}

// one workgroup per tile; part[2 tile + k] and cnt[2 tile + k], k = 0: L1 and n_v, 1: SSIM and n_w
template <int C>
__global__ __launch_bounds__(kWT) void ssim_partials(WarpArgs a, float c1, float c2, float* __restrict__ part,
                                                     int* __restrict__ cnt) {
#pragma clang fp contract(off)
    __shared__ float sx[C][kFN], sy[C][kFN];
    __shared__ unsigned char sv[kFN];
    __shared__ float red[2][kWT / 64];
    __shared__ int redc[2][kWT / 64];
    const TileOrigin o = tile_origin<kLossTH, kLossTW>(a.H, a.W);
    const Camera cam = warp_camera(a, o.b);
    const Proj q = proj_of(a, o.b);
#pragma unroll 1
    for (int idx = threadIdx.x; idx < kFN; idx += kWT)
        stage_pixel<C, kFW, kFN>(a, cam, q, o.b, o.i0 - 1, o.j0 - 1, idx, sx, sy, sv);
    __syncthreads();
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float s1 = 0.f, sw = 0.f;
    int n1 = 0, nw = 0;
#pragma unroll 1
    for (int r = 0; r < kWRows; ++r) {
        const int at = (w + r * (kWT / 64) + 1) * kFW + lane + 1;
        const bool ok = sv[at] != 0;
        const bool win = window_valid<kFW>(sv, at);
        float term = 0.f, termw = 0.f;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            const float e = fabsf(sx[ch][at] - sy[ch][at]);
            term = ch == 0 ? e : term + e;
            const Ssim s = ssim_window<kFW>(sx[ch], sy[ch], at, c1, c2);
            const float ew = ssim_term(s);
            termw = ch == 0 ? ew : termw + ew;
        }
        s1 += ok ? term : 0.f;
        n1 += ok ? 1 : 0;
        sw += win ? termw : 0.f;
        nw += win ? 1 : 0;
    }
    s1 = wave_sum(s1), sw = wave_sum(sw), n1 = wave_sum(n1), nw = wave_sum(nw);
    if (lane == 0) red[0][w] = s1, red[1][w] = sw, redc[0][w] = n1, redc[1][w] = nw;
    __syncthreads();
    if (threadIdx.x < 2) {
        part[2 * (size_t)blockIdx.x + threadIdx.x] = waves_in_order(red[threadIdx.x]);
        cnt[2 * (size_t)blockIdx.x + threadIdx.x] = waves_in_order(redc[threadIdx.x]);
    }
}

// One block. Wave w reduces images w, w + 16, .. (image_tile_sums<2>; the counts likewise in integers).
// After the barrier thread 0 adds the images in order and writes n_v, n_w and
// L = (alpha * Lw) + ((1.0f - alpha) * Lv), Lv = photo_finalize's L, Lw = (float)(Sw / ((double)C * max(n_w, 1))).
__global__ __launch_bounds__(kSsimF) void ssim_finalize(const float* __restrict__ part, const int* __restrict__ cnt,
                                                        int B, int tiles, int C, float alpha,
                                                        double* __restrict__ img, int* __restrict__ icnt,
                                                        int* __restrict__ n_out, float* __restrict__ loss) {
#pragma clang fp contract(off)
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int b = w; b < B; b += kSsimF / 64) {
        const int* cb = cnt + 2 * (size_t)b * tiles;
        double s[2];
        image_tile_sums(part + 2 * (size_t)b * tiles, tiles, lane, s);
        int nv = 0, nw = 0;
        for (int t = lane; t < tiles; t += 64) nv += cb[2 * t], nw += cb[2 * t + 1];
        nv = wave_sum(nv), nw = wave_sum(nw);
        if (lane == 0) img[2 * b] = s[0], img[2 * b + 1] = s[1], icnt[2 * b] = nv, icnt[2 * b + 1] = nw;
    }
    __syncthreads();  // img and icnt written by this block's waves
    if (threadIdx.x == 0) {
        double av = 0.0, aw = 0.0;
        int nv = 0, nw = 0;
        for (int b = 0; b < B; ++b) av += img[2 * b], aw += img[2 * b + 1], nv += icnt[2 * b], nw += icnt[2 * b + 1];
        n_out[0] = nv, n_out[1] = nw;
        const float den = (float)C * (float)max(nv, 1);
        const float Lv = (float)(av / (double)den);
        const float Lw = (float)(aw / ((double)C * (double)max(nw, 1)));
        const float pw = alpha * Lw, pv = (1.0f - alpha) * Lv;
        loss[0] = pw + pv;
    }
}

template <int C>
__global__ __launch_bounds__(kWT) void ssim_grad(WarpArgs a, float alpha, float c1, float c2,
                                                 const float* __restrict__ gloss, const int* __restrict__ n,
                                                 float* __restrict__ g_depth) {
#pragma clang fp contract(off)
    __shared__ float sx[C][kGN], sy[C][kGN];
    __shared__ unsigned char sv[kGN];
    __shared__ float wa[kFN], wb[kFN], wc[kFN];
    const TileOrigin o = tile_origin<kLossTH, kLossTW>(a.H, a.W);
    const Camera cam = warp_camera(a, o.b);
    const Proj q = proj_of(a, o.b);
#pragma unroll 1
    for (int idx = threadIdx.x; idx < kGN; idx += kWT)
        stage_pixel<C, kGW, kGN>(a, cam, q, o.b, o.i0 - 2, o.j0 - 2, idx, sx, sy, sv);
    const float gl = gloss ? gloss[0] : 1.f;
    const float den_v = (float)C * (float)max(n[0], 1), den_w = (float)C * (float)max(n[1], 1);
    const float inv_v = 1.0f / den_v, inv_w = 1.0f / den_w;
    const float kl = (gl * (1.0f - alpha)) * inv_v;  // the L1 part's factor
    const float kw = gl * inv_w;
    const float kq = (alpha * 0.5f) * kw;            // the SSIM part's
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll 1
    for (int ch = 0; ch < C; ++ch) {
        __syncthreads();  // x, y and validity staged (ch == 0); a, b, c of the channel before gathered
#pragma unroll 1
        for (int idx = threadIdx.x; idx < kFN; idx += kWT) {
            const int at = (idx / kFW + 1) * kGW + idx % kFW + 1;  // the window's centre in the 20 x 68 region
            const Ssim s = ssim_window<kGW>(sx[ch], sy[ch], at, c1, c2);
            const bool pass = window_valid<kGW>(sv, at) && s.t >= 0.f && s.t <= 1.f;
            const SsimCoef k = ssim_coef(s);
            wa[idx] = pass ? k.a : 0.f, wb[idx] = pass ? k.b : 0.f, wc[idx] = pass ? k.c : 0.f;
        }
        __syncthreads();
#pragma unroll 1
        for (int r = 0; r < kWRows; ++r) {
            const int ti = w + r * (kWT / 64);
            float SA = 0.f, SB = 0.f, SC = 0.f;
#pragma unroll
            for (int di = 0; di <= 2; ++di) {
#pragma unroll
                for (int dj = 0; dj <= 2; ++dj) {
                    const int p = (ti + di) * kFW + lane + dj;  // the windows centred around (ti + 1, lane + 1)
                    SA = SA + wa[p], SB = SB + wb[p], SC = SC + wc[p];
                }
            }
            const int own = (ti + 2) * kGW + lane + 2;
            const float bx = SB * sx[ch][own], cy = SC * sy[ch][own];
            const float ab = SA + bx;
            const float inner = ab + cy;
            const float scaled = kq * inner;
            sx[ch][own] = -scaled;  // g_x takes x_q's place: from here on only this thread reads it
        }
    }
    const size_t plane = (size_t)a.H * a.W;
#pragma unroll 1
    for (int r = 0; r < kWRows; ++r) {
        const int ti = w + r * (kWT / 64);
        const int i = o.i0 + ti, j = o.j0 + lane;
        const bool inside = i < a.H && j < a.W;
        const Geo g = warp_geometry(a, cam, q, o.b, i, j, inside);
        if (!inside) continue;
        float du, dv;
        warp_duv(cam, q, g, i, j, du, dv);
        const int own = (ti + 2) * kGW + lane + 2;
        float acc = 0.f;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            const Sample p = warp_sample(a, g, o.b, ch);
            const float d = p.s - sy[ch][own];
            const float sg = d > 0.f ? 1.f : d < 0.f ? -1.f : 0.f;
            const float l1 = kl * sg;
            const float gs = l1 + sx[ch][own];
            const float term = warp_gterm(g, p, gs, du, dv);
            acc = ch == 0 ? term : acc + term;
        }
        g_depth[(size_t)o.b * plane + (size_t)i * a.W + j] = g.ok ? acc : 0.f;
    }
}

}  // namespace

size_t photo_ssim_workspace_bytes(int B, int H, int W) {
    // ssim_ws: n_v and n_w, img, icnt, part, cnt
    return 8 + (size_t)B * 16 + (size_t)B * 8 + (size_t)B * loss_tiles_per_image(H, W) * 16;
}

int launch_photo_ssim_loss_fwd(const WarpArgs& a, float alpha, float c1, float c2, float* loss, void* ws,
                               hipStream_t st, const char** why) {
    const int tiles = loss_tiles_per_image(a.H, a.W);
    const SsimWs p = ssim_ws(ws, a.B, tiles);
    const dim3 g(a.B * tiles), t(kWT);
    if (a.C == 1)
        hipLaunchKernelGGL(ssim_partials<1>, g, t, 0, st, a, c1, c2, p.part, p.cnt);
    else
        hipLaunchKernelGGL(ssim_partials<3>, g, t, 0, st, a, c1, c2, p.part, p.cnt);
    hipLaunchKernelGGL(ssim_finalize, dim3(1), dim3(kSsimF), 0, st, p.part, p.cnt, a.B, tiles, a.C, alpha, p.img,
                       p.icnt, p.n, loss);
    return launch_status(why);
}

int launch_photo_ssim_loss_bwd(const WarpArgs& a, float alpha, float c1, float c2, const float* gloss, const void* ws,
                               float* g_depth, hipStream_t st, const char** why) {
    const dim3 g(a.B * loss_tiles_per_image(a.H, a.W)), t(kWT);
    const int* n = (const int*)ws;
    if (a.C == 1)
        hipLaunchKernelGGL(ssim_grad<1>, g, t, 0, st, a, alpha, c1, c2, gloss, n, g_depth);
    else
        hipLaunchKernelGGL(ssim_grad<3>, g, t, 0, st, a, alpha, c1, c2, gloss, n, g_depth);
    return launch_status(why);
}

}  // namespace nconv
