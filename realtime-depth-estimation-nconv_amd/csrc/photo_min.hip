// photo_min.hip — the photometric loss of monodepth2 over several source frames: per target pixel the
// SMALLEST of the sources' reprojection errors E_s = alpha termw_s + (1 - alpha) term_s (the terms of
// photo_ssim.hip and view_warp.hip), optionally dropping a pixel whose UNWARPED source already matches
// better (auto-masking), with every warp fused in, and its gradient with respect to the depth. The rule is
// stated operation by operation in include/nconv.h (nconv_photo_min_loss_*); every operation here is fp32
// in that order, no contraction.
//
// One workgroup of 256 threads per 16 x 64 tile of one image (view_warp.hip's tile and thread map: lane =
// column, wave w owns rows w, w + 4, w + 8, w + 12). The sources are a loop INSIDE the kernels: the LDS that
// holds the warped tile and its validity is reused by every source (and by the identity pass of the
// auto-mask), so LDS does not grow with S; best, winner and Imin of a thread's four pixels stay in registers.
//
//   min_partials   stages y = tgt of the tile and a one-pixel halo once (18 x 66, every channel), then per
//                  source x = warp(src_s) and a validity byte of the same region, a barrier, E_s of the
//                  thread's four pixels from LDS and the replacement test; with auto-masking the same region
//                  again with x = src_s unwarped and every pixel of the image valid. Writes the winner byte
//                  plane (s, 254 masked, 255 none) into the workspace, which the backward reads instead of
//                  recomputing S error maps, and the optional winner and error planes; per tile the fp32 sum
//                  of the kept pixels' best (photo_partials' order) and the counts of pixels with a winner and
//                  of masked ones
//   min_finalize   one block: a wave per image sums its tiles (image_tile_sums<1>; the counts in integers),
//                  thread 0 adds the images in order and writes n_c, n_m and L
//   min_grad       stages y and the winner bytes of the tile and a two-pixel halo once (20 x 68), then per
//                  source x and validity, per channel a, b, c of the 18 x 66 windows that source won (LDS
//                  reused by the channels and the sources) and the gathers, as ssim_grad; the thread's four
//                  g_depth accumulate in registers over the sources. Nothing per-pixel but the winner byte,
//                  g_depth and the optional planes reaches memory
//
// Static LDS: min_partials<3> 29.8 KB (ssim_partials'), min_grad<3> 49.7 KB (ssim_grad's and the 1.4 KB of
// winner bytes), both below 64 KB and independent of S. The image comes from blockIdx alone and the source
// index is uniform, so K, m and the planes' buffer resources stay wave-uniform; an invalid pixel loads no tap;
// no byte outside a view is read. No atomics, no host synchronisation, no allocation: capturable, the same
// bits on every run.
#include "ssim_common.h"

namespace nconv {

namespace {

constexpr int kMinF = 1024;                 // finalize: sixteen waves, one image each at a time
constexpr unsigned char kMasked = 254, kNone = 255;

// the workspace: n_c, n_m first (the backward and the caller read them there)
struct MinWs {
    int* n;                 // [2]: n_c, n_m
    double* img;            // [B]
    int* icnt;              // [B][2]
    float* part;            // [B * tiles]
    int* cnt;               // [B * tiles][2]
    unsigned char* winner;  // [B][H][W]
};
__host__ __device__ MinWs min_ws(void* ws, int B, int tiles) {
    MinWs p;
    p.n = (int*)ws;
    p.img = (double*)(p.n + 2);
    p.icnt = (int*)(p.img + B);
    p.part = (float*)(p.icnt + 2 * (size_t)B);
    p.cnt = (int*)(p.part + (size_t)B * tiles);
    p.winner = (unsigned char*)(p.cnt + 2 * (size_t)B * tiles);
    return p;
}

// y of region pixel idx (every pixel of the image, whatever a source's validity)
template <int C, int RW, int RN>
__device__ __forceinline__ void stage_target(const WarpArgs& a, int b, int i0, int j0, int idx, float (&sy)[C][RN]) {
    const int i = i0 + idx / RW, j = j0 + idx % RW;
    const bool inside = i >= 0 && i < a.H && j >= 0 && j < a.W;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) sy[ch][idx] = tgt_load(a, b, ch, i, j, inside);
}

// x = warp(src) and validity of region pixel idx
template <int C, int RW, int RN>
__device__ __forceinline__ void stage_warped(const WarpArgs& a, const Camera& cam, const Proj& q, int b, int i0,
                                             int j0, int idx, float (&sx)[C][RN], unsigned char (&sv)[RN]) {
    const int i = i0 + idx / RW, j = j0 + idx % RW;
    const bool inside = i >= 0 && i < a.H && j >= 0 && j < a.W;
    const Geo g = warp_geometry(a, cam, q, b, i, j, inside);
#pragma unroll
    for (int ch = 0; ch < C; ++ch) sx[ch][idx] = warp_sample(a, g, b, ch).s;
    sv[idx] = g.ok ? 1 : 0;
}

// x = src unwarped (Hs == H, Ws == W), every pixel of the image valid
template <int C, int RW, int RN>
__device__ __forceinline__ void stage_identity(const WarpArgs& a, int b, int i0, int j0, int idx, float (&sx)[C][RN],
                                               unsigned char (&sv)[RN]) {
    const int i = i0 + idx / RW, j = j0 + idx % RW;
    const bool inside = i >= 0 && i < a.H && j >= 0 && j < a.W;
    const unsigned off = inside ? (unsigned)((long long)i * a.src.rs + j) * 4u : kOOB;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        const __amdgpu_buffer_rsrc_t rs =
            plane_rsrc(a.src.image<float>(b) + (long long)ch * a.scs, view_bytes(a.Hs, a.src.rs, a.Ws, 4));
        sx[ch][idx] = ld_f32(rs, off);
    }
    sv[idx] = inside ? 1 : 0;
}

// E of the pixel at `at` of the forward's region, and whether the pixel is comparable
template <int C>
__device__ __forceinline__ float pixel_error(const float (&sx)[C][kFN], const float (&sy)[C][kFN],
                                             const unsigned char (&sv)[kFN], int at, float alpha, float c1, float c2,
                                             bool& comparable) {
#pragma clang fp contract(off)
    float term = 0.f, termw = 0.f;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        const float e = fabsf(sx[ch][at] - sy[ch][at]);
        term = ch == 0 ? e : term + e;
    }
    if (alpha == 0.f) {  // no window quantity is formed
        comparable = sv[at] != 0;
        return term;
    }
    comparable = window_valid<kFW>(sv, at);
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        const float ew = ssim_term(ssim_window<kFW>(sx[ch], sy[ch], at, c1, c2));
        termw = ch == 0 ? ew : termw + ew;
    }
    const float pw = alpha * termw, pv = (1.0f - alpha) * term;
    return pw + pv;
}

// the replacement rule of the minimum: the first, a smaller one, or a NaN over a number
__device__ __forceinline__ bool replaces(bool has, float e, float best) {
    return !has || e < best || (e != e && best == best);
}

// one workgroup per tile; part[tile], cnt[2 tile + k], k = 0: n_c, 1: n_m
template <int C>
__global__ __launch_bounds__(kWT) void min_partials(MinArgs m, unsigned char* __restrict__ wplane,
                                                    unsigned char* __restrict__ winner, float* __restrict__ error,
                                                    float* __restrict__ part, int* __restrict__ cnt) {
#pragma clang fp contract(off)
    __shared__ float sx[C][kFN], sy[C][kFN];
    __shared__ unsigned char sv[kFN];
    __shared__ float red[kWT / 64];
    __shared__ int redc[2][kWT / 64];
    const WarpArgs& a0 = m.v[0];
    const int H = a0.H, W = a0.W;
    const TileOrigin o = tile_origin<kLossTH, kLossTW>(H, W);
    const Camera cam = warp_camera(a0, o.b);
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll 1
    for (int idx = threadIdx.x; idx < kFN; idx += kWT) stage_target<C, kFW, kFN>(a0, o.b, o.i0 - 1, o.j0 - 1, idx, sy);
    float best[kWRows], imin[kWRows];
    int win[kWRows];
    bool hasi[kWRows];
#pragma unroll
    for (int r = 0; r < kWRows; ++r) best[r] = 0.f, imin[r] = 0.f, win[r] = -1, hasi[r] = false;
#pragma unroll 1
    for (int s = 0; s < m.S; ++s) {
        const WarpArgs& a = m.v[s];
        const Proj q = proj_of(a, o.b);
#pragma unroll 1
        for (int pass = 0; pass <= m.automask; ++pass) {
            __syncthreads();  // the region of the pass before has been read
            if (pass == 0) {
#pragma unroll 1
                for (int idx = threadIdx.x; idx < kFN; idx += kWT)
                    stage_warped<C, kFW, kFN>(a, cam, q, o.b, o.i0 - 1, o.j0 - 1, idx, sx, sv);
            } else {
#pragma unroll 1
                for (int idx = threadIdx.x; idx < kFN; idx += kWT)
                    stage_identity<C, kFW, kFN>(a, o.b, o.i0 - 1, o.j0 - 1, idx, sx, sv);
            }
            __syncthreads();
#pragma unroll 1
            for (int r = 0; r < kWRows; ++r) {
                const int at = (w + r * (kWT / 64) + 1) * kFW + lane + 1;
                bool comparable;
                const float e = pixel_error<C>(sx, sy, sv, at, m.alpha, m.c1, m.c2, comparable);
#pragma unroll
                for (int k = 0; k < kWRows; ++k) {  // static indices: the four pixels' state stays in registers
                    if (k != r || !comparable) continue;
                    if (pass == 0) {
                        if (replaces(win[k] >= 0, e, best[k])) best[k] = e, win[k] = s;
                    } else {
                        if (replaces(hasi[k], e, imin[k])) imin[k] = e, hasi[k] = true;
                    }
                }
            }
        }
    }
    const size_t plane = (size_t)H * W;
    float sum = 0.f;
    int nc = 0, nm = 0;
#pragma unroll
    for (int r = 0; r < kWRows; ++r) {
        const int i = o.i0 + w + r * (kWT / 64), j = o.j0 + lane;
        const bool has = win[r] >= 0;
        const bool masked = has && hasi[r] && imin[r] <= best[r];  // a NaN on either side: not masked
        const bool kept = has && !masked;
        sum += kept ? best[r] : 0.f;
        nc += has ? 1 : 0;
        nm += masked ? 1 : 0;
        if (i < H && j < W) {
            const size_t at = (size_t)o.b * plane + (size_t)i * W + j;
            const unsigned char code = !has ? kNone : masked ? kMasked : (unsigned char)win[r];
            wplane[at] = code;
            if (winner) winner[at] = code;
            if (error) error[at] = kept ? best[r] / (float)C : 0.f;
        }
    }
    sum = wave_sum(sum), nc = wave_sum(nc), nm = wave_sum(nm);
    if (lane == 0) red[w] = sum, redc[0][w] = nc, redc[1][w] = nm;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = waves_in_order(red);
    if (threadIdx.x < 2) cnt[2 * (size_t)blockIdx.x + threadIdx.x] = waves_in_order(redc[threadIdx.x]);
}

// One block. Wave w reduces images w, w + 16, .. (image_tile_sums<1>; the counts likewise in integers).
// After the barrier thread 0 adds the images in order and writes n_c, n_m and
// L = (float)(sum / ((double)C * (double)max(n_c, 1))).
__global__ __launch_bounds__(kMinF) void min_finalize(const float* __restrict__ part, const int* __restrict__ cnt,
                                                      int B, int tiles, int C, double* __restrict__ img,
                                                      int* __restrict__ icnt, int* __restrict__ n_out,
                                                      float* __restrict__ loss) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int b = w; b < B; b += kMinF / 64) {
        const int* cb = cnt + 2 * (size_t)b * tiles;
        double s[1];
        image_tile_sums(part + (size_t)b * tiles, tiles, lane, s);
        int nc = 0, nm = 0;
        for (int t = lane; t < tiles; t += 64) nc += cb[2 * t], nm += cb[2 * t + 1];
        nc = wave_sum(nc), nm = wave_sum(nm);
        if (lane == 0) img[b] = s[0], icnt[2 * b] = nc, icnt[2 * b + 1] = nm;
    }
    __syncthreads();  // img and icnt written by this block's waves
    if (threadIdx.x == 0) {
        double acc = 0.0;
        int nc = 0, nm = 0;
        for (int b = 0; b < B; ++b) acc += img[b], nc += icnt[2 * b], nm += icnt[2 * b + 1];
        n_out[0] = nc, n_out[1] = nm;
        loss[0] = (float)(acc / ((double)C * (double)max(nc, 1)));
    }
}

template <int C>
__global__ __launch_bounds__(kWT) void min_grad(MinArgs m, const float* __restrict__ gloss,
                                                const int* __restrict__ n, const unsigned char* __restrict__ wplane,
                                                float* __restrict__ g_depth) {
#pragma clang fp contract(off)
    __shared__ float sx[C][kGN], sy[C][kGN];
    __shared__ unsigned char sv[kGN], sw[kGN];
    __shared__ float wa[kFN], wb[kFN], wc[kFN];
    const WarpArgs& a0 = m.v[0];
    const int H = a0.H, W = a0.W;
    const TileOrigin o = tile_origin<kLossTH, kLossTW>(H, W);
    const Camera cam = warp_camera(a0, o.b);
    const size_t plane = (size_t)H * W;
    const float alpha = m.alpha;
#pragma unroll 1
    for (int idx = threadIdx.x; idx < kGN; idx += kWT) {
        stage_target<C, kGW, kGN>(a0, o.b, o.i0 - 2, o.j0 - 2, idx, sy);
        const int i = o.i0 - 2 + idx / kGW, j = o.j0 - 2 + idx % kGW;
        const bool inside = i >= 0 && i < H && j >= 0 && j < W;
        sw[idx] = inside ? wplane[(size_t)o.b * plane + (size_t)i * W + j] : kNone;
    }
    const float gl = gloss ? gloss[0] : 1.f;
    const float den = (float)C * (float)max(n[0], 1);
    const float inv = 1.0f / den;
    const float kl = (gl * (1.0f - alpha)) * inv;  // the L1 part's factor
    const float kw = gl * inv;
    const float kq = (alpha * 0.5f) * kw;          // the SSIM part's
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float acc_d[kWRows];
#pragma unroll
    for (int r = 0; r < kWRows; ++r) acc_d[r] = 0.f;
#pragma unroll 1
    for (int s = 0; s < m.S; ++s) {
        const WarpArgs& a = m.v[s];
        const Proj q = proj_of(a, o.b);
        if (alpha != 0.f) {
            __syncthreads();  // y and the winner bytes staged (s == 0); the source before has been read
#pragma unroll 1
            for (int idx = threadIdx.x; idx < kGN; idx += kWT)
                stage_warped<C, kGW, kGN>(a, cam, q, o.b, o.i0 - 2, o.j0 - 2, idx, sx, sv);
#pragma unroll 1
            for (int ch = 0; ch < C; ++ch) {
                __syncthreads();  // x and validity staged (ch == 0); a, b, c of the channel before gathered
#pragma unroll 1
                for (int idx = threadIdx.x; idx < kFN; idx += kWT) {
                    const int at = (idx / kFW + 1) * kGW + idx % kFW + 1;  // the window's centre in the 20 x 68 region
                    const Ssim ss = ssim_window<kGW>(sx[ch], sy[ch], at, m.c1, m.c2);
                    // kept and won by this source (so it has a window), and the channel passes
                    const bool pass = sw[at] == s && window_valid<kGW>(sv, at) && ss.t >= 0.f && ss.t <= 1.f;
                    const SsimCoef k = ssim_coef(ss);
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
        } else if (s == 0) {
            __syncthreads();  // y and the winner bytes staged
        }
#pragma unroll 1
        for (int r = 0; r < kWRows; ++r) {
            const int ti = w + r * (kWT / 64);
            const int i = o.i0 + ti, j = o.j0 + lane;
            const bool inside = i < H && j < W;
            const Geo g = warp_geometry(a, cam, q, o.b, i, j, inside);
            float du, dv;
            warp_duv(cam, q, g, i, j, du, dv);
            const int own = (ti + 2) * kGW + lane + 2;
            const bool won = sw[own] == s;
            float acc = 0.f;
#pragma unroll
            for (int ch = 0; ch < C; ++ch) {
                const Sample p = warp_sample(a, g, o.b, ch);
                const float d = p.s - sy[ch][own];
                const float sg = d > 0.f ? 1.f : d < 0.f ? -1.f : 0.f;
                const float l1 = won ? kl * sg : 0.f;
                const float gx = alpha != 0.f ? sx[ch][own] : 0.f;
                const float gs = l1 + gx;
                const float term = warp_gterm(g, p, gs, du, dv);
                acc = ch == 0 ? term : acc + term;
            }
            const float t = g.ok ? acc : 0.f;
#pragma unroll
            for (int k = 0; k < kWRows; ++k)  // static indices: the four sums stay in registers
                if (k == r) acc_d[k] = s == 0 ? t : acc_d[k] + t;
        }
    }
#pragma unroll
    for (int r = 0; r < kWRows; ++r) {
        const int i = o.i0 + w + r * (kWT / 64), j = o.j0 + lane;
        if (i < H && j < W) g_depth[(size_t)o.b * plane + (size_t)i * W + j] = acc_d[r];
    }
}

}  // namespace

size_t photo_min_workspace_bytes(int B, int H, int W) {
    // min_ws: n_c and n_m, img, icnt, part, cnt, the winner bytes; rounded up to 8
    const size_t tiles = (size_t)B * loss_tiles_per_image(H, W);
    const size_t bytes = 8 + (size_t)B * 8 + (size_t)B * 8 + tiles * 4 + tiles * 8 + (size_t)B * H * W;
    return (bytes + 7) & ~(size_t)7;
}

int launch_photo_min_loss_fwd(const MinArgs& m, float* loss, unsigned char* winner, float* error, void* ws,
                              hipStream_t st, const char** why) {
    const WarpArgs& a = m.v[0];
    const int tiles = loss_tiles_per_image(a.H, a.W);
    const MinWs p = min_ws(ws, a.B, tiles);
    const dim3 g(a.B * tiles), t(kWT);
    if (a.C == 1)
        hipLaunchKernelGGL(min_partials<1>, g, t, 0, st, m, p.winner, winner, error, p.part, p.cnt);
    else
        hipLaunchKernelGGL(min_partials<3>, g, t, 0, st, m, p.winner, winner, error, p.part, p.cnt);
    hipLaunchKernelGGL(min_finalize, dim3(1), dim3(kMinF), 0, st, p.part, p.cnt, a.B, tiles, a.C, p.img, p.icnt, p.n,
                       loss);
    return launch_status(why);
}

int launch_photo_min_loss_bwd(const MinArgs& m, const float* gloss, const void* ws, float* g_depth, hipStream_t st,
                              const char** why) {
    const WarpArgs& a = m.v[0];
    const int tiles = loss_tiles_per_image(a.H, a.W);
    const MinWs p = min_ws(const_cast<void*>(ws), a.B, tiles);
    const dim3 g(a.B * tiles), t(kWT);
    if (a.C == 1)
        hipLaunchKernelGGL(min_grad<1>, g, t, 0, st, m, gloss, p.n, p.winner, g_depth);
    else
        hipLaunchKernelGGL(min_grad<3>, g, t, 0, st, m, gloss, p.n, p.winner, g_depth);
    return launch_status(why);
}

}  // namespace nconv
