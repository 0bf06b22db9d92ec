// smooth_loss.hip — the edge-aware smoothness penalty on the predicted depth that the photometric term
// (view_warp.hip) is trained with: the L1 of the depth's first differences relaxed by an image-edge weight
// (monodepth, order 1) or of its second differences (Ma, Cavalheiro, Karaman, ICRA 2019, order 2), its
// gradient with respect to the depth, and the edge weights exp(-alpha |dI|) of a frame. The rule is stated
// operation by operation in include/nconv.h (nconv_smooth_loss_*, nconv_edge_weights); every operation
// here is fp32 in that order, no contraction.
//
// A term lies along a direction (x: along a row, y: down a column) and is centred on a pixel p:
//   order 1   c = M(p) && M(p + 1)               t = d[p + 1] - d[p]                   w = w_dir(p)
//   order 2   c = M(p - 1) && M(p) && M(p + 1)   t = (d[p - 1] + d[p + 1]) - 2 d[p]    w = min(w_dir(p - 1), w_dir(p))
// M is the mask inside the plane and false outside it, which is what ends the terms at the image edge.
//   s = c ? w |t| : 0          q = c ? (k w) sign(t) : +0
//
// One workgroup of 256 threads per 16 x 64 tile of one image (the loss's tile, view_warp.hip's thread
// map): a wave's 64 lanes lie along a row, a thread takes rows w, w + 4, w + 8, w + 12 of the tile.
//
//   smooth_partials   per tile: the fp32 sums of its 1024 x terms and of its 1024 y terms (a thread's four in
//                     row order, then wave_ops.h's wave_sum and waves_in_order) and the counts of cx and cy
//   smooth_finalize   one block: a wave per image sums its tiles (image_tile_sums<2>; the counts in
//                     integers), thread 0 adds the images in order and writes n_x, n_y and L
//   smooth_grad       g_depth: every pixel gathers the q of the terms it takes part in (four for order 1,
//                     six for order 2) from the depth around it, with kx, ky from the device's counts
//   edge_weights      wx, wy of a frame of one or three channels
//
// The stencils are read through the cache, not staged in LDS: a pixel of the gradient reads d at distance
// up to 1 (order 1) or 2 (order 2) along each axis, every one of those a neighbouring lane's or a
// neighbouring row's own pixel, so a wave's loads of one offset are one contiguous 256-byte row segment
// that the wave itself or the next one has just brought in. Every load goes through a buffer resource
// over exactly the image's extent and is aimed at plane_io.h's kOOB where its pixel is outside the
// plane, so no byte outside a view is read. No atomics, no host synchronisation, no allocation:
// capturable, and the same bits on every run.
#include "nconv_internal.h"

namespace nconv {

namespace {

constexpr int kST = 256;                      // threads: four waves
constexpr int kSRows = kLossTH / (kST / 64);  // rows of the tile per thread
constexpr int kSF = 1024;                     // finalize: sixteen waves, one image each at a time

// the workspace: n_x, n_y first (the backward and the caller read them there)
struct SmoothWs {
    int* n;        // [2]: n_x, n_y
    double* img;   // [B][2]: Sx, Sy of an image
    int* icnt;     // [B][2]
    float* part;   // [B * tiles][2]
    int* cnt;      // [B * tiles][2]
};
__host__ __device__ SmoothWs smooth_ws(void* ws, int B, int tiles) {
    SmoothWs p;
    p.n = (int*)ws;
    p.img = (double*)(p.n + 2);
    p.icnt = (int*)(p.img + 2 * (size_t)B);
    p.part = (float*)(p.icnt + 2 * (size_t)B);
    p.cnt = (int*)(p.part + 2 * (size_t)B * tiles);
    return p;
}

// where a thread works: image b, column j, rows i0 + 4 r (r = 0 .. 3)
struct SmoothTile {
    int b, i0, j;
};
__device__ __forceinline__ SmoothTile smooth_tile(int H, int W) {
    const TileOrigin o = tile_origin<kLossTH, kLossTW>(H, W);
    return SmoothTile{o.b, o.i0 + (int)(threadIdx.x >> 6), o.j0 + (int)(threadIdx.x & 63)};
}

// image b's planes as buffer resources, and the loads of one pixel of them
struct SmoothImage {
    __amdgpu_buffer_rsrc_t rd, rm, rw[2];
    int H, W;
    long long drs, mrs;
    bool masked;
};
template <bool HAS_W>
__device__ __forceinline__ SmoothImage smooth_image(const SmoothArgs& a, int b) {
    SmoothImage s;
    s.H = a.H, s.W = a.W, s.drs = a.depth.rs, s.mrs = a.mask.rs, s.masked = a.mask.base != nullptr;
    s.rd = plane_rsrc(a.depth.image<float>(b), view_bytes(a.H, a.depth.rs, a.W, 4));
    s.rm = bytes_rsrc(s.masked ? a.mask.image<unsigned char>(b) : nullptr, s.masked ? view_bytes(a.H, a.mask.rs, a.W, 1) : 0);
    const size_t plane = (size_t)a.H * a.W;
#pragma unroll
    for (int p = 0; p < 2; ++p)
        s.rw[p] = plane_rsrc(HAS_W ? a.w + ((size_t)b * 2 + p) * plane : nullptr, HAS_W ? (int)(plane * 4) : 0);
    return s;
}
__device__ __forceinline__ bool in_plane(const SmoothImage& s, int i, int j) {
    return i >= 0 && i < s.H && j >= 0 && j < s.W;
}
__device__ __forceinline__ float depth_at(const SmoothImage& s, int i, int j) {
    return ld_f32(s.rd, in_plane(s, i, j) ? (unsigned)((long long)i * s.drs + j) * 4u : kOOB);
}
// M: the mask inside the plane, false outside it
__device__ __forceinline__ bool mask_at(const SmoothImage& s, int i, int j) {
    const bool in = in_plane(s, i, j);
    if (!s.masked) return in;
    return in && (ld_u8(s.rm, in ? (unsigned)((long long)i * s.mrs + j) : kOOB) & 0xffu) != 0u;
}
// w_dir of the edge that starts at (i, j): the last column of wx and the last row of wy are not read
__device__ __forceinline__ float weight_at(const SmoothImage& s, int dir, int i, int j) {
    const bool in = i >= 0 && j >= 0 && i < s.H - (dir == 1) && j < s.W - (dir == 0);
    return ld_f32(s.rw[dir], in ? (unsigned)(i * s.W + j) * 4u : kOOB);
}

// the term of direction dir (0: x, 1: y) centred on (i, j)
struct Term {
    bool c;
    float t, w;
};
template <int ORDER, bool HAS_W>
__device__ __forceinline__ Term smooth_term(const SmoothImage& s, int dir, int i, int j) {
#pragma clang fp contract(off)
    const int di = dir, dj = 1 - dir;
    Term r;
    r.w = 1.f;
    if (ORDER == 1) {
        r.c = mask_at(s, i, j) && mask_at(s, i + di, j + dj);
        r.t = depth_at(s, i + di, j + dj) - depth_at(s, i, j);
        if (HAS_W) r.w = weight_at(s, dir, i, j);
    } else {
        r.c = mask_at(s, i - di, j - dj) && mask_at(s, i, j) && mask_at(s, i + di, j + dj);
        const float ends = depth_at(s, i - di, j - dj) + depth_at(s, i + di, j + dj);
        const float mid = 2.0f * depth_at(s, i, j);
        r.t = ends - mid;
        if (HAS_W) {
            const float w0 = weight_at(s, dir, i - di, j - dj), w1 = weight_at(s, dir, i, j);
            r.w = w1 < w0 ? w1 : w0;
        }
    }
    return r;
}
// s = c ? w |t| : 0
template <int ORDER, bool HAS_W>
__device__ __forceinline__ float smooth_s(const SmoothImage& s, int dir, int i, int j, int& n) {
#pragma clang fp contract(off)
    const Term r = smooth_term<ORDER, HAS_W>(s, dir, i, j);
    n += r.c ? 1 : 0;
    const float e = fabsf(r.t);
    const float v = HAS_W ? r.w * e : e;
    return r.c ? v : 0.f;
}
// q = c ? (k w) sign(t) : +0
template <int ORDER, bool HAS_W>
__device__ __forceinline__ float smooth_q(const SmoothImage& s, int dir, int i, int j, float k) {
#pragma clang fp contract(off)
    const Term r = smooth_term<ORDER, HAS_W>(s, dir, i, j);
    const float sg = r.t > 0.f ? 1.f : r.t < 0.f ? -1.f : 0.f;
    const float kw = HAS_W ? k * r.w : k;
    const float v = kw * sg;
    return r.c ? v : 0.f;
}

// one workgroup per tile; part[2 tile + dir] and cnt[2 tile + dir], the tiles of image b at b * tiles-per-image
template <int ORDER, bool HAS_W>
__global__ __launch_bounds__(kST) void smooth_partials(SmoothArgs a, float* __restrict__ part, int* __restrict__ cnt) {
#pragma clang fp contract(off)
    __shared__ float red[2][kST / 64];
    __shared__ int redc[2][kST / 64];
    const SmoothTile t = smooth_tile(a.H, a.W);
    const SmoothImage im = smooth_image<HAS_W>(a, t.b);
    float sx[kSRows], sy[kSRows];
    int nx = 0, ny = 0;
#pragma unroll
    for (int r = 0; r < kSRows; ++r) {
        const int i = t.i0 + r * (kST / 64);
        sx[r] = smooth_s<ORDER, HAS_W>(im, 0, i, t.j, nx);
        sy[r] = smooth_s<ORDER, HAS_W>(im, 1, i, t.j, ny);
    }
    float tx = ((sx[0] + sx[1]) + sx[2]) + sx[3], ty = ((sy[0] + sy[1]) + sy[2]) + sy[3];
    tx = wave_sum(tx), ty = wave_sum(ty), nx = wave_sum(nx), ny = wave_sum(ny);
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
        red[0][w] = tx, red[1][w] = ty, redc[0][w] = nx, redc[1][w] = ny;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        part[2 * (size_t)blockIdx.x + threadIdx.x] = waves_in_order(red[threadIdx.x]);
        cnt[2 * (size_t)blockIdx.x + threadIdx.x] = waves_in_order(redc[threadIdx.x]);
    }
}

// One block. Wave w reduces images w, w + 16, .. (image_tile_sums; the counts likewise in integers).
// After the barrier thread 0 adds the images in order and writes n_x, n_y and
// L = (float)(Sx / (double)max(n_x, 1) + Sy / (double)max(n_y, 1)).
__global__ __launch_bounds__(kSF) void smooth_finalize(const float* __restrict__ part, const int* __restrict__ cnt,
                                                       int B, int tiles, double* __restrict__ img,
                                                       int* __restrict__ icnt, int* __restrict__ n_out,
                                                       float* __restrict__ loss) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int b = w; b < B; b += kSF / 64) {
        const int* cb = cnt + 2 * (size_t)b * tiles;
        double s[2];
        image_tile_sums(part + 2 * (size_t)b * tiles, tiles, lane, s);
        int nx = 0, ny = 0;
        for (int t = lane; t < tiles; t += 64) nx += cb[2 * t], ny += cb[2 * t + 1];
        nx = wave_sum(nx), ny = wave_sum(ny);
        if (lane == 0) img[2 * b] = s[0], img[2 * b + 1] = s[1], icnt[2 * b] = nx, icnt[2 * b + 1] = ny;
    }
    __syncthreads();  // img and icnt written by this block's waves
    if (threadIdx.x == 0) {
        double ax = 0.0, ay = 0.0;
        int nx = 0, ny = 0;
        for (int b = 0; b < B; ++b) ax += img[2 * b], ay += img[2 * b + 1], nx += icnt[2 * b], ny += icnt[2 * b + 1];
        n_out[0] = nx, n_out[1] = ny;
        const double lx = ax / (double)max(nx, 1), ly = ay / (double)max(ny, 1);
        loss[0] = (float)(lx + ly);
    }
}

template <int ORDER, bool HAS_W>
__global__ __launch_bounds__(kST) void smooth_grad(SmoothArgs a, const float* __restrict__ gloss,
                                                   const int* __restrict__ n, float* __restrict__ g_depth) {
#pragma clang fp contract(off)
    const SmoothTile t = smooth_tile(a.H, a.W);
    const SmoothImage im = smooth_image<HAS_W>(a, t.b);
    const float gl = gloss ? gloss[0] : 1.f;
    const float ix = 1.0f / (float)max(n[0], 1), iy = 1.0f / (float)max(n[1], 1);
    const float kx = gl * ix, ky = gl * iy;
    const size_t plane = (size_t)a.H * a.W;
#pragma unroll
    for (int r = 0; r < kSRows; ++r) {
        const int i = t.i0 + r * (kST / 64), j = t.j;
        if (i >= a.H || j >= a.W) continue;
        float g;
        if (ORDER == 1) {
            const float qxm = smooth_q<1, HAS_W>(im, 0, i, j - 1, kx), qx0 = smooth_q<1, HAS_W>(im, 0, i, j, kx);
            const float qym = smooth_q<1, HAS_W>(im, 1, i - 1, j, ky), qy0 = smooth_q<1, HAS_W>(im, 1, i, j, ky);
            const float gx = qxm - qx0;
            const float gxy = gx + qym;
            g = gxy - qy0;
        } else {
            const float qxm = smooth_q<2, HAS_W>(im, 0, i, j - 1, kx), qx0 = smooth_q<2, HAS_W>(im, 0, i, j, kx);
            const float qxp = smooth_q<2, HAS_W>(im, 0, i, j + 1, kx);
            const float qym = smooth_q<2, HAS_W>(im, 1, i - 1, j, ky), qy0 = smooth_q<2, HAS_W>(im, 1, i, j, ky);
            const float qyp = smooth_q<2, HAS_W>(im, 1, i + 1, j, ky);
            const float ex = qxm + qxp, mx = 2.0f * qx0;
            const float gx = ex - mx;
            const float ey = qym + qyp, my = 2.0f * qy0;
            const float gxy = gx + ey;
            g = gxy - my;
        }
        g_depth[(size_t)t.b * plane + (size_t)i * a.W + j] = g;
    }
}

// E(x) of include/nconv.h: exp(-x) for x >= 0 by 2^(n - y) 2^(-n), y = x log2(e), n = rint(y)
__device__ __forceinline__ float edge_exp(float x) {
#pragma clang fp contract(off)
    const float y0 = x * 1.44269504f;
    const float y = y0 < 126.0f ? y0 : 126.0f;  // a NaN or huge argument ends at 126: flushed below
    const float n = rintf(y);
    const float r = n - y;  // exact, in [-0.5, 0.5]
    float p = 0.000154035297f;
    p = p * r, p = p + 0.00133335579f;
    p = p * r, p = p + 0.00961812865f;
    p = p * r, p = p + 0.0555041097f;
    p = p * r, p = p + 0.240226507f;
    p = p * r, p = p + 0.693147182f;
    p = p * r, p = p + 1.0f;
    const int ni = (int)n;                                                 // 0 .. 126
    const float scale = __builtin_bit_cast(float, (127 - min(ni, 125)) << 23);  // 2^-ni, a normal number
    const float e = p * scale;                                             // exact
    return n > 125.0f ? 0.f : e;
}

template <int C>
__global__ __launch_bounds__(kST) void edge_weights(EdgeArgs a, float* __restrict__ w) {
#pragma clang fp contract(off)
    const SmoothTile t = smooth_tile(a.H, a.W);
    const size_t plane = (size_t)a.H * a.W;
    const int bytes = view_bytes(a.H, a.img.rs, a.W, 4);
#pragma unroll
    for (int r = 0; r < kSRows; ++r) {
        const int i = t.i0 + r * (kST / 64), j = t.j;
        const bool inside = i < a.H && j < a.W;
        const bool hx = inside && j + 1 < a.W, hy = inside && i + 1 < a.H;
        const unsigned o = (unsigned)((long long)i * a.img.rs + j) * 4u;
        float gx = 0.f, gy = 0.f;
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
            const __amdgpu_buffer_rsrc_t ri = plane_rsrc(a.img.image<float>(t.b) + (long long)ch * a.cs, bytes);
            const float v = ld_f32(ri, inside ? o : kOOB);
            const float vx = ld_f32(ri, hx ? o + 4u : kOOB);
            const float vy = ld_f32(ri, hy ? (unsigned)((long long)(i + 1) * a.img.rs + j) * 4u : kOOB);
            const float dx = fabsf(vx - v), dy = fabsf(vy - v);
            gx = ch == 0 ? dx : gx + dx;
            gy = ch == 0 ? dy : gy + dy;
        }
        if (C == 3) gx = gx / 3.0f, gy = gy / 3.0f;
        if (!inside) continue;
        const float ex = edge_exp(a.alpha * gx), ey = edge_exp(a.alpha * gy);
        float* wb = w + (size_t)t.b * 2 * plane + (size_t)i * a.W + j;
        wb[0] = hx ? ex : 1.0f;
        wb[plane] = hy ? ey : 1.0f;
    }
}

}  // namespace

size_t smooth_loss_workspace_bytes(int B, int H, int W) {
    // smooth_ws: n_x and n_y, img, icnt, part, cnt
    return 8 + (size_t)B * 16 + (size_t)B * 8 + (size_t)B * loss_tiles_per_image(H, W) * 16;
}

int launch_smooth_loss_fwd(const SmoothArgs& a, float* loss, void* ws, hipStream_t st, const char** why) {
    const int tiles = loss_tiles_per_image(a.H, a.W);
    const SmoothWs p = smooth_ws(ws, a.B, tiles);
    const dim3 g(a.B * tiles), t(kST);
    if (a.order == 1 && a.w) {
        hipLaunchKernelGGL((smooth_partials<1, true>), g, t, 0, st, a, p.part, p.cnt);
    } else if (a.order == 1) {
        hipLaunchKernelGGL((smooth_partials<1, false>), g, t, 0, st, a, p.part, p.cnt);
    } else if (a.w) {
        hipLaunchKernelGGL((smooth_partials<2, true>), g, t, 0, st, a, p.part, p.cnt);
    } else {
        hipLaunchKernelGGL((smooth_partials<2, false>), g, t, 0, st, a, p.part, p.cnt);
    }
    hipLaunchKernelGGL(smooth_finalize, dim3(1), dim3(kSF), 0, st, p.part, p.cnt, a.B, tiles, p.img, p.icnt, p.n, loss);
    return launch_status(why);
}

int launch_smooth_loss_bwd(const SmoothArgs& a, const float* gloss, const void* ws, float* g_depth, hipStream_t st,
                           const char** why) {
    const dim3 g(a.B * loss_tiles_per_image(a.H, a.W)), t(kST);
    const int* n = (const int*)ws;
    if (a.order == 1 && a.w) {
        hipLaunchKernelGGL((smooth_grad<1, true>), g, t, 0, st, a, gloss, n, g_depth);
    } else if (a.order == 1) {
        hipLaunchKernelGGL((smooth_grad<1, false>), g, t, 0, st, a, gloss, n, g_depth);
    } else if (a.w) {
        hipLaunchKernelGGL((smooth_grad<2, true>), g, t, 0, st, a, gloss, n, g_depth);
    } else {
        hipLaunchKernelGGL((smooth_grad<2, false>), g, t, 0, st, a, gloss, n, g_depth);
    }
    return launch_status(why);
}

int launch_edge_weights(const EdgeArgs& a, float* w, hipStream_t st, const char** why) {
    const dim3 g(a.B * loss_tiles_per_image(a.H, a.W)), t(kST);
    if (a.C == 1)
        hipLaunchKernelGGL(edge_weights<1>, g, t, 0, st, a, w);
    else
        hipLaunchKernelGGL(edge_weights<3>, g, t, 0, st, a, w);
    return launch_status(why);
}

}  // namespace nconv
