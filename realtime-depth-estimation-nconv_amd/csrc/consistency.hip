// consistency.hip — two views compared by their DEPTH: the geometric consistency check and fusion of MVSNet's
// filter_depth / COLMAP's fusion (project a target pixel into a neighbouring view, read that view's depth there,
// carry the point back, keep the pixel if it lands where it started at the depth it started with), and the
// geometry-consistency loss of SC-SfMLearner (Bian et al., NeurIPS 2019) with its gradient with respect to the
// target depth. The rule is stated operation by operation in include/nconv.h (nconv_depth_consistency,
// nconv_geo_consistency_loss_*); every operation here is fp32 in that order, no contraction.
//
// The projection, validity, taps, blend and their derivatives are warp_common.h's, bit for bit: a source is a
// nconv_view_warp whose src is the source's depth plane (C == 1). Per target pixel and source:
//   zs               the blend of the four depth taps; tvalid: every tap t > z_min && t <= z_max (a blend is never
//                    taken across a hole or a NaN)
//   xs, ys           ((u - cxs) * zs) / fxs, likewise y: the point in the source camera's frame
//   u2, v2, z2       m_back . (xs, ys, zs, 1), divided: the point carried back into the target view
//   cons             valid && tvalid && c2 > 0 && d2 <= px_tol^2 && |z2 - z| <= rel_tol z
//   loss             diff = |c - zs| / (c + zs) on valid && tvalid, its mean, and the gather that is its gradient
//
// One workgroup of 256 threads per 16 x 64 tile of one image (view_warp.hip's tile and thread map: lane =
// column, wave w owns rows w, w + 4, w + 8, w + 12). The image comes from blockIdx alone and the source index is
// uniform, so K, m, k_src, m_back and the planes' buffer resources stay wave-uniform. An invalid pixel loads no
// tap (its loads are aimed at plane_io.h's kOOB); no byte outside a view is read.
//
//   depth_consistency  one launch whatever S: the sources are a loop inside the kernel, acc, n and the bit mask of a
//                      thread's four pixels in registers; no LDS (each pixel owns its taps)
//   geo_partials       per tile the fp32 sum of its 1024 terms (photo_partials' order) and its count; the optional
//                      diff plane
//   geo_finalize       one block: a wave per image sums its tiles (image_tile_sums; the counts in integers), thread
//                      0 adds the images in order and writes n_g and L
//   geo_grad           g_depth, recomputing the geometry; kk from the device's n_g
//
// No atomics, no host synchronisation, no allocation: capturable, and the same bits on every run.
#include "warp_common.h"

namespace nconv {

namespace {

constexpr int kGF = 1024;  // finalize: sixteen waves, one image each at a time

// the loss's workspace: n_g first (the backward and the caller read it there); view_warp.hip's layout
struct GeoWs {
    int* n_g;       // [2]: the count and padding
    double* img;    // [B]
    int* icnt;      // [B rounded up to even]
    float* part;    // [B * tiles]
    int* cnt;       // [B * tiles]
};
__host__ __device__ GeoWs geo_ws(void* ws, int B, int tiles) {
    GeoWs p;
    p.n_g = (int*)ws;
    p.img = (double*)(p.n_g + 2);
    p.icnt = (int*)(p.img + B);
    p.part = (float*)(p.icnt + B + (B & 1));
    p.cnt = (int*)(p.part + (size_t)B * tiles);
    return p;
}

// the target pixel's own depth and its own test (warp_geometry's first step): z, and pvalid
__device__ __forceinline__ bool own_depth(const WarpArgs& a, int b, int i, int j, bool inside, float& z) {
    const __amdgpu_buffer_rsrc_t rd = plane_rsrc(a.depth.image<float>(b), view_bytes(a.H, a.depth.rs, a.W, 4));
    z = ld_f32(rd, inside ? (unsigned)((long long)i * a.depth.rs + j) * 4u : kOOB);
    bool ok = inside && z > a.z_min && z <= a.z_max;
    if (a.mask.base) {
        const __amdgpu_buffer_rsrc_t rm =
            bytes_rsrc(a.mask.image<unsigned char>(b), view_bytes(a.H, a.mask.rs, a.W, 1));
        ok = ok && (ld_u8(rm, inside ? (unsigned)((long long)i * a.mask.rs + j) : kOOB) & 0xffu) != 0u;
    }
    return ok;
}

// every tap is a depth: comparisons, so a NaN or the 0 of a hole is not
__device__ __forceinline__ bool taps_valid(const WarpArgs& a, const Sample& p) {
    const float lo = a.z_min, hi = a.z_max;
    return p.a00 > lo && p.a00 <= hi && p.a01 > lo && p.a01 <= hi && p.a10 > lo && p.a10 <= hi && p.a11 > lo &&
           p.a11 <= hi;
}

// c' = d c / d z of the pixel: warp_duv's d[2]
__device__ __forceinline__ float warp_dc(const Camera& cam, const Proj& q, int i, int j) {
#pragma clang fp contract(off)
    const float X = ((float)j - cam.cx) / cam.fx, Y = ((float)i - cam.cy) / cam.fy;
    const float p0 = q.r[2][0] * X, p1 = q.r[2][1] * Y;
    const float s01 = p0 + p1;
    return s01 + q.r[2][2];
}

__global__ __launch_bounds__(kWT) void depth_consistency(ConsistencyArgs m, float* __restrict__ fused,
                                                         unsigned char* __restrict__ count,
                                                         unsigned char* __restrict__ views,
                                                         float* __restrict__ reproj, float* __restrict__ reldiff) {
#pragma clang fp contract(off)
    const WarpArgs& a0 = m.v[0];
    const int H = a0.H, W = a0.W;
    const WarpTile t = warp_tile(a0);
    const Camera cam = warp_camera(a0, t.b);
    const size_t plane = (size_t)H * W;
    const float tol2 = m.px_tol * m.px_tol;
    float z[kWRows], acc[kWRows];
    bool pv[kWRows];
    int n[kWRows];
    unsigned bits[kWRows];
#pragma unroll
    for (int r = 0; r < kWRows; ++r) {
        const int i = t.i0 + r * (kWT / 64);
        pv[r] = own_depth(a0, t.b, i, t.j, i < H && t.j < W, z[r]);
        acc[r] = z[r], n[r] = 0, bits[r] = 0u;
    }
#pragma unroll 1
    for (int s = 0; s < m.S; ++s) {
        const WarpArgs& a = m.v[s];
        const Proj q = proj_of(a, t.b);
        const float* ks = m.k_src[s] + (long long)t.b * m.ksbs[s];
        const Camera cs{ks[0], ks[4], ks[2], ks[5]};
        const float* mb = m.m_back[s] + (long long)t.b * m.mbbs[s];
        Proj back;
#pragma unroll
        for (int k = 0; k < 12; ++k) back.r[k / 4][k % 4] = mb[k];
#pragma unroll
        for (int r = 0; r < kWRows; ++r) {
            const int i = t.i0 + r * (kWT / 64);
            const bool inside = i < H && t.j < W;
            const Geo g = warp_geometry(a, cam, q, t.b, i, t.j, inside);
            const Sample p = warp_sample(a, g, t.b, 0);
            const bool tv = taps_valid(a, p);
            const float zs = p.s;
            const float tu = g.u - cs.cx, tv_ = g.v - cs.cy;
            const float uz = tu * zs, vz = tv_ * zs;
            const float xs = uz / cs.fx, ys = vz / cs.fy;
            const float a2 = warp_dot(back.r[0], xs, ys, zs), b2 = warp_dot(back.r[1], xs, ys, zs),
                        c2 = warp_dot(back.r[2], xs, ys, zs);
            const float u2 = a2 / c2, v2 = b2 / c2;
            const float du = u2 - (float)t.j, dv = v2 - (float)i;
            const float du2 = du * du, dv2 = dv * dv;
            const float d2 = du2 + dv2;
            const float rz = fabsf(c2 - z[r]);
            const float lim = m.rel_tol * z[r];
            const bool seen = g.ok && tv && c2 > 0.f;
            const bool cons = seen && d2 <= tol2 && rz <= lim;
            const float sum = acc[r] + c2;
            acc[r] = cons ? sum : acc[r];
            n[r] += cons ? 1 : 0;
            bits[r] |= cons ? 1u << s : 0u;
            if (inside) {
                const size_t o = ((size_t)t.b * m.S + s) * plane + (size_t)i * W + t.j;
                if (reproj) reproj[o] = seen ? d2 : __builtin_inff();
                if (reldiff) reldiff[o] = seen ? rz / z[r] : __builtin_inff();
            }
        }
    }
#pragma unroll
    for (int r = 0; r < kWRows; ++r) {
        const int i = t.i0 + r * (kWT / 64);
        if (i >= H || t.j >= W) continue;
        const size_t o = (size_t)t.b * plane + (size_t)i * W + t.j;
        const float mean = acc[r] / (float)(n[r] + 1);
        if (fused) fused[o] = pv[r] && n[r] >= m.min_views ? mean : 0.f;
        if (count) count[o] = (unsigned char)n[r];
        if (views) views[o] = (unsigned char)bits[r];
    }
}

// one pixel of the loss: counted, c, zs and what the gradient needs of the taps
struct GeoTerm {
    bool ok;
    float num, den, diff;
};
__device__ __forceinline__ GeoTerm geo_term(const WarpArgs& a, const Geo& g, const Sample& p) {
#pragma clang fp contract(off)
    GeoTerm e;
    e.ok = g.ok && taps_valid(a, p);
    e.num = g.c - p.s;
    e.den = g.c + p.s;
    e.diff = fabsf(e.num) / e.den;
    return e;
}

// one workgroup per tile; part[tile] and cnt[tile], the tiles of image b at b * tiles-per-image
__global__ __launch_bounds__(kWT) void geo_partials(WarpArgs a, float* __restrict__ diff, float* __restrict__ part,
                                                    int* __restrict__ cnt) {
#pragma clang fp contract(off)
    __shared__ float red[kWT / 64];
    __shared__ int redc[kWT / 64];
    const WarpTile t = warp_tile(a);
    const Camera cam = warp_camera(a, t.b);
    const Proj q = proj_of(a, t.b);
    const size_t plane = (size_t)a.H * a.W;
    float s = 0.f;
    int n = 0;
#pragma unroll
    for (int r = 0; r < kWRows; ++r) {
        const int i = t.i0 + r * (kWT / 64);
        const bool inside = i < a.H && t.j < a.W;
        const Geo g = warp_geometry(a, cam, q, t.b, i, t.j, inside);
        const GeoTerm e = geo_term(a, g, warp_sample(a, g, t.b, 0));
        const float term = e.ok ? e.diff : 0.f;
        s += term;
        n += e.ok ? 1 : 0;
        if (diff && inside) diff[(size_t)t.b * plane + (size_t)i * a.W + t.j] = term;
    }
    s = wave_sum(s), n = wave_sum(n);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s, redc[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = waves_in_order(red), cnt[blockIdx.x] = waves_in_order(redc);
}

// One block. Wave w reduces images w, w + 16, .. (image_tile_sums; the counts likewise in integers). After the
// barrier thread 0 adds the images in order and writes n_g and L = (float)(sum / (double)max(n_g, 1)).
__global__ __launch_bounds__(kGF) void geo_finalize(const float* __restrict__ part, const int* __restrict__ cnt, int B,
                                                    int tiles, double* __restrict__ img, int* __restrict__ icnt,
                                                    int* __restrict__ n_g, float* __restrict__ loss) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int b = w; b < B; b += kGF / 64) {
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
        n_g[0] = n;
        loss[0] = (float)(acc / (double)max(n, 1));
    }
}

__global__ __launch_bounds__(kWT) void geo_grad(WarpArgs a, const float* __restrict__ gloss,
                                                const int* __restrict__ n_g, float* __restrict__ g_depth) {
#pragma clang fp contract(off)
    const WarpTile t = warp_tile(a);
    const Camera cam = warp_camera(a, t.b);
    const Proj q = proj_of(a, t.b);
    const float inv = 1.0f / (float)max(n_g[0], 1);
    const float kk = (gloss ? gloss[0] : 1.f) * inv;
    const size_t plane = (size_t)a.H * a.W;
#pragma unroll
    for (int r = 0; r < kWRows; ++r) {
        const int i = t.i0 + r * (kWT / 64);
        const bool inside = i < a.H && t.j < a.W;
        const Geo g = warp_geometry(a, cam, q, t.b, i, t.j, inside);
        if (!inside) continue;
        const Sample p = warp_sample(a, g, t.b, 0);
        const GeoTerm e = geo_term(a, g, p);
        float du, dv;
        warp_duv(cam, q, g, i, t.j, du, dv);
        const float dc = warp_dc(cam, q, i, t.j);
        const float dzs = warp_gterm(g, p, 1.f, du, dv);  // (dIu du) + (dIv dv); the product with 1 is exact
        const float sg = e.num > 0.f ? 1.f : e.num < 0.f ? -1.f : 0.f;
        const float lhs = (dc - dzs) * e.den, rhs = e.num * (dc + dzs);
        const float quot = (lhs - rhs) / (e.den * e.den);
        const float v = (kk * sg) * quot;
        g_depth[(size_t)t.b * plane + (size_t)i * a.W + t.j] = e.ok ? v : 0.f;
    }
}

}  // namespace

size_t geo_consistency_workspace_bytes(int B, int H, int W) {
    // geo_ws: n_g and padding, img, icnt (an even number of ints), part, cnt
    return 8 + (size_t)B * 8 + (size_t)(B + (B & 1)) * 4 + (size_t)B * loss_tiles_per_image(H, W) * 8;
}

int launch_depth_consistency(const ConsistencyArgs& m, float* fused, unsigned char* count, unsigned char* views,
                             float* reproj, float* reldiff, hipStream_t st, const char** why) {
    const WarpArgs& a = m.v[0];
    const dim3 g(a.B * loss_tiles_per_image(a.H, a.W)), t(kWT);
    hipLaunchKernelGGL(depth_consistency, g, t, 0, st, m, fused, count, views, reproj, reldiff);
    return launch_status(why);
}

int launch_geo_consistency_loss_fwd(const WarpArgs& a, float* loss, float* diff, void* ws, hipStream_t st,
                                    const char** why) {
    const int tiles = loss_tiles_per_image(a.H, a.W);
    const GeoWs p = geo_ws(ws, a.B, tiles);
    hipLaunchKernelGGL(geo_partials, dim3(a.B * tiles), dim3(kWT), 0, st, a, diff, p.part, p.cnt);
    hipLaunchKernelGGL(geo_finalize, dim3(1), dim3(kGF), 0, st, p.part, p.cnt, a.B, tiles, p.img, p.icnt, p.n_g, loss);
    return launch_status(why);
}

int launch_geo_consistency_loss_bwd(const WarpArgs& a, const float* gloss, const void* ws, float* g_depth,
                                    hipStream_t st, const char** why) {
    const dim3 g(a.B * loss_tiles_per_image(a.H, a.W)), t(kWT);
    hipLaunchKernelGGL(geo_grad, g, t, 0, st, a, gloss, (const int*)ws, g_depth);
    return launch_status(why);
}

}  // namespace nconv
