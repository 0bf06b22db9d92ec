// warp_common.h — the per-pixel pieces of the depth-driven view warp, shared by view_warp.hip (the warp, its
// gradient, the L1 photometric loss), photo_ssim.hip (the SSIM + L1 loss) and photo_min.hip (its minimum over
// several sources): the projection of a target
// pixel into the source frame, its four taps and their blend, the derivatives of that with respect to the
// depth, and the thread map of the 16 x 64 tile. The rule is stated operation by operation in
// include/nconv.h (nconv_view_warp_*); every operation here is fp32 in that order, no contraction.
//
// The image comes from blockIdx alone, so its K and m are read from wave-uniform addresses (scalar loads,
// scalar registers) and the buffer resources of its planes are scalar too. An invalid pixel loads no tap
// (its loads are aimed at plane_io.h's kOOB); a valid one reads taps inside [0, Hs - 1] x [0, Ws - 1] by
// the clamps, so no byte outside a view's extent is read.
#pragma once
#include "backproject_common.h"

namespace nconv {

constexpr int kWT = 256;                      // threads: four waves
constexpr int kWRows = kLossTH / (kWT / 64);  // rows of the tile (plane_io.h's 16 x 64) per thread

struct Proj {
    float r[3][4];
};
__device__ __forceinline__ Proj proj_of(const WarpArgs& a, int b) {
    const float* m = a.m + (long long)b * a.mbs;
    Proj q;
#pragma unroll
    for (int k = 0; k < 12; ++k) q.r[k / 4][k % 4] = m[k];
    return q;
}
__device__ __forceinline__ Camera warp_camera(const WarpArgs& a, int b) {
    const float* k = a.k + (long long)b * a.kbs;
    return Camera{k[0], k[4], k[2], k[5]};
}

// ((r0 * x + r1 * y) + r2 * z) + r3: five roundings, no fused multiply-add (lidar_project.hip's dot)
__device__ __forceinline__ float warp_dot(const float (&r)[4], float x, float y, float z) {
#pragma clang fp contract(off)
    const float p0 = r[0] * x, p1 = r[1] * y, p2 = r[2] * z;
    const float s01 = p0 + p1;
    const float s012 = s01 + p2;
    return s012 + r[3];
}

// where a thread works: image b, column j, rows i0 + 4 r (r = 0 .. 3)
struct WarpTile {
    int b, i0, j;
};
__device__ __forceinline__ WarpTile warp_tile(const WarpArgs& a) {
    const TileOrigin o = tile_origin<kLossTH, kLossTW>(a.H, a.W);
    return WarpTile{o.b, o.i0 + (int)(threadIdx.x >> 6), o.j0 + (int)(threadIdx.x & 63)};
}

// the projection of one target pixel: validity, the coordinates, the weights and the taps' byte offsets.
// inside: (i, j) lies in the target plane (a pixel outside it reads nothing and is not valid)
struct Geo {
    bool ok;
    float u, v, c;
    float wu, w0u, wv, w0v;
    unsigned o00, o01, o10, o11;
};
__device__ __forceinline__ Geo warp_geometry(const WarpArgs& a, const Camera& cam, const Proj& q, int b, int i, int j,
                                             bool inside) {
#pragma clang fp contract(off)
    Geo g;
    const __amdgpu_buffer_rsrc_t rd = plane_rsrc(a.depth.image<float>(b), view_bytes(a.H, a.depth.rs, a.W, 4));
    const float z = ld_f32(rd, inside ? (unsigned)((long long)i * a.depth.rs + j) * 4u : kOOB);
    bool ok = inside && z > a.z_min && z <= a.z_max;
    if (a.mask.base) {
        const __amdgpu_buffer_rsrc_t rm =
            bytes_rsrc(a.mask.image<unsigned char>(b), view_bytes(a.H, a.mask.rs, a.W, 1));
        ok = ok && (ld_u8(rm, inside ? (unsigned)((long long)i * a.mask.rs + j) : kOOB) & 0xffu) != 0u;
    }
    float x, y;
    project(cam, i, j, z, x, y);
    const float pa = warp_dot(q.r[0], x, y, z), pb = warp_dot(q.r[1], x, y, z), pc = warp_dot(q.r[2], x, y, z);
    g.c = pc;
    g.u = pa / pc;
    g.v = pb / pc;
    // float comparisons before any conversion: NaN, infinities and huge coordinates are not valid
    const float wmax = (float)(a.Ws - 1), hmax = (float)(a.Hs - 1);
    ok = ok && pc > 0.f && g.u >= 0.f && g.u <= wmax && g.v >= 0.f && g.v <= hmax;
    g.ok = ok;
    const float u = ok ? g.u : 0.f, v = ok ? g.v : 0.f;  // an invalid pixel converts 0
    const float fu = floorf(u), fv = floorf(v);
    const int j0 = (int)fu, i0 = (int)fv;
    const int j1 = min(j0 + 1, a.Ws - 1), i1 = min(i0 + 1, a.Hs - 1);
    g.wu = u - fu, g.wv = v - fv;
    g.w0u = 1.0f - g.wu, g.w0v = 1.0f - g.wv;
    const long long r0 = (long long)i0 * a.src.rs, r1 = (long long)i1 * a.src.rs;
    g.o00 = (unsigned)(r0 + j0) * 4u, g.o01 = (unsigned)(r0 + j1) * 4u;
    g.o10 = (unsigned)(r1 + j0) * 4u, g.o11 = (unsigned)(r1 + j1) * 4u;
    return g;
}

// the four taps of channel ch (0 where the pixel is not valid: nothing is read) and their blend
struct Sample {
    float a00, a01, a10, a11, top, bot, s;
};
__device__ __forceinline__ Sample warp_sample(const WarpArgs& a, const Geo& g, int b, int ch) {
#pragma clang fp contract(off)
    const __amdgpu_buffer_rsrc_t rs =
        plane_rsrc(a.src.image<float>(b) + (long long)ch * a.scs, view_bytes(a.Hs, a.src.rs, a.Ws, 4));
    Sample p;
    p.a00 = ld_f32(rs, g.ok ? g.o00 : kOOB);
    p.a01 = ld_f32(rs, g.ok ? g.o01 : kOOB);
    p.a10 = ld_f32(rs, g.ok ? g.o10 : kOOB);
    p.a11 = ld_f32(rs, g.ok ? g.o11 : kOOB);
    const float t0 = g.w0u * p.a00, t1 = g.wu * p.a01;
    p.top = t0 + t1;
    const float b0 = g.w0u * p.a10, b1 = g.wu * p.a11;
    p.bot = b0 + b1;
    const float s0 = g.w0v * p.top, s1 = g.wv * p.bot;
    p.s = s0 + s1;
    return p;
}

// d u / d z and d v / d z of the pixel
__device__ __forceinline__ void warp_duv(const Camera& cam, const Proj& q, const Geo& g, int i, int j, float& du,
                                         float& dv) {
#pragma clang fp contract(off)
    const float X = ((float)j - cam.cx) / cam.fx, Y = ((float)i - cam.cy) / cam.fy;
    float d[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float p0 = q.r[r][0] * X, p1 = q.r[r][1] * Y;
        const float s01 = p0 + p1;
        d[r] = s01 + q.r[r][2];
    }
    const float uc = g.u * d[2], vc = g.v * d[2];
    const float nu = d[0] - uc, nv = d[1] - vc;
    du = nu / g.c;
    dv = nv / g.c;
}

// g_s (dIu du + dIv dv) of one channel
__device__ __forceinline__ float warp_gterm(const Geo& g, const Sample& p, float gs, float du, float dv) {
#pragma clang fp contract(off)
    const float d0 = p.a01 - p.a00, d1 = p.a11 - p.a10;
    const float e0 = g.w0v * d0, e1 = g.wv * d1;
    const float dIu = e0 + e1;
    const float dIv = p.bot - p.top;
    const float f0 = dIu * du, f1 = dIv * dv;
    const float f = f0 + f1;
    return gs * f;
}

__device__ __forceinline__ float tgt_load(const WarpArgs& a, int b, int ch, int i, int j, bool inside) {
    const __amdgpu_buffer_rsrc_t rt =
        plane_rsrc(a.tgt.image<float>(b) + (long long)ch * a.tcs, view_bytes(a.H, a.tgt.rs, a.W, 4));
    return ld_f32(rt, inside ? (unsigned)((long long)i * a.tgt.rs + j) * 4u : kOOB);
}

}  // namespace nconv
