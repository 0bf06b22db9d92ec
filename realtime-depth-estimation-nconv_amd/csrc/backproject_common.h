// backproject_common.h — what backproject.hip and normals.hip share: the tiling (one wave per segment of
// 256 row pixels, four pixels per lane), the validity rule of a pixel and its 3-D point, each defined
// once. See backproject.hip for the definitions in words.
#pragma once
#include "nconv_internal.h"

namespace nconv {

constexpr int kBT = 256;                // threads: four waves, one segment each
constexpr int kSeg = 64 * 4;            // pixels per segment (four per lane)

struct Camera {
    float fx, fy, cx, cy;
};

// where a wave works: image b, row i, first pixel j of the lane, n = its pixels inside the row (<= 0: none)
struct Where {
    int s, b, i, j, n;
};

__device__ __forceinline__ bool segment_of_wave(const BackprojectArgs& a, Where& w) {
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    w.s = (int)blockIdx.x * (kBT / 64) + wave;
    if (w.s >= a.nseg) return false;
    const int nsw = (a.W + kSeg - 1) / kSeg, row = w.s / nsw;
    w.b = row / a.H;
    w.i = row - w.b * a.H;
    w.j = (w.s - row * nsw) * kSeg + (int)(threadIdx.x & 63) * 4;
    w.n = min(4, a.W - w.j);
    return true;
}

// the four fp32 of view v at the wave's place, the leading n of them (<= 0: none); the others, and all
// four where the row w.i is outside the plane (in_row false), read 0
__device__ __forceinline__ f4 view_load4(const BackprojectArgs& a, const PlaneView& v, const float* image,
                                         const Where& w, int n, bool in_row = true) {
    const __amdgpu_buffer_rsrc_t r = plane_rsrc(image, view_bytes(a.H, v.rs, a.W, 4));
    return load4_f32(r, v.wide != 0, in_row, n, (unsigned)((long long)w.i * v.rs + w.j) * 4u);
}

// the validity rule on the values of a pixel inside the image: comparisons, so a NaN is not valid
__device__ __forceinline__ bool depth_valid(const BackprojectArgs& a, float z) { return z > a.z_min && z <= a.z_max; }
__device__ __forceinline__ bool conf_valid(const BackprojectArgs& a, float c) { return c >= a.conf_min; }

// bit k: pixel j + k of row i is valid; z = the four depths (0 past the row, and in a row outside the
// plane: in_row false). Being inside the image is a mask of its own, not the 0 such a pixel reads.
__device__ __forceinline__ unsigned valid4(const BackprojectArgs& a, const Where& w, f4& z, bool in_row = true) {
    const unsigned inside = in_row && w.n > 0 ? (1u << w.n) - 1u : 0u;
    z = view_load4(a, a.depth, a.depth.image<float>(w.b), w, w.n, in_row);
    unsigned m = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) m |= (unsigned)depth_valid(a, z[k]) << k;
    m &= inside;
    if (a.conf.base) {
        const f4 c = view_load4(a, a.conf, a.conf.image<float>(w.b), w, w.n, in_row);
        unsigned mc = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) mc |= (unsigned)conf_valid(a, c[k]) << k;
        m &= mc;
    }
    return m;
}

// the same rule for the single pixel (i, j) of image b, which may lie outside the image (inside false:
// nothing is read, z = 0, not valid)
__device__ __forceinline__ bool valid1(const BackprojectArgs& a, int b, int i, int j, bool inside, float& z) {
    const __amdgpu_buffer_rsrc_t r = plane_rsrc(a.depth.image<float>(b), view_bytes(a.H, a.depth.rs, a.W, 4));
    z = ld_f32(r, inside ? (unsigned)((long long)i * a.depth.rs + j) * 4u : kOOB);
    bool ok = inside && depth_valid(a, z);
    if (a.conf.base) {
        const __amdgpu_buffer_rsrc_t rc = plane_rsrc(a.conf.image<float>(b), view_bytes(a.H, a.conf.rs, a.W, 4));
        ok = ok && conf_valid(a, ld_f32(rc, inside ? (unsigned)((long long)i * a.conf.rs + j) * 4u : kOOB));
    }
    return ok;
}

__device__ __forceinline__ Camera camera_of(const BackprojectArgs& a, int b) {
    const float* k = a.k + (long long)b * a.kbs;
    return Camera{k[0], k[4], k[2], k[5]};
}

// the point of pixel (i, j) at depth z: subtract, multiply, divide, one fp32 rounding each
__device__ __forceinline__ void project(const Camera& c, int i, int j, float z, float& x, float& y) {
#pragma clang fp contract(off)
    const float u = (float)j - c.cx, v = (float)i - c.cy;
    const float uz = u * z, vz = v * z;
    x = uz / c.fx;
    y = vz / c.fy;
}

// n = c / l with l = sqrt((c.x c.x + c.y c.y) + c.z c.z): one fp32 rounding per operation, division and square
// root correctly rounded. True iff c has a direction: l > 0 && l < inf (normals.hip's unit normals, and the
// mean normal of voxel_merge.hip)
__device__ __forceinline__ bool unit_vector(float cx, float cy, float cz, float (&n)[3]) {
#pragma clang fp contract(off)
    const float xx = cx * cx, yy = cy * cy, zz = cz * cz;
    const float xy = xx + yy;
    const float len = sqrtf(xy + zz);  // the correctly rounded one (__fsqrt_rn is the hardware's approximation here)
    n[0] = __fdiv_rn(cx, len), n[1] = __fdiv_rn(cy, len), n[2] = __fdiv_rn(cz, len);
    return len > 0.f && len < __builtin_inff();
}

}  // namespace nconv
