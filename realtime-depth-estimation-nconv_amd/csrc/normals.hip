// normals.hip — surface normals of a depth map from the camera intrinsics, on the image grid.
//
//   depth_normals_map     fp32 depth (B, H, W) view -> unit normals (B, 3, H, W), NaN in all three planes
//                         where the pixel has none, and / or the camera-space normal picture (B, H, W, 3)
//                         uint8, which never sees the fp32 map in memory. One launch.
//   depth_normals_points  the normals of the rows of a packed cloud (nconv_backproject_points' index and
//                         offsets) as (capacity, 3) fp32, (0, 0, 0) where there is none. One launch.
//
// The definition (include/nconv.h states it as the contract): validity V and point P of a pixel are
// nconv_backproject's (backproject_common.h), and a pixel outside the image is not valid. A centre c
// that is not valid has no normal. A neighbour n of a valid centre at depth z is usable iff
//   V(n) && (gate off || fabsf(z_n - z) <= jump_abs + jump_rel * z)
// (comparisons: a NaN is not usable; the gate is off when jump_rel == jump_abs == 0). With R, L the
// pixels right and left of the centre the horizontal tangent is
//   tu = P(R) - P(L) | P(R) - P(c) | P(c) - P(L)   as both | only R | only L are usable, else no normal
// and the vertical tangent tv likewise from D (below, in R's role) and T (above). Then
//   c = tv x tu                       each component two products and one subtraction
//   d = (c.x P.x + c.y P.y) + c.z P.z; d > 0: c = -c      (towards the camera: n . P <= 0)
//   l = sqrt((c.x c.x + c.y c.y) + c.z c.z); a normal iff l > 0 && l < inf; n = c / l
// every operation one fp32 rounding in that order, no contraction, division and square root correctly
// rounded. A fronto-parallel surface gets (0, 0, -1).
//
// The map kernel keeps backproject.hip's tiling: a wave owns 256 consecutive pixels of row i, a lane
// four of them. It reads rows i - 1, i, i + 1 with load4_f32 (a row outside the plane reads nothing);
// the pixels left and right of a lane's four come from the adjacent lanes by __shfl_up / __shfl_down
// (ds_bpermute, no LDS storage), and the two at the wave's ends from one range-checked load: lane 0
// reads pixel j - 1, lane 63 pixel j + 4, the other lanes aim it past the view. No load touches a byte
// outside a view. The points kernel reads a pixel and its four neighbours with five such single loads
// and runs the same normal_of. Nothing depends on the order of execution: the result is the same on
// every run. No workspace, no host synchronisation: the calls can be captured in a hipGraph.
#include <algorithm>
#include "backproject_common.h"

namespace nconv {

namespace {

struct P3 {
    float x, y, z;
};

__device__ __forceinline__ P3 point_of(const Camera& cam, int i, int j, float z) {
    P3 p;
    project(cam, i, j, z, p.x, p.y);
    p.z = z;
    return p;
}

// hi - lo of the two neighbours on an axis, the centre standing in for the one that is not usable
__device__ __forceinline__ P3 tangent(const P3& c, const P3& lo, bool use_lo, const P3& hi, bool use_hi) {
#pragma clang fp contract(off)
    const P3 p = use_hi ? hi : c, q = use_lo ? lo : c;
    return P3{p.x - q.x, p.y - q.y, p.z - q.z};
}

// The normal of a pixel from its point c and those of its four neighbours (v*: validity). False: none.
__device__ __forceinline__ bool normal_of(const NormalsArgs& o, bool vc, const P3& c, bool vl, const P3& l, bool vr,
                                          const P3& r, bool vt, const P3& t, bool vd, const P3& d, float (&n)[3]) {
#pragma clang fp contract(off)
    const float jz = o.jump_rel * c.z;
    const float tol = o.jump_abs + jz;
    const bool open = o.gate == 0;
    const bool ul = vl && (open || fabsf(l.z - c.z) <= tol), ur = vr && (open || fabsf(r.z - c.z) <= tol);
    const bool ut = vt && (open || fabsf(t.z - c.z) <= tol), ud = vd && (open || fabsf(d.z - c.z) <= tol);
    const P3 tu = tangent(c, l, ul, r, ur), tv = tangent(c, t, ut, d, ud);
    const float a0 = tv.y * tu.z, a1 = tv.z * tu.y, b0 = tv.z * tu.x, b1 = tv.x * tu.z, c0 = tv.x * tu.y,
                c1 = tv.y * tu.x;
    float cx = a0 - a1, cy = b0 - b1, cz = c0 - c1;
    const float dx = cx * c.x, dy = cy * c.y, dz = cz * c.z;
    const float dxy = dx + dy;
    const float dot = dxy + dz;
    if (dot > 0.f) cx = -cx, cy = -cy, cz = -cz;
    const bool unit = unit_vector(cx, cy, cz, n);  // backproject_common.h
    return vc && (ul || ur) && (ut || ud) && unit;
}

// clamp(rintf((0.5 + s * t * 0.5) * 255), 0, 255), s = +1 / -1: the products with 0.5 and -1 are exact
__device__ __forceinline__ unsigned channel_q(float t, bool negate) {
#pragma clang fp contract(off)
    const float h = t * 0.5f;
    const float u = negate ? 0.5f - h : h + 0.5f;
    float q = rintf(u * 255.0f);
    q = q > 0.f ? q : 0.f;
    q = q < 255.f ? q : 255.f;
    return (unsigned)q;
}

__global__ __launch_bounds__(kBT) void depth_normals_map(BackprojectArgs a, NormalsArgs o, float* __restrict__ normals,
                                                         unsigned char* __restrict__ image) {
    Where w;
    if (!segment_of_wave(a, w)) return;  // the whole wave
    const int lane = (int)(threadIdx.x & 63);
    Where wt = w, wd = w;
    wt.i = w.i - 1, wd.i = w.i + 1;
    f4 zc, zt, zd;
    const unsigned mc = valid4(a, w, zc);
    const unsigned mt = valid4(a, wt, zt, w.i > 0);
    const unsigned md = valid4(a, wd, zd, w.i + 1 < a.H);
    // the pixel before the wave's first (lane 0) and after its last (lane 63); no other lane reads
    const int je = lane == 0 ? w.j - 1 : w.j + 4;
    float ze;
    const bool ve = valid1(a, w.b, w.i, je, (lane == 0 || lane == 63) && je >= 0 && je < a.W, ze);
    float zl = __shfl_up(zc[3], 1), zr = __shfl_down(zc[0], 1);
    bool vl = (__shfl_up((int)mc, 1) >> 3) & 1, vr = __shfl_down((int)mc, 1) & 1;
    if (lane == 0) zl = ze, vl = ve;
    if (lane == 63) zr = ze, vr = ve;
    if (w.n <= 0) return;  // past the row; its lanes have served their neighbours

    const Camera cam = camera_of(a, w.b);
    P3 row[6], top[4], bot[4];
    row[0] = point_of(cam, w.i, w.j - 1, zl);
    row[5] = point_of(cam, w.i, w.j + 4, zr);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        row[k + 1] = point_of(cam, w.i, w.j + k, zc[k]);
        top[k] = point_of(cam, w.i - 1, w.j + k, zt[k]);
        bot[k] = point_of(cam, w.i + 1, w.j + k, zd[k]);
    }
    const unsigned mrow = (unsigned)vl | (mc << 1) | ((unsigned)vr << 5);
    const float nan = __builtin_nanf("");
    f4 nx, ny, nz;
    unsigned p[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float n[3];
        const bool ok = normal_of(o, (mrow >> (k + 1)) & 1u, row[k + 1], (mrow >> k) & 1u, row[k], (mrow >> (k + 2)) & 1u,
                                  row[k + 2], (mt >> k) & 1u, top[k], (md >> k) & 1u, bot[k], n);
        nx[k] = ok ? n[0] : nan;
        ny[k] = ok ? n[1] : nan;
        nz[k] = ok ? n[2] : nan;
        p[k] = ok ? channel_q(n[0], false) | (channel_q(n[1], true) << 8) | (channel_q(n[2], true) << 16) : o.empty;
    }
    if (normals) {
        const size_t plane = (size_t)a.H * a.W;
        float* q = normals + (size_t)w.b * 3 * plane + (size_t)w.i * a.W + w.j;
        store4_f32(q, nx, w.n);
        store4_f32(q + plane, ny, w.n);
        store4_f32(q + 2 * plane, nz, w.n);
    }
    if (image) {
        const unsigned d[3] = {p[0] | (p[1] << 24), (p[1] >> 8) | (p[2] << 16), (p[2] >> 16) | (p[3] << 8)};
        unsigned char* q = image + (((size_t)w.b * a.H + w.i) * a.W + w.j) * 3;
        if (w.n == 4 && ((size_t)q & 3) == 0) {
            unsigned* qw = (unsigned*)q;
            qw[0] = d[0], qw[1] = d[1], qw[2] = d[2];
        } else {
#pragma unroll
            for (int c = 0; c < 12; ++c)
                if (c < 3 * w.n) q[c] = (unsigned char)(d[c >> 2] >> ((c & 3) * 8));
        }
    }
}

__global__ __launch_bounds__(kBT) void depth_normals_points(BackprojectArgs a, NormalsArgs o,
                                                            const int* __restrict__ index,
                                                            const int* __restrict__ offsets, int capacity,
                                                            float* __restrict__ normals) {
    const long long r = (long long)blockIdx.x * kBT + threadIdx.x;
    if (r >= min(offsets[a.B], capacity)) return;
    const int pix = index[r];
    float n[3];
    bool ok = false;
    if (pix >= 0 && pix < a.B * a.H * a.W) {  // B * H * W < 2^31; nothing is read for an index outside
        const int line = pix / a.W, j = pix - line * a.W, b = line / a.H, i = line - b * a.H;
        float zc, zl, zr, zt, zd;
        const bool vc = valid1(a, b, i, j, true, zc);
        const bool vl = valid1(a, b, i, j - 1, j > 0, zl), vr = valid1(a, b, i, j + 1, j + 1 < a.W, zr);
        const bool vt = valid1(a, b, i - 1, j, i > 0, zt), vd = valid1(a, b, i + 1, j, i + 1 < a.H, zd);
        const Camera cam = camera_of(a, b);
        ok = normal_of(o, vc, point_of(cam, i, j, zc), vl, point_of(cam, i, j - 1, zl), vr, point_of(cam, i, j + 1, zr),
                       vt, point_of(cam, i - 1, j, zt), vd, point_of(cam, i + 1, j, zd), n);
    }
    float* q = normals + (size_t)r * 3;
    q[0] = ok ? n[0] : 0.f, q[1] = ok ? n[1] : 0.f, q[2] = ok ? n[2] : 0.f;
}

}  // namespace

int launch_depth_normals(const BackprojectArgs& a, const NormalsArgs& o, float* normals, unsigned char* image,
                         hipStream_t st, const char** why) {
    hipLaunchKernelGGL(depth_normals_map, dim3((a.nseg + kBT / 64 - 1) / (kBT / 64)), dim3(kBT), 0, st, a, o, normals,
                       image);
    return launch_status(why);
}

int launch_depth_normals_points(const BackprojectArgs& a, const NormalsArgs& o, const int* index, const int* offsets,
                                int capacity, float* normals, hipStream_t st, const char** why) {
    // offsets[B] <= B * H * W: rows past that are never written
    const long long rows = std::min<long long>(capacity, (long long)a.B * a.H * a.W);
    if (rows <= 0) return 0;
    hipLaunchKernelGGL(depth_normals_points, dim3((unsigned)((rows + kBT - 1) / kBT)), dim3(kBT), 0, st, a, o, index,
                       offsets, capacity, normals);
    return launch_status(why);
}

}  // namespace nconv
