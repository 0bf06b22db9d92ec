// colorize.hip — a strided view of fp32 depth planes to the picture people look at: uint8 (B, H, W, 3)
// through a 256-entry colour table (the reference's save_depth, utils.py:12-16: min-max normalise, then
// OpenCV's INFERNO map), with sparse planes drawn as squares over a camera image.
//
//   colorize_range_reset   the per-image range keys set to (all ones, 0): the empty minimum and maximum
//   colorize_range         the minimum and maximum of the non-empty pixels of every image: per thread, per
//                          wave (shuffles), per workgroup (LDS), then one atomic minimum and one atomic
//                          maximum per workgroup on order-preserving uint32 keys; a workgroup takes every
//                          kRangeChunks-th tile of its image (same-address atomics serialise)
//   colorize_map<SPLAT>    the picture. SPLAT: each output pixel shows the smallest non-empty value of its
//                          (2 r + 1)^2 window, reduced separably (rows, then columns) in LDS
//
// Per pixel value v, all fp32, contraction off:
//   empty    iff v is not finite or v <= floor
//   lo, hi   the minimum and maximum of the image's non-empty source pixels (auto range), or vmin, vmax
//   s        = 255.0f / (hi - lo), one correctly rounded division
//   idx      = clamp((int)rintf((v - lo) * s), 0, 255), ties to even; the clamp is made on the float, so
//              a product past the int range saturates and a NaN (0 * inf) gives 0; hi <= lo: idx = 0
// A non-empty pixel gets table[idx], an empty one the background pixel (byte for byte) or empty_rgb. The
// window minimum does not depend on the order it is taken in (the candidates are finite; +0 and -0 give
// the same index), nor do the integer atomics of the range: the picture is the same on every run.
//
// A workgroup takes a tile of kTH rows x kTW pixels; a lane takes four consecutive pixels of kR rows:
// one 128-bit load per row where the view allows it (plane_io.h), twelve output bytes per row as three
// dword stores where they start on a 4-byte boundary, byte stores otherwise. The table is staged in LDS
// packed one dword per entry, already in the output's channel order, so bgr costs nothing per pixel.
#include <algorithm>
#include "colormaps.h"
#include "nconv_internal.h"

namespace nconv {

namespace {

constexpr int kT = 256;             // threads: four waves
constexpr int kR = 2;               // rows per wave
constexpr int kTH = kT / 64 * kR;   // rows per tile
constexpr int kTW = 64 * 4;         // pixels per tile row (four per lane)
constexpr int kMaxR = 4;            // largest splat radius
constexpr int kAW = kTW + 2 * kMaxR;  // row pitch of the staged tile with its halo
constexpr int kAH = kTH + 2 * kMaxR;
constexpr int kRangeChunks = 32;    // workgroups per image of the range pass

// fp32 -> uint32 whose unsigned order is the float order (-0 below +0), and back
__device__ __forceinline__ unsigned range_key(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float range_val(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__device__ __forceinline__ bool non_empty(float v, float floor) { return __builtin_isfinite(v) && v > floor; }

// three roundings (subtract, multiply, rint), no fused multiply-add; float comparisons, so NaN -> 0
__device__ __forceinline__ unsigned color_index(float v, float lo, float s) {
#pragma clang fp contract(off)
    const float d = v - lo;
    const float x = d * s;
    float q = rintf(x);
    q = q > 0.f ? q : 0.f;
    q = q < 255.f ? q : 255.f;
    return (unsigned)q;
}

// pixel k (0..3) of three dwords of interleaved bytes, as a packed 24-bit value
__device__ __forceinline__ unsigned pix24(const unsigned (&d)[3], int k) {
    switch (k) {
        case 0: return d[0] & 0xffffffu;
        case 1: return (d[0] >> 24) | ((d[1] & 0xffffu) << 8);
        case 2: return (d[1] >> 16) | ((d[2] & 0xffu) << 16);
        default: return d[2] >> 8;
    }
}

__global__ __launch_bounds__(kT) void colorize_range_reset(unsigned* __restrict__ range, unsigned n) {
    const unsigned t = blockIdx.x * (unsigned)kT + threadIdx.x;  // n = 2 B < 2^32
    if (t < n) range[t] = (t & 1) ? 0u : 0xffffffffu;
}

// chunks workgroups per image, each taking every chunks-th tile of it: one pair of atomics per workgroup,
// so at most kRangeChunks pairs meet on an image's two keys
__global__ __launch_bounds__(kT) void colorize_range(ColorizeArgs a, int chunks) {
    __shared__ unsigned s_min[kT / 64], s_max[kT / 64];
    const int per = tiles_per_image<kTH, kTW>(a.H, a.W);
    const int b = blockIdx.x / chunks, chunk = blockIdx.x - b * chunks;
    const __amdgpu_buffer_rsrc_t r = plane_rsrc(a.d.image<float>(b), view_bytes(a.H, a.d.rs, a.W, 4));
    unsigned kmin = 0xffffffffu, kmax = 0u;
    for (int t = chunk; t < per; t += chunks) {
        int i0, j;
        tile_corner<kTH, kTW>(a.W, t, i0, j);
        i0 += (threadIdx.x >> 6) * kR, j += (threadIdx.x & 63) * 4;
        const int n = min(4, a.W - j);  // <= 0: the lane is past the row
        f4 v[kR];
#pragma unroll
        for (int rr = 0; rr < kR; ++rr) {
            const int i = i0 + rr;
            v[rr] = load4_f32(r, a.d.wide != 0, i < a.H, n, (unsigned)((long long)i * a.d.rs + j) * 4u);
        }
#pragma unroll
        for (int rr = 0; rr < kR; ++rr)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                // a pixel outside the plane reads 0, which may be a non-empty value: it is not one of the image's
                const bool in = i0 + rr < a.H && k < n;
                if (in && non_empty(v[rr][k], a.floor)) {
                    const unsigned key = range_key(v[rr][k]);
                    kmin = min(kmin, key), kmax = max(kmax, key);
                }
            }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        kmin = min(kmin, (unsigned)__shfl_xor((int)kmin, off));
        kmax = max(kmax, (unsigned)__shfl_xor((int)kmax, off));
    }
    if ((threadIdx.x & 63) == 0) s_min[threadIdx.x >> 6] = kmin, s_max[threadIdx.x >> 6] = kmax;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kT / 64; ++w) kmin = min(kmin, s_min[w]), kmax = max(kmax, s_max[w]);
        if (kmin <= kmax) {  // these tiles hold a non-empty pixel
            __hip_atomic_fetch_min(a.range + 2 * (size_t)b, kmin, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_max(a.range + 2 * (size_t)b + 1, kmax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

template <bool SPLAT>
__global__ __launch_bounds__(kT) void colorize_map(ColorizeArgs a) {
    __shared__ unsigned s_lut[256];
    __shared__ __attribute__((aligned(16))) float s_a[SPLAT ? kAH * kAW : 4];  // the tile and its halo
    __shared__ __attribute__((aligned(16))) float s_b[SPLAT ? kAH * kTW : 4];  // its row minima
    const float kNone = __builtin_inff();  // an empty pixel among the window's candidates
    const TileOrigin o = tile_origin<kTH, kTW>(a.H, a.W);
    const int b = o.b, ti = o.i0, tj = o.j0;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i0 = ti + wave * kR, j = tj + lane * 4;
    {
        const unsigned e = threadIdx.x;  // kT == 256 entries
        unsigned cr, cg, cb;
        if (a.lut) {
            cr = a.lut[3 * e], cg = a.lut[3 * e + 1], cb = a.lut[3 * e + 2];
        } else if (a.cmap < 4) {
            const unsigned char* t = kColormaps[a.cmap];
            cr = t[3 * e], cg = t[3 * e + 1], cb = t[3 * e + 2];
        } else {
            cr = cg = cb = e;
        }
        s_lut[e] = a.bgr ? (cb | (cg << 8) | (cr << 16)) : (cr | (cg << 8) | (cb << 16));
    }
    const __amdgpu_buffer_rsrc_t r = plane_rsrc(a.d.image<float>(b), view_bytes(a.H, a.d.rs, a.W, 4));
    const int n = min(4, a.W - j);  // <= 0: the lane is past the row
    f4 m[kR];                       // the value each pixel shows, kNone where it is empty
    if (SPLAT) {
        const int rad = a.radius, rows = kTH + 2 * rad, cols = kTW + 2 * rad;
        for (int row = 0; row < rows; ++row) {
            const int gi = ti - rad + row;
            for (int c = threadIdx.x; c < cols; c += kT) {
                const int gj = tj - rad + c;
                const bool in = gi >= 0 && gi < a.H && gj >= 0 && gj < a.W;
                const float v = ld_f32(r, in ? (unsigned)((long long)gi * a.d.rs + gj) * 4u : kOOB);
                s_a[row * kAW + c] = in && non_empty(v, a.floor) ? v : kNone;
            }
        }
        __syncthreads();
        for (int row = 0; row < rows; ++row) {
            float q = kNone;
            for (int k = 0; k <= 2 * rad; ++k) q = fminf(q, s_a[row * kAW + threadIdx.x + k]);
            s_b[row * kTW + threadIdx.x] = q;
        }
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < kR; ++rr) {
            f4 q = {kNone, kNone, kNone, kNone};
            for (int k = 0; k <= 2 * rad; ++k) {
                const f4 w = *(const f4*)&s_b[(wave * kR + rr + k) * kTW + lane * 4];
                q.x = fminf(q.x, w.x), q.y = fminf(q.y, w.y), q.z = fminf(q.z, w.z), q.w = fminf(q.w, w.w);
            }
            m[rr] = q;
        }
    } else {
#pragma unroll
        for (int rr = 0; rr < kR; ++rr) {
            const int i = i0 + rr;
            const f4 v = load4_f32(r, a.d.wide != 0, i < a.H, n, (unsigned)((long long)i * a.d.rs + j) * 4u);
#pragma unroll
            for (int k = 0; k < 4; ++k) m[rr][k] = non_empty(v[k], a.floor) ? v[k] : kNone;
        }
        __syncthreads();  // the table
    }
    unsigned bgd[kR][3];
    if (a.bg.base) {
        const __amdgpu_buffer_rsrc_t rb =
            bytes_rsrc(a.bg.image<unsigned char>(b), view_bytes(a.H, a.bg.rs, 3LL * a.W, 1));
#pragma unroll
        for (int rr = 0; rr < kR; ++rr) {
            const int i = i0 + rr;
            load4_rgb8(rb, a.bg.wide != 0, i < a.H, n, (unsigned)((long long)i * a.bg.rs + 3LL * j), bgd[rr]);
        }
    }
    float lo = a.lo, hi = a.hi;
    if (a.auto_range) lo = range_val(a.range[2 * (size_t)b]), hi = range_val(a.range[2 * (size_t)b + 1]);
    const bool flat = hi <= lo;
    const float s = __fdiv_rn(255.0f, hi - lo);
#pragma unroll
    for (int rr = 0; rr < kR; ++rr) {
        const int i = i0 + rr;
        if (i >= a.H || n <= 0) continue;
        unsigned p[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float v = m[rr][k];
            const unsigned idx = flat ? 0u : color_index(v, lo, s);
            const unsigned none = a.bg.base ? pix24(bgd[rr], k) : a.empty;
            p[k] = v < kNone ? s_lut[idx] : none;
        }
        const unsigned o[3] = {p[0] | (p[1] << 24), (p[1] >> 8) | (p[2] << 16), (p[2] >> 16) | (p[3] << 8)};
        unsigned char* q = a.out + (((size_t)b * a.H + i) * a.W + j) * 3;
        if (n == 4 && ((size_t)q & 3) == 0) {
            unsigned* qw = (unsigned*)q;
            qw[0] = o[0], qw[1] = o[1], qw[2] = o[2];
        } else {
#pragma unroll
            for (int c = 0; c < 12; ++c)
                if (c < 3 * n) q[c] = (unsigned char)(o[c >> 2] >> ((c & 3) * 8));
        }
    }
}

}  // namespace

int launch_depth_colorize(const ColorizeArgs& a, hipStream_t st, const char** why) {
    const dim3 grid((unsigned)a.B * (unsigned)tiles_per_image<kTH, kTW>(a.H, a.W));
    if (a.auto_range) {
        const unsigned keys = 2u * (unsigned)a.B;
        hipLaunchKernelGGL(colorize_range_reset, dim3((keys - 1) / kT + 1), dim3(kT), 0, st, a.range, keys);
        const int chunks = std::min(tiles_per_image<kTH, kTW>(a.H, a.W), kRangeChunks);
        hipLaunchKernelGGL(colorize_range, dim3((unsigned)a.B * (unsigned)chunks), dim3(kT), 0, st, a, chunks);
    }
    if (a.radius > 0)
        hipLaunchKernelGGL(colorize_map<true>, grid, dim3(kT), 0, st, a);
    else
        hipLaunchKernelGGL(colorize_map<false>, grid, dim3(kT), 0, st, a);
    return launch_status(why);
}

}  // namespace nconv
