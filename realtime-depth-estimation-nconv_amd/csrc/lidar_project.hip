// lidar_project.hip — an unordered LiDAR scan and a 3 x 4 projection to the sparse depth plane the
// models take: the inverse of backproject.hip, under the same convention (pixel centres at integer
// coordinates, one fp32 rounding per operation).
//
//   lidar_fill       the z-buffer set to all ones (the key no point can have)
//   lidar_scatter    one thread per point row: project, test, and reduce into the z-buffer with an
//                    unsigned integer atomic minimum (no return value)
//   lidar_resolve*   the z-buffer turned into the outputs: all ones -> depth 0 (and index -1)
//
// Per point p = (x, y, z) of image b, with the rows r of b's matrix m, contraction off:
//   dot(r, p) = ((r0 * x + r1 * y) + r2 * z) + r3,   a, b, c = dot(m[0..2], p)
//   u = a / c, v = b / c (IEEE),   fj = rintf(u), fi = rintf(v)
//   valid iff c > z_min && c <= z_max && fj >= 0 && fj <= W - 1 && fi >= 0 && fi <= H - 1
// all float comparisons made before the conversion to int, so NaN, infinities and huge coordinates
// are not valid and every converted value is a pixel of the plane. A valid c is positive, so its bit
// pattern orders as an unsigned integer, and the minimum of integers does not depend on the order the
// hardware takes the points in: the outputs are the same on every run.
//
// Two z-buffers. Without index the output plane itself holds bits(c), reduced with a 32-bit minimum:
// no workspace. With index a workspace holds one 64-bit key (bits(c) << 32) | row per pixel, reduced
// with a 64-bit minimum, so that among bit-equal depths the smallest row number wins; the resolve pass
// splits the key into the two outputs.
//
// A block takes 256 consecutive rows and reads them through a buffer resource over exactly its rows'
// extent (the last row ends after its third float): 128-bit loads of whole 4-float rows where the
// stride is 4 and the base 16-byte aligned, the last row of the scan excepted (its fourth float is
// past the extent), element loads otherwise. A lane without a row aims at plane_io.h's kOOB and reads 0.
// The image of a row comes from a binary search of offsets, staged in LDS up to kLdsOffsets entries
// and read from global memory above that. A wave whose first and last rows are in the same image
// (almost every wave) takes the matrix from wave-uniform addresses, which the compiler turns into
// scalar loads; a wave that straddles a boundary searches and loads per lane.
//
// The atomics go to the memory side one pixel per lane, scattered (the order-of-magnitude slow shape
// of a float atomic sum), but there is one per valid point and nothing waits on it: at 8 x 120 k rows
// of which a fifth are valid that is 0.2 M atomics per call. Fill and resolve move 16 bytes per lane
// from the first 16-byte boundary of the plane on; the words before it and the ragged tail go singly.
#include "nconv_internal.h"

namespace nconv {

namespace {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));

constexpr int kT = 256;                 // threads of every kernel here; rows of a scatter block
constexpr int kLdsOffsets = 1024;       // offsets are staged in LDS up to this many entries (B + 1)
constexpr unsigned kEmpty32 = 0xFFFFFFFFu;
constexpr unsigned long long kEmpty64 = ~0ull;

// The n 4-byte words at `base` dealt to threads: thread 0 takes the (up to three) words before the
// first 16-byte boundary, thread t >= 1 the t-th group of four from that boundary on, the last group
// possibly short. lo = first word, n = words (0: none).
struct Span {
    size_t lo;
    int n;
};

__host__ __device__ __forceinline__ size_t span_head(const void* base, size_t n) {
    const size_t head = ((16 - ((size_t)base & 15)) & 15) / 4;
    return head < n ? head : n;
}

__device__ __forceinline__ Span span_of(const void* base, size_t n) {
    const size_t t = (size_t)blockIdx.x * kT + threadIdx.x;
    const size_t head = span_head(base, n);
    const size_t lo = t ? head + 4 * (t - 1) : 0;
    size_t hi = t ? lo + 4 : head;
    hi = hi < n ? hi : n;
    return Span{lo, lo < hi ? (int)(hi - lo) : 0};
}

unsigned span_blocks(const void* base, size_t n) {
    const size_t threads = 1 + (n - span_head(base, n) + 3) / 4;
    return (unsigned)((threads + kT - 1) / kT);
}

__device__ __forceinline__ bool aligned16(const void* p) { return ((size_t)p & 15) == 0; }

__global__ __launch_bounds__(kT) void lidar_fill(unsigned* __restrict__ p, size_t n) {
    const Span s = span_of(p, n);
    unsigned* q = p + s.lo;
    if (s.n == 4 && aligned16(q)) {
        *(u32x4*)q = u32x4{kEmpty32, kEmpty32, kEmpty32, kEmpty32};
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < s.n) q[k] = kEmpty32;
}

// the 32-bit z-buffer is the output plane: a pixel no point reached becomes 0.0f, in place
__global__ __launch_bounds__(kT) void lidar_resolve32(unsigned* __restrict__ p, size_t n) {
    const Span s = span_of(p, n);
    unsigned* q = p + s.lo;
    if (s.n == 4 && aligned16(q)) {
        u32x4 v = *(const u32x4*)q;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = v[k] == kEmpty32 ? 0u : v[k];
        *(u32x4*)q = v;
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < s.n) {
            const unsigned v = q[k];
            q[k] = v == kEmpty32 ? 0u : v;
        }
}

// the 64-bit keys split into depth (the high word's float, 0.0f for an empty pixel) and index (the low
// word, -1 for an empty pixel); the groups of four start on depth's 16-byte boundaries
__global__ __launch_bounds__(kT) void lidar_resolve64(const unsigned long long* __restrict__ keys,
                                                      unsigned* __restrict__ depth, int* __restrict__ index, size_t n) {
    const Span s = span_of(depth, n);
    if (s.n == 0) return;
    const unsigned long long* kq = keys + s.lo;
    unsigned long long key[4] = {kEmpty64, kEmpty64, kEmpty64, kEmpty64};
    if (s.n == 4 && aligned16(kq)) {
        const u64x2 lo = *(const u64x2*)kq, hi = *(const u64x2*)(kq + 2);
        key[0] = lo.x, key[1] = lo.y, key[2] = hi.x, key[3] = hi.y;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < s.n) key[k] = kq[k];
    }
    u32x4 d;
    i32x4 ix;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool empty = key[k] == kEmpty64;
        d[k] = empty ? 0u : (unsigned)(key[k] >> 32);
        ix[k] = empty ? -1 : (int)(unsigned)key[k];
    }
    unsigned* dq = depth + s.lo;
    int* iq = index + s.lo;
    if (s.n == 4 && aligned16(dq)) {
        *(u32x4*)dq = d;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < s.n) dq[k] = d[k];
    }
    if (s.n == 4 && aligned16(iq)) {
        *(i32x4*)iq = ix;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < s.n) iq[k] = ix[k];
    }
}

// The image of row r: the number of entries of off[0..B] that are <= r, less one. -1 below off[0], B
// from off[B] on; always in [-1, B], whatever the array holds.
template <class P>
__device__ __forceinline__ int image_of(P off, int B, int r) {
    int lo = 0, hi = B + 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= r)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo - 1;
}

struct Matrix {
    float r[3][4];
};

__device__ __forceinline__ Matrix matrix_at(const float* m) {
    Matrix q;
#pragma unroll
    for (int k = 0; k < 12; ++k) q.r[k / 4][k % 4] = m[k];
    return q;
}

// ((r0 * x + r1 * y) + r2 * z) + r3: five roundings, no fused multiply-add
__device__ __forceinline__ float dot_row(const float (&r)[4], float x, float y, float z) {
#pragma clang fp contract(off)
    const float p0 = r[0] * x, p1 = r[1] * y, p2 = r[2] * z;
    const float s01 = p0 + p1;
    const float s012 = s01 + p2;
    return s012 + r[3];
}

// project the lane's point with image b's matrix and, where it is valid, reduce it into the z-buffer
template <bool KEYS>
__device__ __forceinline__ void scatter_point(const LidarArgs& a, float wmax, float hmax, const Matrix& q, int b,
                                              bool in, int row, float x, float y, float z, unsigned* zbuf,
                                              unsigned long long* keys) {
    const float pa = dot_row(q.r[0], x, y, z), pb = dot_row(q.r[1], x, y, z), c = dot_row(q.r[2], x, y, z);
    const float u = pa / c, v = pb / c;
    const float fj = rintf(u), fi = rintf(v);
    const bool ok = in && c > a.z_min && c <= a.z_max && fj >= 0.f && fj <= wmax && fi >= 0.f && fi <= hmax;
    if (!ok) return;
    // fj in [0, W - 1] and fi in [0, H - 1] as floats: the pixel is inside the plane, below 2^31
    const int pix = (b * a.H + (int)fi) * a.W + (int)fj;
    const unsigned bits = __float_as_uint(c);
    if (KEYS)
        __hip_atomic_fetch_min(keys + pix, ((unsigned long long)bits << 32) | (unsigned)row, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    else
        __hip_atomic_fetch_min(zbuf + pix, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// wmax, hmax: the largest floats <= W - 1, H - 1 (the host rounds down where W - 1 is not a float)
template <bool KEYS>
__global__ __launch_bounds__(kT) void lidar_scatter(LidarArgs a, float wmax, float hmax, unsigned* __restrict__ zbuf,
                                                    unsigned long long* __restrict__ keys) {
    __shared__ int s_off[kLdsOffsets];
    const bool staged = a.B + 1 <= kLdsOffsets;
    if (staged) {
        for (int q = threadIdx.x; q <= a.B; q += kT) s_off[q] = a.offsets[q];
        __syncthreads();
    }
    const int t = threadIdx.x;
    const int r0 = (int)(blockIdx.x * (unsigned)kT);  // < n_rows < 2^31
    const int nb = min(kT, a.n_rows - r0);            // rows of this block, >= 1
    const int wave_first = r0 + (t & ~63);
    if (wave_first >= a.n_rows) return;
    const int wave_last = min(wave_first + 63, a.n_rows - 1);
    const bool live = t < nb;
    const int row = r0 + t;

    // x, y, z through a resource over this block's rows alone (its extent is below 2^31 bytes): whole
    // rows where a later block's row follows, else up to the third float of the scan's last row
    const int bytes = view_bytes(nb, a.stride, r0 + nb < a.n_rows ? a.stride : 3, 4);
    const __amdgpu_buffer_rsrc_t rs = plane_rsrc(a.points + (size_t)r0 * a.stride, bytes);
    float x, y, z;
    if (a.vec && (t + 1) * 16 <= bytes) {
        const f4 p = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(rs, (unsigned)t * 16u, 0, 0));
        x = p.x, y = p.y, z = p.z;
    } else {
        const unsigned off = live ? (unsigned)t * (unsigned)a.stride * 4u : kOOB;
        x = ld_f32(rs, off);
        y = ld_f32(rs, off + 4u);
        z = ld_f32(rs, off + 8u);
    }

    int b_first, b_last;
    if (staged) {
        b_first = image_of(s_off, a.B, wave_first);
        b_last = image_of(s_off, a.B, wave_last);
    } else {
        b_first = image_of(a.offsets, a.B, wave_first);
        b_last = image_of(a.offsets, a.B, wave_last);
    }
    b_first = __builtin_amdgcn_readfirstlane(b_first);
    b_last = __builtin_amdgcn_readfirstlane(b_last);
    if (b_first == b_last) {
        // the whole wave in one image (offsets do not decrease), or in none
        if (b_first < 0 || b_first >= a.B) return;
        const Matrix q = matrix_at(a.m + (long long)b_first * a.mbs);
        scatter_point<KEYS>(a, wmax, hmax, q, b_first, live, row, x, y, z, zbuf, keys);
    } else {
        const int b = staged ? image_of(s_off, a.B, row) : image_of(a.offsets, a.B, row);
        const bool in = live && b >= 0 && b < a.B;
        const Matrix q = matrix_at(a.m + (long long)(in ? b : 0) * a.mbs);
        scatter_point<KEYS>(a, wmax, hmax, q, in ? b : 0, in, row, x, y, z, zbuf, keys);
    }
}

// the largest float <= n (n >= 0): n itself where it is a float, else the float below
float float_floor(int n) {
    float f = (float)n;
    if ((long long)f > (long long)n) f = __builtin_nextafterf(f, 0.f);
    return f;
}

}  // namespace

int launch_lidar_project(const LidarArgs& a, float* depth, int* index, unsigned long long* keys, hipStream_t st,
                         const char** why) {
    const size_t npix = (size_t)a.B * a.H * a.W;
    unsigned* zbuf = (unsigned*)depth;
    unsigned* fill = keys ? (unsigned*)keys : zbuf;
    const size_t words = keys ? 2 * npix : npix;
    hipLaunchKernelGGL(lidar_fill, dim3(span_blocks(fill, words)), dim3(kT), 0, st, fill, words);
    if (int rc = launch_status(why)) return rc;
    if (a.n_rows > 0) {
        const dim3 grid((unsigned)(((long long)a.n_rows + kT - 1) / kT));
        const float wmax = float_floor(a.W - 1), hmax = float_floor(a.H - 1);
        if (keys)
            hipLaunchKernelGGL(lidar_scatter<true>, grid, dim3(kT), 0, st, a, wmax, hmax, zbuf, keys);
        else
            hipLaunchKernelGGL(lidar_scatter<false>, grid, dim3(kT), 0, st, a, wmax, hmax, zbuf, keys);
        if (int rc = launch_status(why)) return rc;
    }
    if (keys)
        hipLaunchKernelGGL(lidar_resolve64, dim3(span_blocks(depth, npix)), dim3(kT), 0, st,
                           (const unsigned long long*)keys, zbuf, index, npix);
    else
        hipLaunchKernelGGL(lidar_resolve32, dim3(span_blocks(depth, npix)), dim3(kT), 0, st, zbuf, npix);
    return launch_status(why);
}

}  // namespace nconv
