// backproject.hip — a depth map and the camera intrinsics to metric 3-D points.
//
//   backproject_map     fp32 depth (B, H, W) view -> organised xyz planes (B, 3, H, W), NaN in all
//                       three planes where the pixel is not valid. One launch.
//   backproject_points  the valid pixels compacted to xyz (capacity, 3) [+ rgb (capacity, 3) uint8,
//                       + index (capacity) int32], raster order inside an image, images in batch
//                       order, and offsets (B + 1). Three launches: count, scan, write.
//
// A pixel (b, i, j) with z = depth[b, i, j] is valid iff z > z_min && z <= z_max && (no confidence
// || conf[b, i, j] >= conf_min): comparisons, so a NaN depth or confidence is not valid. Its point is
//   x = ((float)j - cx) * z / fx,  y = ((float)i - cy) * z / fy,  z
// one fp32 rounding per operation in that order, the division IEEE (correctly rounded); fx, fy, cx,
// cy = K[0][0], K[1][1], K[0][2], K[1][2] of image b's 3 x 3 matrix, read here (the other entries
// are not read).
//
// As in frame_io.hip a wave of 64 lanes takes four consecutive pixels per lane: one wave owns a
// segment of 256 consecutive pixels of one image row, a block of four waves four segments. Sources
// are read through buffer resources sized to the view's exact extent: 128-bit loads of 4 fp32 (96-bit
// of 4 interleaved RGB pixels) where base and strides are aligned and the four pixels lie inside the
// row, element-wide otherwise; a lane with nothing to read aims past the resource (kOOB) and gets 0.
// No load touches memory outside the views.
//
// Compaction: `count` writes each segment's number of valid pixels (four 64-bit ballots, popcount) to
// the workspace; `scan` (one workgroup looping over the array) turns them in place into exclusive
// prefix sums and writes offsets; `write` recomputes the validity (a second 4 B/px read of depth is
// cheaper than storing masks) and gives each valid pixel the rank
//   segment prefix + sum_k popcount(ballot_k & lanes below) + the lane's own earlier valid pixels,
// storing only ranks below the capacity. Order comes from the scan alone: no atomics, no flag or
// counter one workgroup waits on, so the result is the same on every run. No allocation and no host
// synchronisation: the calls can be captured in a hipGraph.
#include "nconv_internal.h"

namespace nconv {

namespace {

typedef unsigned u32x3 __attribute__((ext_vector_type(3)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int kBT = 256;                // threads: four waves, one segment each
constexpr int kSeg = 64 * 4;            // pixels per segment (four per lane)
constexpr int kScanT = 1024;            // the scan's single workgroup
constexpr int kScanE = 4;               // segments per thread and round
constexpr unsigned kOOB = 0x80000000u;  // past every resource (extents are < 2^31 bytes): reads 0

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

// values k (bits of `want`, all below n) of the four fp32 at byte offset off; the others read 0
__device__ __forceinline__ f4 row_load4(__amdgpu_buffer_rsrc_t r, bool vec, int n, unsigned want, unsigned off) {
    if (vec && (n == 4 || want == 0u))
        return __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(r, want ? off : kOOB, 0, 0));
    f4 v;
    v.x = ld_f32(r, want & 1u ? off : kOOB);
    v.y = ld_f32(r, want & 2u ? off + 4u : kOOB);
    v.z = ld_f32(r, want & 4u ? off + 8u : kOOB);
    v.w = ld_f32(r, want & 8u ? off + 12u : kOOB);
    return v;
}

// bit k: pixel j + k of row i is valid; z = the four depths (0 past the row)
__device__ __forceinline__ unsigned valid4(const BackprojectArgs& a, const Where& w, f4& z) {
    const unsigned in_row = w.n > 0 ? (1u << w.n) - 1u : 0u;
    const int dbytes = (int)(((long long)(a.H - 1) * a.drs + a.W) * 4);
    const __amdgpu_buffer_rsrc_t rd = plane_rsrc(a.depth + (long long)w.b * a.dbs, dbytes);
    z = row_load4(rd, a.d_vec != 0, w.n, in_row, (unsigned)((long long)w.i * a.drs + w.j) * 4u);
    unsigned m = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) m |= (unsigned)(z[k] > a.z_min && z[k] <= a.z_max) << k;
    m &= in_row;
    if (a.conf) {
        const int cbytes = (int)(((long long)(a.H - 1) * a.crs + a.W) * 4);
        const __amdgpu_buffer_rsrc_t rc = plane_rsrc(a.conf + (long long)w.b * a.cbs, cbytes);
        const f4 c = row_load4(rc, a.c_vec != 0, w.n, in_row, (unsigned)((long long)w.i * a.crs + w.j) * 4u);
        unsigned mc = 0u;
#pragma unroll
        for (int k = 0; k < 4; ++k) mc |= (unsigned)(c[k] >= a.conf_min) << k;
        m &= mc;
    }
    return m;
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

// clamp(rintf(v), 0, 255); comparisons, so a NaN becomes 0
__device__ __forceinline__ unsigned colour_q(float v) {
    float q = rintf(v);
    q = q > 0.f ? q : 0.f;
    q = q < 255.f ? q : 255.f;
    return (unsigned)q;
}

// c[k] = the three output bytes of pixel k (byte 0 first) for the pixels in `want`
__device__ __forceinline__ void colour4(const BackprojectArgs& a, const Where& w, unsigned want, unsigned (&c)[4]) {
    c[0] = c[1] = c[2] = c[3] = 0u;
    if (a.color_kind == NCONV_COLOR_F32_PLANAR) {
        const float* base = (const float*)a.color + (long long)w.b * a.obs;
        const int bytes = (int)(((long long)(a.H - 1) * a.ors + a.W) * 4);
        const unsigned off = (unsigned)((long long)w.i * a.ors + w.j) * 4u;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const __amdgpu_buffer_rsrc_t r = plane_rsrc(base + (long long)ch * a.ocs, bytes);
            const f4 v = row_load4(r, a.o_fast != 0, w.n, want, off);
            const int sh = 8 * (a.reverse ? 2 - ch : ch);
#pragma unroll
            for (int k = 0; k < 4; ++k) c[k] |= colour_q(v[k]) << sh;
        }
    } else {
        const unsigned char* base = (const unsigned char*)a.color + (long long)w.b * a.obs;
        const int bytes = (int)((long long)(a.H - 1) * a.ors + 3LL * a.W);
        const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc((void*)base, (short)0, bytes, 0x00020000);
        const unsigned off = (unsigned)((long long)w.i * a.ors + 3LL * w.j);
        unsigned d[3] = {0u, 0u, 0u};
        if (a.o_fast && (w.n == 4 || want == 0u)) {
            const u32x3 v = __builtin_amdgcn_raw_buffer_load_b96(r, want ? off : kOOB, 0, 0);
            d[0] = v.x, d[1] = v.y, d[2] = v.z;
        } else {
#pragma unroll
            for (int q = 0; q < 12; ++q) {
                const unsigned byte = __builtin_amdgcn_raw_buffer_load_b8(r, (want >> (q / 3)) & 1u ? off + q : kOOB, 0, 0);
                d[q >> 2] |= (byte & 0xffu) << ((q & 3) * 8);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const int q = 3 * k + ch;
                c[k] |= ((d[q >> 2] >> ((q & 3) * 8)) & 0xffu) << (8 * (a.reverse ? 2 - ch : ch));
            }
    }
}

// n (0..4) leading values of v to p[0..n): one 128-bit store where p is 16-byte aligned
__device__ __forceinline__ void put4(float* p, f4 v, int n) {
    if (n == 4 && ((size_t)p & 15) == 0) {
        *(f4*)p = v;
        return;
    }
    if (n > 0) p[0] = v.x;
    if (n > 1) p[1] = v.y;
    if (n > 2) p[2] = v.z;
    if (n > 3) p[3] = v.w;
}

// lanes below this one that have their bit set in the ballot
__device__ __forceinline__ int lanes_below(unsigned long long ballot) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ballot, 0u));
}

__global__ __launch_bounds__(kBT) void backproject_map(BackprojectArgs a, float* __restrict__ xyz) {
    Where w;
    if (!segment_of_wave(a, w) || w.n <= 0) return;
    f4 z;
    const unsigned m = valid4(a, w, z);
    const Camera cam = camera_of(a, w.b);
    const float nan = __builtin_nanf("");
    f4 x, y;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float px, py;
        project(cam, w.i, w.j + k, z[k], px, py);
        const bool ok = (m >> k) & 1u;
        x[k] = ok ? px : nan;
        y[k] = ok ? py : nan;
        z[k] = ok ? z[k] : nan;
    }
    const size_t plane = (size_t)a.H * a.W;
    float* p = xyz + (size_t)w.b * 3 * plane + (size_t)w.i * a.W + w.j;
    put4(p, x, w.n);
    put4(p + plane, y, w.n);
    put4(p + 2 * plane, z, w.n);
}

__global__ __launch_bounds__(kBT) void backproject_count(BackprojectArgs a, int* __restrict__ counts) {
    Where w;
    if (!segment_of_wave(a, w)) return;
    f4 z;
    const unsigned m = valid4(a, w, z);
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) cnt += __popcll(__ballot((m >> k) & 1u));
    if ((threadIdx.x & 63) == 0) counts[w.s] = cnt;
}

// counts[0..nseg) -> their exclusive prefix sums, in place; offsets[b] = the prefix at image b's first
// segment, offsets[B] = the total. One workgroup: kScanT * kScanE segments per round.
__global__ __launch_bounds__(kScanT) void backproject_scan(int* __restrict__ counts, int nseg, int per_image, int B,
                                                           int* __restrict__ offsets) {
    __shared__ int wave_sum[kScanT / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;
    for (int base = 0; base < nseg; base += kScanT * kScanE) {
        const int idx = base + (int)threadIdx.x * kScanE;
        int v[kScanE], mine = 0;
#pragma unroll
        for (int k = 0; k < kScanE; ++k) {
            v[k] = idx + k < nseg ? counts[idx + k] : 0;
            mine += v[k];
        }
        int inc = mine;  // inclusive scan over the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int t = __shfl_up(inc, d);
            if (lane >= d) inc += t;
        }
        if (lane == 63) wave_sum[wave] = inc;
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int q = 0; q < kScanT / 64; ++q) {
            const int t = wave_sum[q];
            before += q < wave ? t : 0;
            total += t;
        }
        int ex = carry + before + inc - mine;
#pragma unroll
        for (int k = 0; k < kScanE; ++k) {
            if (idx + k < nseg) {
                counts[idx + k] = ex;
                const int img = (idx + k) / per_image;
                if ((idx + k) - img * per_image == 0) offsets[img] = ex;
            }
            ex += v[k];
        }
        carry += total;
        __syncthreads();  // wave_sum is rewritten in the next round
    }
    if (threadIdx.x == 0) offsets[B] = carry;
}

__global__ __launch_bounds__(kBT) void backproject_write(BackprojectArgs a, const int* __restrict__ prefix,
                                                         float* __restrict__ xyz, unsigned char* __restrict__ rgb,
                                                         int* __restrict__ index, int capacity) {
    Where w;
    if (!segment_of_wave(a, w)) return;
    f4 z;
    const unsigned m = valid4(a, w, z);
    int rank = prefix[w.s];
#pragma unroll
    for (int k = 0; k < 4; ++k) rank += lanes_below(__ballot((m >> k) & 1u));
    // the pixels this lane stores: valid and ranked below the capacity (ranks ascend with k)
    unsigned st = 0u;
    {
        int r = rank;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if ((m >> k) & 1u) {
                st |= (unsigned)(r < capacity) << k;
                ++r;
            }
    }
    unsigned col[4] = {0u, 0u, 0u, 0u};
    if (rgb) colour4(a, w, st, col);
    if (st == 0u) return;
    const Camera cam = camera_of(a, w.b);
    const int pix = (w.b * a.H + w.i) * a.W + w.j;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!((st >> k) & 1u)) continue;  // st is a prefix of m's bits: rank counts exactly the stored ones
        float px, py;
        project(cam, w.i, w.j + k, z[k], px, py);
        float* p = xyz + (size_t)rank * 3;
        p[0] = px, p[1] = py, p[2] = z[k];
        if (rgb) {
            unsigned char* q = rgb + (size_t)rank * 3;
            q[0] = (unsigned char)col[k], q[1] = (unsigned char)(col[k] >> 8), q[2] = (unsigned char)(col[k] >> 16);
        }
        if (index) index[rank] = pix + k;
        ++rank;
    }
}

int launch_status(const char** why) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        *why = hipGetErrorString(e);
        return -5;
    }
    return 0;
}

}  // namespace

long long backproject_segments(int B, int H, int W) { return (long long)B * H * ((W + kSeg - 1) / kSeg); }

size_t backproject_workspace_bytes(int B, int H, int W) {
    return (size_t)((backproject_segments(B, H, W) + 3) / 4 * 4) * sizeof(int);
}

int launch_backproject_map(const BackprojectArgs& a, float* xyz, hipStream_t st, const char** why) {
    hipLaunchKernelGGL(backproject_map, dim3((a.nseg + kBT / 64 - 1) / (kBT / 64)), dim3(kBT), 0, st, a, xyz);
    return launch_status(why);
}

int launch_backproject_points(const BackprojectArgs& a, float* xyz, unsigned char* rgb, int* index, int capacity,
                              int* offsets, int* ws, hipStream_t st, const char** why) {
    const dim3 grid((a.nseg + kBT / 64 - 1) / (kBT / 64));
    hipLaunchKernelGGL(backproject_count, grid, dim3(kBT), 0, st, a, ws);
    if (int rc = launch_status(why)) return rc;
    hipLaunchKernelGGL(backproject_scan, dim3(1), dim3(kScanT), 0, st, ws, a.nseg, a.nseg / a.B, a.B, offsets);
    if (int rc = launch_status(why)) return rc;
    hipLaunchKernelGGL(backproject_write, grid, dim3(kBT), 0, st, a, (const int*)ws, xyz, rgb, index, capacity);
    return launch_status(why);
}

}  // namespace nconv
