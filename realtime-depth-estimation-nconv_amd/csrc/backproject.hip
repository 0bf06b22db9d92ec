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
// The tiling, the validity rule and the point are defined in backproject_common.h, which normals.hip
// shares. A wave of 64 lanes takes four consecutive pixels per lane: one wave owns a segment of 256
// consecutive pixels of one image row, a block of four waves four segments. Depth, confidence and
// colour are views read with plane_io.h's loaders (load4_f32, load4_rgb8); a lane with nothing to
// read passes n = 0 and gets 0. No load touches memory outside the views.
//
// Compaction: `count` writes each segment's number of valid pixels (four 64-bit ballots, popcount) to
// the workspace; `scan` (one workgroup looping over the array) turns them in place into exclusive
// prefix sums and writes offsets; `write` recomputes the validity (a second 4 B/px read of depth is
// cheaper than storing masks) and gives each valid pixel the rank
//   segment prefix + sum_k popcount(ballot_k & lanes below) + the lane's own earlier valid pixels,
// storing only ranks below the capacity. Order comes from the scan alone: no atomics, no flag or
// counter one workgroup waits on, so the result is the same on every run. No allocation and no host
// synchronisation: the calls can be captured in a hipGraph.
#include "backproject_common.h"

namespace nconv {

namespace {

constexpr int kScanT = 1024;            // the scan's single workgroup
constexpr int kScanE = 4;               // segments per thread and round

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
    const int n = want ? w.n : 0;  // the row's pixels where the lane stores any of them, else nothing
    if (a.color_kind == NCONV_COLOR_F32_PLANAR) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            const f4 v = view_load4(a, a.color, a.color.image<float>(w.b) + (long long)ch * a.ocs, w, n);
            const int sh = 8 * (a.reverse ? 2 - ch : ch);
#pragma unroll
            for (int k = 0; k < 4; ++k) c[k] |= colour_q(v[k]) << sh;
        }
    } else {
        const __amdgpu_buffer_rsrc_t r =
            bytes_rsrc(a.color.image<unsigned char>(w.b), view_bytes(a.H, a.color.rs, 3LL * a.W, 1));
        unsigned d[3];
        load4_rgb8(r, a.color.wide != 0, true, n, (unsigned)((long long)w.i * a.color.rs + 3LL * w.j), d);
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const int q = 3 * k + ch;
                c[k] |= ((d[q >> 2] >> ((q & 3) * 8)) & 0xffu) << (8 * (a.reverse ? 2 - ch : ch));
            }
    }
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
    store4_f32(p, x, w.n);
    store4_f32(p + plane, y, w.n);
    store4_f32(p + 2 * plane, z, w.n);
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
    __shared__ int s_wave[kScanT / 64];
    int carry = 0;
    for (int base = 0; base < nseg; base += kScanT * kScanE) {
        const int idx = base + (int)threadIdx.x * kScanE;
        int v[kScanE], mine = 0;
#pragma unroll
        for (int k = 0; k < kScanE; ++k) {
            v[k] = idx + k < nseg ? counts[idx + k] : 0;
            mine += v[k];
        }
        int total;
        int ex = carry + block_excl_scan<kScanT / 64>(mine, s_wave, total);
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
        __syncthreads();  // s_wave is rewritten in the next round
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
