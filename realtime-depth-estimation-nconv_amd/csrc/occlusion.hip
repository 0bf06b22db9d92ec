// occlusion.hip — LiDAR returns the camera cannot see, taken out of a sparse depth plane
// (nconv_depth_occlusion). The scanner sits above and behind the camera, so beside every foreground
// silhouette the projected scan holds background returns between the foreground ones; a return is
// dropped when enough clearly nearer returns lie in its window. include/nconv.h states the rule as the
// contract; per image and pixel p with value v_p, all fp32, contraction off:
//   valid(p)    v_p is finite and v_p > floor
//   lim(q)      = v_q + (jump_abs + jump_rel * v_q)        (multiply, add, add)
//   support(p)  = the number of valid q != p inside the image with |i_q - i_p| <= rh, |j_q - j_p| <= rw
//                 and v_p > lim(q)
//   removed(p)  = valid(p) && support(p) >= min_support
//
//   occlusion_counts_reset   zeroes the 2 B counters (only when counts is asked for)
//   occlusion_filter         everything else, one launch. A workgroup takes a tile of kTH x kTW pixels:
//     1. lim of the tile and its halo goes to LDS, +inf where the pixel is outside the image or not
//        valid (v_p > +inf never holds, so such a pixel supports nothing; the in-image test is made on
//        the coordinates, never on the 0 a load past the view returns: 0 is a valid depth under a
//        negative floor). The staged columns start a multiple of four left of the tile, so that every
//        group of four is one 128-bit load where the view allows it (plane_io.h).
//     2. every thread reads its own eight pixels (two groups of four) and appends the valid ones to a
//        list in LDS (ballot, one LDS atomic per wave and pixel slot): on a LiDAR plane one pixel in
//        twenty, so a loop per pixel would leave nineteen lanes in twenty idle.
//     3. the list is worked off by groups of G lanes, G the power of two that holds the window's taps
//        (at most 64): the lanes of a group share one centre's window, consecutive lanes on consecutive
//        columns of a row of the staged tile, and add their counts with shuffles. The group's first
//        lane sets the centre's flag byte in LDS.
//     4. every thread writes its eight pixels: dst as 128-bit stores, removed as dwords, index only
//        where it becomes -1, and the workgroup adds its two counts with one integer atomic each.
// The list's order depends on the atomics, the result does not: a flag is a function of the centre's
// window alone, and the counters are integer sums. The source is only read.
#include "nconv_internal.h"
#include "plane_io.h"

namespace nconv {

namespace {

constexpr int kT = 256;                  // threads: four waves
constexpr int kTH = 32, kTW = 64;        // the tile: eight pixels per thread
constexpr int kMaxR = 16;                // largest rh, rw
constexpr int kPitch = kTW + 2 * kMaxR;  // row pitch of the staged tile with its halo
constexpr int kRows = kTH + 2 * kMaxR;
constexpr int kGroupsPerRow = kTW / 4;   // the tile's groups of four pixels: 16 per row
constexpr int kPix = kTH * kTW / kT;     // 8

__device__ __forceinline__ bool valid_depth(float v, float floor) { return __builtin_isfinite(v) && v > floor; }

// lim(q): three roundings, no fused multiply-add
__device__ __forceinline__ float lim_of(float v, float jump_abs, float jump_rel) {
#pragma clang fp contract(off)
    const float t = jump_rel * v;
    const float u = jump_abs + t;
    return v + u;
}

__global__ __launch_bounds__(kT) void occlusion_counts_reset(int* __restrict__ counts, unsigned n) {
    const unsigned t = blockIdx.x * (unsigned)kT + threadIdx.x;  // n = 2 B < 2^32
    if (t < n) counts[t] = 0;
}

__global__ __launch_bounds__(kT) void occlusion_filter(OcclusionArgs a) {
    __shared__ __attribute__((aligned(16))) float s_lim[kRows * kPitch];  // lim, +inf: supports nothing
    __shared__ float s_cv[kTH * kTW];                                     // the valid centres: value
    __shared__ unsigned short s_cp[kTH * kTW];                            //   and position row * kTW + col
    __shared__ __attribute__((aligned(4))) unsigned char s_rm[kTH * kTW];  // 1: removed
    __shared__ unsigned s_n, s_nrm;
    const float kNone = __builtin_inff();
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const TileOrigin o = tile_origin<kTH, kTW>(a.H, a.W);
    const int b = o.b, ti = o.i0, tj = o.j0;
    const int rh = a.rh, rw = a.rw, rwp = (rw + 3) & ~3;  // the staged columns start at tj - rwp
    const __amdgpu_buffer_rsrc_t r = plane_rsrc(a.s.image<float>(b), view_bytes(a.H, a.s.rs, a.W, 4));
    const bool wide = a.s.wide != 0;

    // 1. lim of the tile and its halo
    if (tid == 0) s_n = 0u, s_nrm = 0u;
    {
        const int rows = kTH + 2 * rh, gpr = (kTW + 2 * rwp) / 4;
        for (int g = tid; g < rows * gpr; g += kT) {
            const int row = g / gpr, grp = g - row * gpr;
            const int gi = ti - rh + row, gj = tj - rwp + 4 * grp;  // gj is a multiple of 4: < 0 means <= -4
            const bool in_row = gi >= 0 && gi < a.H && gj >= 0;
            const int n = min(4, a.W - gj);
            const f4 v = load4_f32(r, wide, in_row, n, (unsigned)((long long)gi * a.s.rs + gj) * 4u);
            f4 l;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                l[k] = in_row && k < n && valid_depth(v[k], a.floor) ? lim_of(v[k], a.jump_abs, a.jump_rel) : kNone;
            *(f4*)&s_lim[row * kPitch + 4 * grp] = l;
        }
    }
    for (int i = tid; i < kTH * kTW / 4; i += kT) ((unsigned*)s_rm)[i] = 0u;
    __syncthreads();

    // 2. this thread's pixels: groups tid and tid + kT of the tile, the valid ones to the list
    f4 v[2];
    bool ok[2][4];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int g = tid + h * kT, pr = g / kGroupsPerRow, pc = (g % kGroupsPerRow) * 4;
        const int i = ti + pr, j = tj + pc, n = min(4, a.W - j);
        v[h] = load4_f32(r, wide, i < a.H, n, (unsigned)((long long)i * a.s.rs + j) * 4u);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            ok[h][k] = i < a.H && k < n && valid_depth(v[h][k], a.floor);
            const unsigned long long m = __ballot(ok[h][k]);
            unsigned base = 0u;
            if (lane == 0 && m) base = atomicAdd(&s_n, (unsigned)__popcll(m));
            base = (unsigned)__shfl((int)base, 0);
            if (ok[h][k]) {
                const unsigned at = base + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
                s_cv[at] = v[h][k];
                s_cp[at] = (unsigned short)(pr * kTW + pc + k);
            }
        }
    }
    __syncthreads();

    // 3. G lanes per centre: lane q of a group takes the taps q, q + G, ... of the (2 rh + 1) x (2 rw + 1)
    //    window in raster order, stepping (dr, dc) by (G / nw, G % nw) with a carry
    {
        const int nw = 2 * rw + 1, taps = (2 * rh + 1) * nw;
        int G = 4;
        while (G < taps && G < 64) G <<= 1;
        const int sq = G / nw, sr = G - sq * nw;
        const int q = tid & (G - 1), gid = tid / G, ngroups = kT / G;
        const int dr0 = q / nw, dc0 = q - dr0 * nw;
        const int n = (int)s_n;
        for (int c0 = 0; c0 < n; c0 += ngroups) {  // the same trips for every lane: the shuffles need them all
            const int c = c0 + gid;
            const bool live = c < n;
            const float vp = live ? s_cv[c] : -kNone;  // -inf is above no lim
            const int pos = live ? (int)s_cp[c] : 0;
            const int pr = pos / kTW, pc = pos - pr * kTW;
            const float* w = &s_lim[pr * kPitch + pc + rwp - rw];  // the window's first tap
            int cnt = 0;
            for (int tap = q, dr = dr0, dc = dc0; tap < taps; tap += G) {
                const bool centre = dr == rh && dc == rw;
                cnt += !centre && vp > w[dr * kPitch + dc];
                dr += sq, dc += sr;
                if (dc >= nw) dc -= nw, ++dr;
            }
            for (int off = G >> 1; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
            if (live && q == 0 && cnt >= a.min_support) {
                s_rm[pos] = 1;
                atomicAdd(&s_nrm, 1u);
            }
        }
    }
    __syncthreads();

    // 4. the outputs
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int g = tid + h * kT, pr = g / kGroupsPerRow, pc = (g % kGroupsPerRow) * 4;
        const int i = ti + pr, j = tj + pc, n = min(4, a.W - j);
        if (i >= a.H || n <= 0) continue;
        const unsigned rm = *(const unsigned*)&s_rm[pr * kTW + pc];
        f4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = ok[h][k] && !((rm >> (8 * k)) & 1u) ? v[h][k] : 0.f;
        store4_f32(a.dst + (long long)b * a.dbs + (long long)i * a.drs + j, o, n);
        const size_t at = ((size_t)b * a.H + i) * a.W + j;
        if (a.removed) {
            unsigned char* p = a.removed + at;
            if (n == 4 && ((size_t)p & 3) == 0) {
                *(unsigned*)p = rm;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < n) p[k] = (unsigned char)((rm >> (8 * k)) & 1u);
            }
        }
        if (a.index) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < n && (!ok[h][k] || ((rm >> (8 * k)) & 1u))) a.index[at + k] = -1;
        }
    }
    if (a.counts && tid == 0) {
        if (s_n) atomicAdd(&a.counts[2 * (size_t)b], (int)s_n);
        if (s_nrm) atomicAdd(&a.counts[2 * (size_t)b + 1], (int)s_nrm);
    }
}

}  // namespace

int launch_depth_occlusion(const OcclusionArgs& a, hipStream_t st, const char** why) {
    static_assert(kTH * kTW == kT * kPix && kPix == 8, "two groups of four pixels per thread");
    static_assert(kTH * kTW <= 65536, "positions are 16-bit");
    if (a.counts) {
        const unsigned n = 2u * (unsigned)a.B;
        hipLaunchKernelGGL(occlusion_counts_reset, dim3((n - 1) / kT + 1), dim3(kT), 0, st, a.counts, n);
    }
    const long long tiles = tiles_per_image<kTH, kTW>(a.H, a.W);
    hipLaunchKernelGGL(occlusion_filter, dim3((unsigned)(a.B * tiles)), dim3(kT), 0, st, a);  // <= B * H * W < 2^31
    return launch_status(why);
}

}  // namespace nconv
