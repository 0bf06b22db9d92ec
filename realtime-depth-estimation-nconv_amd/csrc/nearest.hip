// nearest.hip — for every pixel of a sparse depth plane the nearest sample and its distance
// (nconv_depth_nearest): the exact Euclidean distance transform with its feature (nearest-sample) map,
// in integers. include/nconv.h states the rule as the contract; per image and pixel p = (r, c):
//   sample(q)   v_q is finite and v_q > floor
//   d2(p, q)    = (r - r')^2 + (c - c')^2, an int32 (the host keeps H^2 + W^2 below 2^31)
//   near(p)     = the sample with the smallest d2, ties to the smallest pixel number r' * W + c'
//   none        where the image has no sample, or d2(p, near(p)) > max_dist2 >= 0
// The transform is separable, and so is the tie rule:
//   nearest_columns   work[r, c] = the row of the nearest sample of column c, the upper one on a tie, -1
//                     for a column without samples. Inside one column every sample but the column's
//                     nearest has a strictly larger d2 to (r, c'') for every c'', and of two at the same
//                     distance the upper has the smaller pixel number: no other sample of the column can
//                     be near(p) of a pixel of row r.
//                     A wave takes 64 rows of 64 columns, lanes across columns (a row is one coalesced
//                     load): the validity of its rows is one 64-bit mask per lane, and the nearest sample
//                     above and below a row inside the segment is a count of leading / trailing zeros.
//                     What lies outside the segment comes from a scan of the rows above and below it,
//                     ended per lane as soon as a row further out could not win against the segment's own
//                     samples, and for the wave when no lane asks any more. No workgroup waits for another.
//   nearest_rows      a workgroup takes one row r of one image, its work[r, :] in LDS where W <= kLdsW
//                     (read through the cache otherwise). A lane takes a pixel and searches c' = c, c -+ 1,
//                     c -+ 2, ... for the smallest 64-bit key (d2 << 32) | pixel number, which is the
//                     order of the rule in one unsigned min. It stops when the squared column offset
//                     exceeds the best d2 so far or max_dist2: "exceeds", because at k^2 == best a sample
//                     of row r itself still ties, and may have the smaller pixel number. Then dst, index,
//                     dist2 and dist are written; dst gathers the source value at near(p).
// The search is O(distance to the nearest sample) per pixel, O(W) where an image holds one sample or none.
// Integers only, no atomics: the result is a function of the input alone. The source is only read.
#include "nconv_internal.h"
#include "plane_io.h"

namespace nconv {

namespace {

constexpr int kT = 256;        // threads: four waves
constexpr int kSeg = 64;       // rows of a wave's segment: one bit each
constexpr int kLdsW = 4096;    // the widest row kept in LDS (16 KiB)
constexpr int kNoD2 = 0x7fffffff;

__device__ __forceinline__ bool is_sample(float v, float floor) { return __builtin_isfinite(v) && v > floor; }

__global__ __launch_bounds__(kT) void nearest_columns(NearestArgs a) {
    const int lane = (int)threadIdx.x & 63;
    const int nstrip = (a.W + 63) / 64, nseg = (a.H + kSeg - 1) / kSeg;
    const long long unit = (long long)blockIdx.x * (kT / 64) + ((int)threadIdx.x >> 6);  // wave-uniform
    if (unit >= (long long)a.B * nseg * nstrip) return;
    const int strip = (int)(unit % nstrip), seg = (int)(unit / nstrip % nseg), b = (int)(unit / nstrip / nseg);
    const int c = strip * 64 + lane, r0 = seg * kSeg, n = min(kSeg, a.H - r0);
    const bool active = c < a.W;
    const __amdgpu_buffer_rsrc_t rs = plane_rsrc(a.s.image<float>(b), view_bytes(a.H, a.s.rs, a.W, 4));
    // the sample at (row, c)? Lanes past the row's end aim at kOOB and are never samples.
    auto sample_at = [&](int row) {
        const float v = ld_f32(rs, active ? (unsigned)((long long)row * a.s.rs + c) * 4u : kOOB);
        return active && is_sample(v, a.floor);
    };

    unsigned long long m = 0ull;  // bit i: (r0 + i, c) is a sample
    for (int i = 0; i < n; ++i) m |= (unsigned long long)sample_at(r0 + i) << i;
    const int first = m ? __builtin_ctzll(m) : 0, last = m ? 63 - __builtin_clzll(m) : 0;

    // The nearest sample above the segment. Row rr can be nearest to a row of the segment only while
    // r0 - rr <= first (the segment's first row, which an upper sample wins on a tie).
    int up = -1;
    for (int rr = r0 - 1; rr >= 0; --rr) {
        const bool ask = active && up < 0 && (!m || r0 - rr <= first);
        if (!__any(ask)) break;
        if (sample_at(rr) && ask) up = rr;
    }
    // Below it: row rr wins for the segment's last row only while it is strictly nearer than `last`.
    int dn = -1;
    for (int rr = r0 + n; rr < a.H; ++rr) {
        const bool ask = active && dn < 0 && (!m || rr - (r0 + n - 1) < n - 1 - last);
        if (!__any(ask)) break;
        if (sample_at(rr) && ask) dn = rr;
    }

    if (!active) return;
    int* w = a.work + ((size_t)b * a.H + r0) * a.W + c;
    for (int i = 0; i < n; ++i) {
        const unsigned long long ma = m & (~0ull >> (63 - i)), mb = m >> i;
        const int r = r0 + i;
        const int above = ma ? r0 + 63 - __builtin_clzll(ma) : up;
        const int below = mb ? r + __builtin_ctzll(mb) : dn;
        w[(size_t)i * a.W] = above < 0 ? below : below < 0 || r - above <= below - r ? above : below;
    }
}

template <bool kLds>
__global__ __launch_bounds__(kT) void nearest_rows(NearestArgs a) {
    __shared__ int s_row[kLds ? kLdsW : 1];
    const int tid = (int)threadIdx.x;
    const int b = blockIdx.x / a.H, r = blockIdx.x - b * a.H;
    const size_t at = ((size_t)b * a.H + r) * a.W;  // of (b, r, 0) in the contiguous planes
    const int* __restrict__ g_row = a.work + at;
    if (kLds) {
        for (int j = tid; j < a.W; j += kT) s_row[j] = g_row[j];
        __syncthreads();
    }
    const int* row = kLds ? s_row : g_row;
    const __amdgpu_buffer_rsrc_t rs = plane_rsrc(a.s.image<float>(b), view_bytes(a.H, a.s.rs, a.W, 4));
    const int lim = a.max_dist2 < 0 ? kNoD2 : a.max_dist2;
    const unsigned long long kNone = ~0ull;

    for (int c = tid; c < a.W; c += kT) {
        unsigned long long best = kNone;
        int bound = lim;  // min(best d2, max_dist2): a column offset k with k * k > bound ends the search
        // the candidate of column cc, dc columns away
        auto take = [&](int cc, int dc2) {
            const int rr = row[cc];
            if (rr < 0) return;
            const int dr = r - rr, d2 = dc2 + dr * dr;  // < H^2 + W^2 < 2^31
            const unsigned long long key = ((unsigned long long)(unsigned)d2 << 32) | (unsigned)(rr * a.W + cc);
            if (key < best) best = key, bound = min(bound, d2);
        };
        take(c, 0);
        for (int k = 1; k * k <= bound; ++k) {  // k < W: k * k < 2^31
            const int lo = c - k, hi = c + k;
            if (lo < 0 && hi >= a.W) break;
            if (lo >= 0) take(lo, k * k);
            if (hi < a.W) take(hi, k * k);
        }
        const int d2 = (int)(best >> 32), px = (int)(unsigned)best;
        const bool found = best != kNone && d2 <= lim;
        if (a.dst) {
            const int pr = px / a.W, pc = px - pr * a.W;
            const float v = ld_f32(rs, found ? (unsigned)((long long)pr * a.s.rs + pc) * 4u : kOOB);
            a.dst[(long long)b * a.dbs + (long long)r * a.drs + c] = found ? v : 0.f;
        }
        if (a.index) a.index[at + c] = found ? px : -1;
        if (a.dist2) a.dist2[at + c] = found ? d2 : kNoD2;
        if (a.dist) a.dist[at + c] = found ? __builtin_sqrtf((float)d2) : __builtin_inff();
    }
}

}  // namespace

int launch_depth_nearest(const NearestArgs& a, hipStream_t st, const char** why) {
    const long long units = (long long)a.B * ((a.H + kSeg - 1) / kSeg) * ((a.W + 63) / 64);  // <= B * H * W < 2^31
    hipLaunchKernelGGL(nearest_columns, dim3((unsigned)((units + kT / 64 - 1) / (kT / 64))), dim3(kT), 0, st, a);
    const dim3 grid((unsigned)(a.B * a.H));
    if (a.W <= kLdsW)
        hipLaunchKernelGGL(nearest_rows<true>, grid, dim3(kT), 0, st, a);
    else
        hipLaunchKernelGGL(nearest_rows<false>, grid, dim3(kT), 0, st, a);
    return launch_status(why);
}

}  // namespace nconv
