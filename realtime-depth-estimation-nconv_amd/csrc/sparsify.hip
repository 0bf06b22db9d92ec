// sparsify.hip — an exact-count random subset of a depth plane (nconv_depth_sparsify): the reference's
// preprocess_depth (randperm, gather / scatter noise, mask) without the host, "N random samples", and
// thinning a LiDAR plane to a budget. include/nconv.h states the definition as the contract.
//
// Per image b and logical pixel p = row * W + col, (w0, w1, w2, w3) = Philox4x32-10((p, b, draw, 0),
// (seed_lo, seed_hi)) (philox.h). The n_b candidates with the smallest composite key
//   K = (w0 & key_mask) << 32 | p
// are kept. K is unique inside an image, so the kept set is the set {K <= T} with T the key of rank
// n_b - 1, and T is found by a radix select from the top: six digits of 11, 11, 11, 11, 10, 10 bits.
//
//   sparsify_reset      zeroes the six histograms of every image. A kernel and not hipMemsetAsync: with
//                       the memset captured as a node of a hipGraph, every replay after the first kept
//                       nothing (the thresholds came out 0, as from empty histograms)
//   sparsify_hist<j>    j = 0..5: the histogram of digit j over the candidates whose digits 0..j-1 are
//                       the threshold's. A workgroup first resolves digit j - 1 itself from histogram
//                       j - 1 (2048 bins: eight per thread, a scan over the workgroup) and the state
//                       after digit j - 2, which the first workgroup of the image left in the workspace
//                       during pass j - 1: the bucket scan is folded into the following pass, and no
//                       workgroup waits for another. After pass 0 the histogram's total is C_b, from
//                       which the target n_b follows (mode, n, n_dev, keep).
//   sparsify_apply      resolves digit 5, which completes T, and writes dst (and kept).
//
// Eight kernels whatever the data, the mode and n. A workgroup counts in a private LDS
// histogram and adds its non-zero bins to the image's with integer atomics, so the counts, T and the
// output do not depend on the order of execution or on how many workgroups share an image. The keys are
// recomputed in every pass (about sixty integer operations per pixel) rather than stored: the workspace
// stays 48 KiB per image and a pass reads four bytes per pixel. Every thread reads and writes only its
// own pixels, so dst may be src. The state buffer is only read. No host synchronisation: capturable.
#include <algorithm>
#include "nconv_internal.h"
#include "philox.h"
#include "plane_io.h"

namespace nconv {

namespace {

constexpr int kT = 256;            // threads: four waves
constexpr int kPix = 16;           // pixels per thread and tile
constexpr int kTile = kT * kPix;   // consecutive pixel numbers per tile
constexpr int kBins = 2048;        // 11-bit digits (the last two use 1024 of them)
constexpr int kPasses = 6;
constexpr int kMaxBlocks = 64;     // workgroups per image; each takes every nblk-th tile

__host__ __device__ constexpr int digit_shift(int j) { return j < 4 ? 53 - 11 * j : (5 - j) * 10; }
__host__ __device__ constexpr int digit_bits(int j) { return j < 4 ? 11 : 10; }

int blocks_per_image(int H, int W) {
    const long long tiles = ((long long)H * W + kTile - 1) / kTile;
    return (int)std::min<long long>(tiles, kMaxBlocks);
}

struct Pixel {
    bool cand;
    float d;
    unsigned long long key;
    unsigned w1, w2;
};

// pixel p of image b: its value, whether it is a candidate and, if so, its words
__device__ __forceinline__ Pixel pixel_of(const SparsifyArgs& a, int b, unsigned p, unsigned s0, unsigned s1,
                                          unsigned draw) {
    Pixel x;
    const unsigned row = p / (unsigned)a.W, col = p - row * (unsigned)a.W;
    x.d = a.src[(long long)b * a.sbs + (long long)row * a.srs + col];
    bool m = true;
    if (a.mask) m = a.mask[(long long)b * a.mbs + (long long)row * a.mrs + col] != 0;
    x.cand = m && (a.all_pixels || (x.d > a.floor && x.d <= __FLT_MAX__));
    x.key = 0, x.w1 = 0, x.w2 = 0;
    if (x.cand) {
        const uint32_t ctr[4] = {p, (uint32_t)b, draw, 0u}, key[2] = {s0, s1};
        uint32_t w[4];
        nconv_philox4x32_10(ctr, key, w);
        x.key = ((unsigned long long)(w[0] & a.key_mask) << 32) | p;
        x.w1 = w[1], x.w2 = w[2];
    }
    return x;
}

// n_b from the number of candidates
__device__ __forceinline__ int target_of(const SparsifyArgs& a, int b, unsigned C) {
    switch (a.mode) {
        case NCONV_SPARSIFY_COUNT: return (int)min((unsigned)a.n, C);
        case NCONV_SPARSIFY_COUNT_DEV: return (int)min((unsigned)max(a.n_dev[b], 0), C);
        case NCONV_SPARSIFY_FRACTION: return (int)floor((double)a.keep * (double)C);
        default: return (int)C;
    }
}

// The selection state after digit jp, by the whole workgroup: histogram jp of image b is scanned for the
// bucket that holds the wanted rank. jp == 0 starts from the histogram's total, C_b; later digits from
// the state after digit jp - 1 in the workspace (written during an earlier kernel).
__device__ SparsifySel resolve(const SparsifyArgs& a, int jp, int b) {
    __shared__ unsigned s_wave[kT / 64], s_digit, s_before;
    const int tid = (int)threadIdx.x;
    const unsigned* h = a.hist + ((size_t)jp * a.B + b) * kBins + tid * (kBins / kT);
    unsigned v[kBins / kT], sum = 0;
#pragma unroll
    for (int k = 0; k < kBins / kT; ++k) v[k] = h[k], sum += v[k];
    if (tid == 0) s_digit = 0u, s_before = 0u;  // the scan's barrier covers these too
    unsigned total;
    const unsigned excl = block_excl_scan<kT / 64>(sum, s_wave, total);
    SparsifySel s;
    if (jp == 0) {
        s.n = target_of(a, b, total);
        s.prefix = 0ull, s.rank = s.n > 0 ? (unsigned)s.n - 1u : 0u;
    } else {
        s = a.sel[(size_t)(jp - 1) * a.B + b];
    }
    if (s.rank >= excl && s.rank - excl < sum) {  // one thread at most; none where the image has no candidate
        unsigned c = excl;
#pragma unroll
        for (int k = 0; k < kBins / kT; ++k) {
            if (s.rank >= c && s.rank - c < v[k]) s_digit = (unsigned)(tid * (kBins / kT) + k), s_before = c;
            c += v[k];
        }
    }
    __syncthreads();
    s.prefix = (s.prefix << digit_bits(jp)) | s_digit;
    s.rank -= s_before;
    return s;
}

__global__ __launch_bounds__(kT) void sparsify_reset(unsigned* __restrict__ hist, size_t words) {
    for (size_t i = (size_t)blockIdx.x * kT + threadIdx.x; i < words; i += (size_t)gridDim.x * kT) hist[i] = 0u;
}

template <int j>
__global__ __launch_bounds__(kT) void sparsify_hist(SparsifyArgs a, int nblk) {
    __shared__ unsigned s_hist[kBins];
    const int tid = (int)threadIdx.x;
    const int b = (int)blockIdx.x / nblk, blk = (int)blockIdx.x - b * nblk;
    SparsifySel s{0ull, 0u, 0};
    if (j > 0) {
        s = resolve(a, j - 1, b);
        if (blk == 0 && tid == 0) a.sel[(size_t)(j - 1) * a.B + b] = s;
    }
    for (int i = tid; i < kBins; i += kT) s_hist[i] = 0u;
    __syncthreads();
    const unsigned s0 = a.state[0], s1 = a.state[1], draw = a.state[2];
    const unsigned hw = (unsigned)a.H * (unsigned)a.W;  // < 2^31, so p below stays under 2^32
    constexpr int sh = digit_shift(j), hi = j > 0 ? digit_shift(j - 1) : 0;
    constexpr unsigned dm = (1u << digit_bits(j)) - 1u;
    for (unsigned t0 = (unsigned)blk * kTile; t0 < hw; t0 += (unsigned)nblk * kTile) {
#pragma unroll 4
        for (int k = 0; k < kPix; ++k) {
            const unsigned p = t0 + (unsigned)(k * kT + tid);
            if (p >= hw) break;
            const Pixel x = pixel_of(a, b, p, s0, s1, draw);
            if (x.cand && (j == 0 || (x.key >> hi) == s.prefix)) atomicAdd(&s_hist[(unsigned)(x.key >> sh) & dm], 1u);
        }
    }
    __syncthreads();
    unsigned* g = a.hist + ((size_t)j * a.B + b) * kBins;
    for (int i = tid; i < kBins; i += kT) {
        const unsigned c = s_hist[i];
        if (c) atomicAdd(&g[i], c);
    }
}

// out = d + d * (noise_amp * (2 u - 1)), u = (w2 >> 8) * 2^-24: one rounding per operation
__device__ __forceinline__ float noisy(float d, unsigned w2, float amp) {
#pragma clang fp contract(off)
    const float u = (float)(w2 >> 8) * 0x1p-24f;  // exact
    const float s = 2.0f * u - 1.0f;              // exact
    const float r = amp * s;
    const float t = d * r;
    return d + t;
}

__global__ __launch_bounds__(kT) void sparsify_apply(SparsifyArgs a, int nblk) {
    const int tid = (int)threadIdx.x;
    const int b = (int)blockIdx.x / nblk, blk = (int)blockIdx.x - b * nblk;
    const SparsifySel s = resolve(a, kPasses - 1, b);  // prefix: the whole threshold key
    if (blk == 0 && tid == 0 && a.kept) a.kept[b] = s.n;
    const unsigned s0 = a.state[0], s1 = a.state[1], draw = a.state[2];
    const unsigned hw = (unsigned)a.H * (unsigned)a.W;
    for (unsigned t0 = (unsigned)blk * kTile; t0 < hw; t0 += (unsigned)nblk * kTile) {
#pragma unroll 4
        for (int k = 0; k < kPix; ++k) {
            const unsigned p = t0 + (unsigned)(k * kT + tid);
            if (p >= hw) break;
            const Pixel x = pixel_of(a, b, p, s0, s1, draw);
            float out = 0.f;
            if (x.cand && s.n > 0 && x.key <= s.prefix) out = x.w1 < a.noise_threshold ? noisy(x.d, x.w2, a.noise_amp) : x.d;
            const unsigned row = p / (unsigned)a.W, col = p - row * (unsigned)a.W;
            a.dst[(long long)b * a.dbs + (long long)row * a.drs + col] = out;
        }
    }
}

}  // namespace

size_t sparsify_workspace_bytes(int B) {
    return (size_t)B * kPasses * (kBins * sizeof(unsigned) + sizeof(SparsifySel));
}

int launch_depth_sparsify(SparsifyArgs a, void* workspace, hipStream_t st, const char** why) {
    // the states first (16 bytes each), the histograms behind them
    a.sel = (SparsifySel*)workspace;
    a.hist = (unsigned*)((char*)workspace + (size_t)a.B * kPasses * sizeof(SparsifySel));
    const int nblk = blocks_per_image(a.H, a.W);
    const dim3 grid((unsigned)((long long)a.B * nblk));  // <= B * H * W < 2^31
    const size_t words = (size_t)a.B * kPasses * kBins;
    const unsigned nreset = (unsigned)std::min<size_t>((words + kT - 1) / kT, 1u << 20);
    hipLaunchKernelGGL(sparsify_reset, dim3(nreset), dim3(kT), 0, st, a.hist, words);
    hipLaunchKernelGGL(sparsify_hist<0>, grid, dim3(kT), 0, st, a, nblk);
    hipLaunchKernelGGL(sparsify_hist<1>, grid, dim3(kT), 0, st, a, nblk);
    hipLaunchKernelGGL(sparsify_hist<2>, grid, dim3(kT), 0, st, a, nblk);
    hipLaunchKernelGGL(sparsify_hist<3>, grid, dim3(kT), 0, st, a, nblk);
    hipLaunchKernelGGL(sparsify_hist<4>, grid, dim3(kT), 0, st, a, nblk);
    hipLaunchKernelGGL(sparsify_hist<5>, grid, dim3(kT), 0, st, a, nblk);
    static_assert(kPasses == 6, "one launch per digit");
    hipLaunchKernelGGL(sparsify_apply, grid, dim3(kT), 0, st, a, nblk);
    return launch_status(why);
}

}  // namespace nconv
