// radix_pass.h — one digit of a stable least-significant-digit radix sort of (key32, value32) pairs, for
// one segment whose length n is read on the device. A sort is kernels that call hist_pass and then
// scatter_pass once per digit, from the lowest up, with the two buffer pairs swapped in between; the number
// of digits is the caller's (from the key range it knows on the host), so the launches never depend on the
// data. voxel_merge.hip sorts with these; sparsification.hip's spars_hist / spars_scatter are the same passes
// and can adopt them (a segment there is a pointer offset and an n of its own).
//
//   hist_pass     the segment is cut into nblk equal runs of whole sort tiles (run_of; the run length follows
//                 from n), one per workgroup. A workgroup counts the digit of its run's keys in LDS (integer
//                 atomics: counting only) and writes all kBins counts: nothing to zero beforehand
//   scatter_pass  thread d sums column d of the segment's nblk histograms (the runs before its own, and all);
//                 a scan over the workgroup gives digit d's base. Then, kTile keys at a time in run order, a
//                 key's rank among the equal digits is
//                   keys of earlier rounds (thread d's running count) + of lower waves of this round (a fixed
//                   wave-order prefix in LDS) + of lower lanes of its wave (ballots),
//                 never the order in which anything lands: the scatter is stable, and the same on every run
//
// A workgroup is kT = 256 threads (four waves), one bin per thread. No global atomics, no floating point.
#pragma once
#include "wave_ops.h"

namespace nconv {
namespace radix {

constexpr int kT = 256;                 // threads: four waves
constexpr int kDigitBits = 8;           // digit width
constexpr int kBins = 1 << kDigitBits;  // one bin per thread
constexpr int kTile = kT;               // sort tile: the keys of one round, one per thread
static_assert(kBins == kT, "thread d owns digit d");
static_assert(kT / 64 == 4, "scatter_pass spells out its four waves");

// digits that keys in [0, max_key] need: ceil(bits(max_key) / kDigitBits); 0 where max_key == 0
inline int passes_for(unsigned max_key) {
    int bits = 0;
    while (max_key) ++bits, max_key >>= 1;
    return (bits + kDigitBits - 1) / kDigitBits;
}

// the run [lo, hi) of positions that workgroup blk of nblk takes of a segment of n keys
__device__ __forceinline__ void run_of(int n, int nblk, int blk, long long& lo, long long& hi) {
    const long long per = ((long long)n + nblk - 1) / nblk;
    const long long run = (per + kTile - 1) / kTile * kTile;
    lo = (long long)blk * run < n ? (long long)blk * run : n;
    hi = lo + run < n ? lo + run : n;
}

// hist: the segment's nblk x kBins counts; this workgroup writes row blk
__device__ __forceinline__ void hist_pass(const unsigned* __restrict__ kin, int n, int nblk, int blk, int shift,
                                          unsigned* __restrict__ hist) {
    __shared__ unsigned s_h[kBins];
    long long lo, hi;
    run_of(n, nblk, blk, lo, hi);
    s_h[threadIdx.x] = 0u;
    __syncthreads();
    for (long long i = lo + threadIdx.x; i < hi; i += kT) atomicAdd(&s_h[(kin[i] >> shift) & (kBins - 1)], 1u);
    __syncthreads();
    hist[(size_t)blk * kBins + threadIdx.x] = s_h[threadIdx.x];
}

// (kin, vin) -> (kout, vout), all of at least n elements and the two pairs distinct
__device__ __forceinline__ void scatter_pass(const unsigned* __restrict__ kin, const unsigned* __restrict__ vin,
                                             unsigned* __restrict__ kout, unsigned* __restrict__ vout, int n, int nblk,
                                             int blk, int shift, const unsigned* __restrict__ hist) {
    __shared__ unsigned s_wcnt[kT / 64][kBins];  // this round's keys of digit d in wave w
    __shared__ unsigned s_off[kT / 64][kBins];   // where wave w's first key of digit d goes
    __shared__ unsigned s_wave[kT / 64];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long lo, hi;
    run_of(n, nblk, blk, lo, hi);
#pragma unroll
    for (int w = 0; w < kT / 64; ++w) s_wcnt[w][tid] = 0u;
    // digit tid: the keys in the runs before this one, and in the whole segment
    unsigned before = 0, all = 0;
    for (int i = 0; i < nblk; ++i) {
        const unsigned v = hist[(size_t)i * kBins + tid];
        all += v;
        before += i < blk ? v : 0u;
    }
    unsigned total;
    unsigned run = block_excl_scan<kT / 64, unsigned>(all, s_wave, total) + before;  // its barrier also covers s_wcnt's zeroes
    for (long long r0 = lo; r0 < hi; r0 += kTile) {
        const long long i = r0 + tid;
        const bool act = i < hi;
        const unsigned key = act ? kin[i] : 0u, val = act ? vin[i] : 0u;
        const unsigned d = (key >> shift) & (kBins - 1);
        unsigned long long peers = __ballot(act);  // the lanes of this wave with the same digit
#pragma unroll
        for (int bit = 0; bit < kDigitBits; ++bit) {
            const bool one = (d >> bit) & 1u;
            const unsigned long long bv = __ballot(act && one);
            peers &= one ? bv : ~bv;
        }
        const unsigned rank = (unsigned)__popcll(peers & ((1ull << lane) - 1ull));
        if (act && rank == 0u) s_wcnt[wave][d] = (unsigned)__popcll(peers);
        __syncthreads();
        {
            const unsigned c0 = s_wcnt[0][tid], c1 = s_wcnt[1][tid], c2 = s_wcnt[2][tid], c3 = s_wcnt[3][tid];
            s_off[0][tid] = run;
            s_off[1][tid] = run + c0;
            s_off[2][tid] = run + c0 + c1;
            s_off[3][tid] = run + c0 + c1 + c2;
            run += c0 + c1 + c2 + c3;
            s_wcnt[0][tid] = 0u, s_wcnt[1][tid] = 0u, s_wcnt[2][tid] = 0u, s_wcnt[3][tid] = 0u;
        }
        __syncthreads();
        if (act) {
            const unsigned dst = s_off[wave][d] + rank;
            if (dst < (unsigned)n) kout[dst] = key, vout[dst] = val;  // always: a permutation of [0, n)
        }
        // s_off is rewritten only after the next round's first barrier, s_wcnt written only after this one's second
    }
}

}  // namespace radix
}  // namespace nconv
