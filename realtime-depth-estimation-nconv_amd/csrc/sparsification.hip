// sparsification.hip — sparsification curves of a confidence plane (nconv_depth_sparsification): remove the
// least confident valid pixels step by step and sum the error of the rest, beside the oracle that removes
// the largest errors first. include/nconv.h states the definition as the contract.
//
// The hot part is a segmented, stable, least-significant-digit radix sort of (key32, pixel number) pairs.
// Image b has two segments, 2 b (confidence key) and 2 b + 1 (oracle key); all 2 B segments go through the
// same launches. Invalid pixels never enter the sort: the prepare step is a raster-order compaction (as in
// backproject.hip), so the n_b pairs of a segment start in ascending pixel number, and a stable sort by key
// then breaks ties by ascending pixel number without the pixel number being part of the key.
//
//   spars_count       valid pixels of every raster tile of kPrepTile pixels -> tilecnt[b][tile]
//   spars_prepare     per tile: its base (the sum of the tiles before it; the sum of all is n_b), then
//                     each valid pixel's two keys and its pixel number at its raster rank, and the terms
//                     a = |e|, q = e^2 at its pixel number
//   per digit (kPasses x):
//   spars_hist<j>     segment s is cut into nblk equal runs of whole sort tiles, one per workgroup (the run
//                     length follows from n_b, read on the device). A workgroup counts the digit of its run
//                     in LDS (integer atomics: counting only) and writes all kBins counts: nothing to zero
//   spars_scatter<j>  thread d sums column d of the segment's histograms (the runs before its own, and all),
//                     a scan over the workgroup gives digit d's base. Then, kTile keys at a time in run
//                     order, a key's rank among the equal digits is
//                       keys of earlier rounds (thread d's running count) + of lower waves of this round
//                       (a fixed wave-order prefix in LDS) + of lower lanes of its wave (ballots),
//                     never the order in which anything lands: the scatter is stable
//   spars_chunk_sums  the sorted pixel numbers -> order; a and q gathered in sorted order; one double
//                     partial pair per chunk of kChunk sorted positions
//   spars_curve       one workgroup per (segment, j): thread t starts from the term at position
//                     c kChunk + t (c = k_j / kChunk) where that position is in [k_j, n_b), else 0, adds the
//                     partials of chunks c + 1 + t, c + 1 + t + kT, .. in that order, and the kT values go
//                     through the same fixed tree as a chunk's terms (block_sum2)
//
// Twelve launches whatever the data, n_b and whether order is asked for; no global atomics, no floating
// atomics, no host synchronisation (capturable); every buffer is in the caller's workspace.
#include <algorithm>
#include "nconv_internal.h"

namespace nconv {

namespace {

constexpr int kT = 256;                  // threads: four waves
constexpr int kDigitBits = 8;            // digit width
constexpr int kBins = 1 << kDigitBits;   // one bin per thread
constexpr int kPasses = 32 / kDigitBits;
constexpr int kTile = kT;                // sort tile: the keys of one round, one per thread
constexpr int kMaxBlocks = 64;           // workgroups per segment
constexpr int kPrepPix = 8;              // consecutive pixels per thread in count / prepare
constexpr int kPrepTile = kT * kPrepPix;
constexpr int kChunk = kT;               // sorted positions per partial sum
static_assert(kBins == kT, "thread d owns digit d");
static_assert(kPasses == 4, "one hist and one scatter launch per digit");

struct Layout {
    int ntiles, nblk, nchunks;
    size_t hw;
    size_t part, keys0, vals0, keys1, vals1, ta, tq, hist, tilecnt, nvalid, bytes;
};

Layout layout_of(int B, int H, int W) {
    Layout l;
    l.hw = (size_t)H * W;
    l.ntiles = (int)((l.hw + kPrepTile - 1) / kPrepTile);
    l.nblk = (int)std::min<size_t>((l.hw + kTile - 1) / kTile, kMaxBlocks);
    l.nchunks = (int)((l.hw + kChunk - 1) / kChunk);
    const size_t seg = 2 * (size_t)B;
    size_t o = 0;
    l.part = o, o += seg * l.nchunks * 2 * sizeof(double);
    l.keys0 = o, o += seg * l.hw * 4;
    l.vals0 = o, o += seg * l.hw * 4;
    l.keys1 = o, o += seg * l.hw * 4;
    l.vals1 = o, o += seg * l.hw * 4;
    l.ta = o, o += (size_t)B * l.hw * 4;
    l.tq = o, o += (size_t)B * l.hw * 4;
    l.hist = o, o += seg * l.nblk * kBins * 4;
    l.tilecnt = o, o += (size_t)B * l.ntiles * 4;
    l.nvalid = o, o += (size_t)B * 4;
    l.bytes = (o + 7) & ~(size_t)7;
    return l;
}

struct Buffers {
    double* part;
    unsigned *keys0, *vals0, *keys1, *vals1;
    float *ta, *tq;
    unsigned *hist, *tilecnt;
    int* nvalid;
};

__device__ __forceinline__ bool valid_gt(const SparsificationArgs& A, float g) {
    return g > 0.f && g >= A.g_lo && g <= A.g_hi;
}

__device__ __forceinline__ float plane_at(const PlaneView& v, int b, unsigned row, unsigned col) {
    return v.image<float>(b)[(long long)row * v.rs + col];
}

// exclusive prefix of v over the workgroup's threads in thread order, and the total (wave_ops.h); a
// kernel's calls share s_wave
__device__ __forceinline__ unsigned excl_scan(unsigned v, unsigned& total) {
    __shared__ unsigned s_wave[kT / 64];
    return block_excl_scan<kT / 64, unsigned, true>(v, s_wave, total);
}

// wave_ops.h's tree over kT doubles, twice behind one barrier. Every thread returns with the totals.
__device__ __forceinline__ void block_sum2(double& x, double& y) {
    __shared__ double s_x[kT / 64], s_y[kT / 64];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    x = wave_sum(x), y = wave_sum(y);
    if (lane == 0) s_x[wave] = x, s_y[wave] = y;
    __syncthreads();
    x = waves_in_order(s_x), y = waves_in_order(s_y);
}

__global__ __launch_bounds__(kT) void spars_count(SparsificationArgs A, unsigned* __restrict__ tilecnt, int ntiles) {
    const int b = (int)blockIdx.x / ntiles, tile = (int)blockIdx.x - b * ntiles;
    const unsigned hw = (unsigned)A.H * (unsigned)A.W;  // < 2^31
    const unsigned p0 = (unsigned)tile * kPrepTile + threadIdx.x * kPrepPix;
    unsigned c = 0;
#pragma unroll
    for (int k = 0; k < kPrepPix; ++k) {
        const unsigned p = p0 + k;
        if (p < hw) {
            const unsigned row = p / (unsigned)A.W, col = p - row * (unsigned)A.W;
            c += valid_gt(A, plane_at(A.g, b, row, col)) ? 1u : 0u;
        }
    }
    unsigned total;
    excl_scan(c, total);
    if (threadIdx.x == 0) tilecnt[blockIdx.x] = total;
}

__global__ __launch_bounds__(kT) void spars_prepare(SparsificationArgs A, Buffers w, int ntiles) {
#pragma clang fp contract(off)
    const int b = (int)blockIdx.x / ntiles, tile = (int)blockIdx.x - b * ntiles;
    const unsigned hw = (unsigned)A.H * (unsigned)A.W;
    // the tiles before this one, and all of them
    unsigned bef = 0, all = 0;
    for (int i = (int)threadIdx.x; i < ntiles; i += kT) {
        const unsigned v = w.tilecnt[(size_t)b * ntiles + i];
        all += v;
        bef += i < tile ? v : 0u;
    }
    unsigned before, nb, tmp;
    excl_scan(bef, before);  // the totals are all this needs
    excl_scan(all, nb);
    if (tile == 0 && threadIdx.x == 0) w.nvalid[b] = (int)nb;

    const unsigned p0 = (unsigned)tile * kPrepTile + threadIdx.x * kPrepPix;
    unsigned ck[kPrepPix], ok[kPrepPix], mask = 0, c = 0;
#pragma unroll
    for (int k = 0; k < kPrepPix; ++k) {
        const unsigned p = p0 + k;
        ck[k] = 0, ok[k] = 0;
        if (p >= hw) continue;
        const unsigned row = p / (unsigned)A.W, col = p - row * (unsigned)A.W;
        const float g = plane_at(A.g, b, row, col);
        if (!valid_gt(A, g)) continue;
        float P = plane_at(A.p, b, row, col);  // comparisons, not fminf / fmaxf: a NaN stays NaN
        P = P < A.c_lo ? A.c_lo : P;
        P = P > A.c_hi ? A.c_hi : P;
        const float e = P - g, a = fabsf(e), q = e * e;
        const float cf = plane_at(A.c, b, row, col);
        const unsigned bits = __float_as_uint(cf);
        unsigned u = bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u);
        if (A.uncertainty) u = ~u;
        if (cf != cf) u = 0u;  // a NaN is removed first under either reading of the plane
        ck[k] = u, ok[k] = ~__float_as_uint(a);
        w.ta[(size_t)b * hw + p] = a;
        w.tq[(size_t)b * hw + p] = q;
        mask |= 1u << k, ++c;
    }
    unsigned r = before + excl_scan(c, tmp);
    const size_t s0 = (size_t)(2 * b) * hw, s1 = s0 + hw;
#pragma unroll
    for (int k = 0; k < kPrepPix; ++k) {
        if (!((mask >> k) & 1u)) continue;
        if (r < hw) {  // always: r < n_b <= H * W
            w.keys0[s0 + r] = ck[k], w.vals0[s0 + r] = p0 + k;
            w.keys0[s1 + r] = ok[k], w.vals0[s1 + r] = p0 + k;
        }
        ++r;
    }
}

// the run [lo, hi) of sorted positions that workgroup blk of nblk takes of a segment of n keys
__device__ __forceinline__ void run_of(int n, int nblk, int blk, long long& lo, long long& hi) {
    const long long per = ((long long)n + nblk - 1) / nblk;
    const long long run = (per + kTile - 1) / kTile * kTile;
    lo = (long long)blk * run < n ? (long long)blk * run : n;
    hi = lo + run < n ? lo + run : n;
}

template <int j>
__global__ __launch_bounds__(kT) void spars_hist(const unsigned* __restrict__ kin, const int* __restrict__ nvalid,
                                                 unsigned* __restrict__ hist, size_t hw, int nblk) {
    __shared__ unsigned s_h[kBins];
    const int seg = (int)blockIdx.x / nblk, blk = (int)blockIdx.x - seg * nblk;
    long long lo, hi;
    run_of(nvalid[seg >> 1], nblk, blk, lo, hi);
    s_h[threadIdx.x] = 0u;
    __syncthreads();
    const unsigned* k = kin + (size_t)seg * hw;
    for (long long i = lo + threadIdx.x; i < hi; i += kT) atomicAdd(&s_h[(k[i] >> (j * kDigitBits)) & (kBins - 1)], 1u);
    __syncthreads();
    hist[(size_t)blockIdx.x * kBins + threadIdx.x] = s_h[threadIdx.x];
}

template <int j>
__global__ __launch_bounds__(kT) void spars_scatter(const unsigned* __restrict__ kin, const unsigned* __restrict__ vin,
                                                    unsigned* __restrict__ kout, unsigned* __restrict__ vout,
                                                    const int* __restrict__ nvalid, const unsigned* __restrict__ hist,
                                                    size_t hw, int nblk) {
    __shared__ unsigned s_wcnt[kT / 64][kBins];  // this round's keys of digit d in wave w
    __shared__ unsigned s_off[kT / 64][kBins];   // where wave w's first key of digit d goes
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int seg = (int)blockIdx.x / nblk, blk = (int)blockIdx.x - seg * nblk;
    const int n = nvalid[seg >> 1];
    long long lo, hi;
    run_of(n, nblk, blk, lo, hi);
#pragma unroll
    for (int w = 0; w < kT / 64; ++w) s_wcnt[w][tid] = 0u;
    // digit tid: the keys in the runs before this one, and in the whole segment
    unsigned before = 0, all = 0;
    const unsigned* h = hist + (size_t)seg * nblk * kBins + tid;
    for (int i = 0; i < nblk; ++i) {
        const unsigned v = h[(size_t)i * kBins];
        all += v;
        before += i < blk ? v : 0u;
    }
    unsigned total;
    unsigned run = excl_scan(all, total) + before;  // its barriers also cover s_wcnt's zeroes
    const size_t sb = (size_t)seg * hw;
    for (long long r0 = lo; r0 < hi; r0 += kTile) {
        const long long i = r0 + tid;
        const bool act = i < hi;
        const unsigned key = act ? kin[sb + i] : 0u, val = act ? vin[sb + i] : 0u;
        const unsigned d = (key >> (j * kDigitBits)) & (kBins - 1);
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
            if (dst < (unsigned)n) kout[sb + dst] = key, vout[sb + dst] = val;  // always: a permutation of [0, n)
        }
        // s_off is rewritten only after the next round's first barrier, s_wcnt written only after this one's second
    }
}

__global__ __launch_bounds__(kT) void spars_chunk_sums(Buffers w, int* __restrict__ order, size_t hw, int nchunks) {
    const int seg = (int)blockIdx.x / nchunks, c = (int)blockIdx.x - seg * nchunks;
    const int b = seg >> 1, n = w.nvalid[b];
    const size_t i = (size_t)c * kChunk + threadIdx.x;
    const bool in = i < (size_t)n;
    const unsigned pix = in ? w.vals0[(size_t)seg * hw + i] : 0u;
    if (order && i < hw) order[(size_t)seg * hw + i] = in ? (int)pix : -1;
    double x = in ? (double)w.ta[(size_t)b * hw + pix] : 0.0;
    double y = in ? (double)w.tq[(size_t)b * hw + pix] : 0.0;
    block_sum2(x, y);
    if (threadIdx.x == 0) {
        w.part[((size_t)seg * nchunks + c) * 2] = x;
        w.part[((size_t)seg * nchunks + c) * 2 + 1] = y;
    }
}

__global__ __launch_bounds__(kT) void spars_curve(Buffers w, double* __restrict__ curves, size_t hw, int nchunks, int J) {
    const int seg = (int)blockIdx.x / J, j = (int)blockIdx.x - seg * J;
    const int b = seg >> 1, n = w.nvalid[b];
    const long long k = (long long)j * n / J;
    const long long c = k / kChunk;
    const long long i = c * kChunk + threadIdx.x;
    const bool in = i >= k && i < n;
    const unsigned pix = in ? w.vals0[(size_t)seg * hw + i] : 0u;
    double x = in ? (double)w.ta[(size_t)b * hw + pix] : 0.0;
    double y = in ? (double)w.tq[(size_t)b * hw + pix] : 0.0;
    const long long used = ((long long)n + kChunk - 1) / kChunk;  // the chunks that hold a term
    const double* part = w.part + (size_t)seg * nchunks * 2;
    for (long long cc = c + 1 + threadIdx.x; cc < used; cc += kT) {
        x += part[cc * 2];
        y += part[cc * 2 + 1];
    }
    block_sum2(x, y);
    if (threadIdx.x == 0) {
        double* out = curves + ((size_t)seg * J + j) * 3;
        out[0] = (double)(n - k);
        out[1] = x;
        out[2] = y;
    }
}

}  // namespace

size_t sparsification_workspace_bytes(int B, int H, int W) { return layout_of(B, H, W).bytes; }

int launch_depth_sparsification(const SparsificationArgs& a, void* workspace, hipStream_t st, const char** why) {
    const Layout l = layout_of(a.B, a.H, a.W);
    char* ws = (char*)workspace;
    Buffers w;
    w.part = (double*)(ws + l.part);
    w.keys0 = (unsigned*)(ws + l.keys0), w.vals0 = (unsigned*)(ws + l.vals0);
    w.keys1 = (unsigned*)(ws + l.keys1), w.vals1 = (unsigned*)(ws + l.vals1);
    w.ta = (float*)(ws + l.ta), w.tq = (float*)(ws + l.tq);
    w.hist = (unsigned*)(ws + l.hist), w.tilecnt = (unsigned*)(ws + l.tilecnt);
    w.nvalid = (int*)(ws + l.nvalid);
    // every grid below is at most 2 * B * ceil(H * W / kT) < 2^31 (B * H * W < 2^31)
    const dim3 blk(kT), gprep((unsigned)((long long)a.B * l.ntiles)), gsort((unsigned)(2LL * a.B * l.nblk));
    hipLaunchKernelGGL(spars_count, gprep, blk, 0, st, a, w.tilecnt, l.ntiles);
    hipLaunchKernelGGL(spars_prepare, gprep, blk, 0, st, a, w, l.ntiles);
    hipLaunchKernelGGL(spars_hist<0>, gsort, blk, 0, st, w.keys0, w.nvalid, w.hist, l.hw, l.nblk);
    hipLaunchKernelGGL(spars_scatter<0>, gsort, blk, 0, st, w.keys0, w.vals0, w.keys1, w.vals1, w.nvalid, w.hist, l.hw, l.nblk);
    hipLaunchKernelGGL(spars_hist<1>, gsort, blk, 0, st, w.keys1, w.nvalid, w.hist, l.hw, l.nblk);
    hipLaunchKernelGGL(spars_scatter<1>, gsort, blk, 0, st, w.keys1, w.vals1, w.keys0, w.vals0, w.nvalid, w.hist, l.hw, l.nblk);
    hipLaunchKernelGGL(spars_hist<2>, gsort, blk, 0, st, w.keys0, w.nvalid, w.hist, l.hw, l.nblk);
    hipLaunchKernelGGL(spars_scatter<2>, gsort, blk, 0, st, w.keys0, w.vals0, w.keys1, w.vals1, w.nvalid, w.hist, l.hw, l.nblk);
    hipLaunchKernelGGL(spars_hist<3>, gsort, blk, 0, st, w.keys1, w.nvalid, w.hist, l.hw, l.nblk);
    hipLaunchKernelGGL(spars_scatter<3>, gsort, blk, 0, st, w.keys1, w.vals1, w.keys0, w.vals0, w.nvalid, w.hist, l.hw, l.nblk);
    hipLaunchKernelGGL(spars_chunk_sums, dim3((unsigned)(2LL * a.B * l.nchunks)), blk, 0, st, w, a.order, l.hw, l.nchunks);
    hipLaunchKernelGGL(spars_curve, dim3((unsigned)(2LL * a.B * a.steps)), blk, 0, st, w, a.curves, l.hw, l.nchunks, a.steps);
    return launch_status(why);
}

}  // namespace nconv
