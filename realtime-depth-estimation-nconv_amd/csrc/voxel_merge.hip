// voxel_merge.hip — per-frame point clouds merged into one voxel-grid map (nconv_voxel_merge): every point goes
// to the world frame by its segment's pose, points of one grid cell become one output row holding their weighted
// mean position, colour and normal, and the rows come out in ascending cell number. include/nconv.h states the
// rule operation by operation as the contract.
//
// The hot part is radix_pass.h's stable LSD radix sort of (cell number, rank) pairs. Points that are dropped
// (outside the box, not finite, weight <= 0, in no segment) never enter it: the prepare step is a raster-order
// compaction (as in backproject.hip and sparsification.hip), so the pairs start in ascending input row and the
// stable sort keeps the rows of one cell in that order without the row being part of the key.
//
//   vox_count     inside points of every tile of kPrepTile input rows -> tilecnt[tile]
//   vox_prepare   per tile: its base (the sum of the tiles before it; the sum of all is n_inside), then each
//                 inside point's cell number and rank, and at its rank the world point, the rotated normal, the
//                 packed colour and the weight; stats[1..3]
//   per digit (P = ceil(bits(nx ny nz - 1) / 8) times, known from dims on the host):
//   vox_hist, vox_scatter   radix_pass.h, kSortBlocks workgroups
//   vox_heads     per chunk of kChunk sorted positions: the number of run heads (a position whose key differs
//                 from the one before it) -> chunkcnt[chunk]; and where the chunk's first key continues the run of
//                 the chunk before, the sums of that leading piece -> lead[chunk]
//   vox_scan      one workgroup: the exclusive prefix of chunkcnt -> chunkbase, the total -> stats[0]
//   vox_combine   per chunk: every run head sums its run's terms inside the chunk left to right, adds the leading
//                 pieces of the following chunks while their first key is its own, divides and writes output
//                 row chunkbase[chunk] + (heads before it in the chunk)
//
// The terms of a chunk are gathered through the sorted ranks into LDS by all threads at once (independent
// loads); the double sums then walk LDS, not a chain of dependent global loads. A thread adds at most kChunk
// terms of its own chunk and one leading piece per following chunk: kChunk + N / kChunk additions per sum.
// 5 + 2 P launches whatever the data; no global atomics, no floating atomics, no host synchronisation
// (capturable); every buffer is in the caller's workspace.
#include <algorithm>
#include "radix_pass.h"
#include "warp_common.h"

namespace nconv {

namespace {

using radix::kT;
constexpr int kSortBlocks = 256;          // workgroups per sort pass (at most)
constexpr int kPrepPts = 4;               // consecutive input rows per thread in count / prepare
constexpr int kPrepTile = kT * kPrepPts;
constexpr int kChunk = kT;                // sorted positions per chunk, one per thread
constexpr int kSums = 9;                  // the double sums of a run: w p (3), w c (3), w n (3)

struct Layout {
    int ntiles, nblk, nchunks;
    size_t lead, leadw, keys0, vals0, keys1, vals1, wp, wn, wt, col, hist, tilecnt, chunkcnt, chunkbase, nin, bytes;
};

Layout layout_of(long long N) {
    Layout l;
    const size_t cap = (size_t)std::max<long long>(N, 1);
    l.ntiles = (int)((cap + kPrepTile - 1) / kPrepTile);
    l.nblk = (int)std::min<size_t>((cap + radix::kTile - 1) / radix::kTile, kSortBlocks);
    l.nchunks = (int)((cap + kChunk - 1) / kChunk);
    size_t o = 0;
    l.lead = o, o += (size_t)l.nchunks * kSums * sizeof(double);
    l.leadw = o, o += (size_t)l.nchunks * sizeof(long long);
    l.keys0 = o, o += cap * 4;
    l.vals0 = o, o += cap * 4;
    l.keys1 = o, o += cap * 4;
    l.vals1 = o, o += cap * 4;
    l.wp = o, o += cap * 12;
    l.wn = o, o += cap * 12;
    l.wt = o, o += cap * 4;
    l.col = o, o += cap * 4;
    l.hist = o, o += (size_t)l.nblk * radix::kBins * 4;
    l.tilecnt = o, o += (size_t)l.ntiles * 4;
    l.chunkcnt = o, o += (size_t)l.nchunks * 4;
    l.chunkbase = o, o += (size_t)l.nchunks * 4;
    l.nin = o, o += 4;
    l.bytes = (o + 7) & ~(size_t)7;
    return l;
}

struct Buffers {
    double* lead;        // [chunk][kSums]
    long long* leadw;    // [chunk]
    unsigned *keys0, *vals0, *keys1, *vals1;
    float *wp, *wn;      // [rank][3]: the world point, the rotated normal
    int* wt;             // [rank]
    unsigned* col;       // [rank]: r | g << 8 | b << 16
    unsigned *hist, *tilecnt, *chunkcnt, *chunkbase;
    int* nin;            // n_inside
};

// exclusive prefix of v over the workgroup's threads in thread order, and the total (wave_ops.h); a
// kernel's calls share s_wave
__device__ __forceinline__ unsigned excl_scan(unsigned v, unsigned& total) {
    __shared__ unsigned s_wave[kT / 64];
    return block_excl_scan<kT / 64, unsigned, true>(v, s_wave, total);
}

// the segment of input row i: the number of offsets[0 .. S] that are <= i, minus one, by bisection (offsets is
// non-decreasing); -1 where that is no segment (i < offsets[0] or i >= offsets[S])
__device__ __forceinline__ int segment_of(const VoxelArgs& a, long long i) {
    if (!a.offsets) return 0;
    int lo = 0, hi = a.S + 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((long long)a.offsets[mid] <= i) lo = mid + 1;
        else hi = mid;
    }
    return lo >= 1 && lo <= a.S ? lo - 1 : -1;
}

// (r0 x + r1 y) + r2 z: warp_dot without the translation (a normal is rotated, not moved)
__device__ __forceinline__ float rot_dot(const float (&r)[4], float x, float y, float z) {
#pragma clang fp contract(off)
    const float p0 = r[0] * x, p1 = r[1] * y, p2 = r[2] * z;
    const float s01 = p0 + p1;
    return s01 + p2;
}

// floorf((p - o) / voxel) of one axis; inside iff 0 <= f < n as floats (a NaN or an infinity fails)
__device__ __forceinline__ bool axis_cell(float p, float o, float voxel, int n, int& idx) {
#pragma clang fp contract(off)
    const float d = p - o;
    const float q = __fdiv_rn(d, voxel);
    const float f = floorf(q);
    const bool ok = f >= 0.f && f < (float)n;
    idx = ok ? (int)f : 0;
    return ok;
}

struct Point {
    bool in;
    int key, seg, w;
    float p[3];
    Proj m;  // the segment's [R | t] (read where seg >= 0 and there are poses)
};

// input row i < N: its segment, world point, weight, and whether it is inside, with its cell number
__device__ __forceinline__ Point classify(const VoxelArgs& a, long long i) {
    Point q;
    q.seg = segment_of(a, i);
    q.w = a.w ? a.w[i] : 1;
    const float* x = a.xyz + i * a.xs;
    const float x0 = x[0], x1 = x[1], x2 = x[2];
    q.p[0] = x0, q.p[1] = x1, q.p[2] = x2;
    if (a.poses && q.seg >= 0) {
        const float* m = a.poses + (long long)q.seg * 12;
#pragma unroll
        for (int k = 0; k < 12; ++k) q.m.r[k / 4][k % 4] = m[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) q.p[k] = warp_dot(q.m.r[k], x0, x1, x2);
    }
    int ix, iy, iz;
    const bool bx = axis_cell(q.p[0], a.ox, a.voxel, a.nx, ix);
    const bool by = axis_cell(q.p[1], a.oy, a.voxel, a.ny, iy);
    const bool bz = axis_cell(q.p[2], a.oz, a.voxel, a.nz, iz);
    q.in = q.seg >= 0 && q.w > 0 && bx && by && bz;
    q.key = (iz * a.ny + iy) * a.nx + ix;  // < nx ny nz < 2^31
    return q;
}

__global__ __launch_bounds__(kT) void vox_count(VoxelArgs a, unsigned* __restrict__ tilecnt) {
    const long long i0 = (long long)blockIdx.x * kPrepTile + threadIdx.x * kPrepPts;
    unsigned c = 0;
#pragma unroll
    for (int k = 0; k < kPrepPts; ++k) {
        if (i0 + k < a.N) c += classify(a, i0 + k).in ? 1u : 0u;
    }
    unsigned total;
    excl_scan(c, total);
    if (threadIdx.x == 0) tilecnt[blockIdx.x] = total;
}

__global__ __launch_bounds__(kT) void vox_prepare(VoxelArgs a, Buffers w, int ntiles) {
    const int tile = (int)blockIdx.x;
    // the tiles before this one, and all of them
    unsigned bef = 0, all = 0;
    for (int i = (int)threadIdx.x; i < ntiles; i += kT) {
        const unsigned v = w.tilecnt[i];
        all += v;
        bef += i < tile ? v : 0u;
    }
    unsigned before, nin, tmp;
    excl_scan(bef, before);  // the totals are all this needs
    excl_scan(all, nin);
    if (tile == 0 && threadIdx.x == 0) {
        w.nin[0] = (int)nin;
        a.stats[1] = (int)nin, a.stats[2] = (int)(a.N - (long long)nin), a.stats[3] = 0;
    }
    const long long i0 = (long long)tile * kPrepTile + threadIdx.x * kPrepPts;
    Point pt[kPrepPts];
    unsigned c = 0;
#pragma unroll
    for (int k = 0; k < kPrepPts; ++k) {
        pt[k].in = false;
        if (i0 + k < a.N) pt[k] = classify(a, i0 + k);
        c += pt[k].in ? 1u : 0u;
    }
    long long r = (long long)before + excl_scan(c, tmp);
#pragma unroll
    for (int k = 0; k < kPrepPts; ++k) {
        if (!pt[k].in) continue;
        if (r < a.N) {  // always: r < n_inside <= N
            const long long i = i0 + k;
            w.keys0[r] = (unsigned)pt[k].key, w.vals0[r] = (unsigned)r;
            w.wp[r * 3] = pt[k].p[0], w.wp[r * 3 + 1] = pt[k].p[1], w.wp[r * 3 + 2] = pt[k].p[2];
            w.wt[r] = pt[k].w;
            if (a.rgb) {
                const unsigned char* c3 = a.rgb + i * a.cs;
                w.col[r] = (unsigned)c3[0] | (unsigned)c3[1] << 8 | (unsigned)c3[2] << 16;
            }
            if (a.nrm) {
                const float* n3 = a.nrm + i * a.ns;
                float n0 = n3[0], n1 = n3[1], n2 = n3[2];
                if (a.poses) {
                    const float x = n0, y = n1, z = n2;
                    n0 = rot_dot(pt[k].m.r[0], x, y, z), n1 = rot_dot(pt[k].m.r[1], x, y, z);
                    n2 = rot_dot(pt[k].m.r[2], x, y, z);
                }
                w.wn[r * 3] = n0, w.wn[r * 3 + 1] = n1, w.wn[r * 3 + 2] = n2;
            }
        }
        ++r;
    }
}

__global__ __launch_bounds__(kT) void vox_hist(const unsigned* __restrict__ kin, const int* __restrict__ nin,
                                               unsigned* __restrict__ hist, int nblk, int shift) {
    radix::hist_pass(kin, nin[0], nblk, (int)blockIdx.x, shift, hist);
}

__global__ __launch_bounds__(kT) void vox_scatter(const unsigned* __restrict__ kin, const unsigned* __restrict__ vin,
                                                  unsigned* __restrict__ kout, unsigned* __restrict__ vout,
                                                  const int* __restrict__ nin, const unsigned* __restrict__ hist,
                                                  int nblk, int shift) {
    radix::scatter_pass(kin, vin, kout, vout, nin[0], nblk, (int)blockIdx.x, shift, hist);
}

// a chunk's keys, weights and term values in LDS, by sorted position inside the chunk
struct Stage {
    unsigned key[kChunk];
    int w[kChunk];
    float v[kSums][kChunk];
};

// position t of the chunk holds the point of rank r
__device__ __forceinline__ void stage_point(Stage& s, const Buffers& b, int t, unsigned r, bool rgb, bool nrm) {
    s.w[t] = b.wt[r];
#pragma unroll
    for (int k = 0; k < 3; ++k) s.v[k][t] = b.wp[(size_t)r * 3 + k];
    if (rgb) {
        const unsigned c = b.col[r];
        s.v[3][t] = (float)(c & 255u), s.v[4][t] = (float)((c >> 8) & 255u), s.v[5][t] = (float)((c >> 16) & 255u);
    }
    if (nrm) {
#pragma unroll
        for (int k = 0; k < 3; ++k) s.v[6 + k][t] = b.wn[(size_t)r * 3 + k];
    }
}

// whether position i (thread t of its chunk, key in s.key[t]) starts a run
__device__ __forceinline__ bool run_head(const Stage& s, const unsigned* __restrict__ keys, long long i, int t, int n) {
    if (i >= n) return false;
    if (i == 0) return true;
    const unsigned prev = t > 0 ? s.key[t - 1] : keys[i - 1];
    return prev != s.key[t];
}

__global__ __launch_bounds__(kT) void vox_heads(const unsigned* __restrict__ keys, const unsigned* __restrict__ vals,
                                                Buffers b, int rgb, int nrm) {
#pragma clang fp contract(off)
    __shared__ Stage s;
    const int c = (int)blockIdx.x, t = (int)threadIdx.x, n = b.nin[0];
    const long long i = (long long)c * kChunk + t;
    s.key[t] = i < n ? keys[i] : 0u;
    __syncthreads();
    unsigned heads;
    excl_scan(run_head(s, keys, i, t, n) ? 1u : 0u, heads);
    if (t == 0) b.chunkcnt[c] = heads;
    // the leading piece: only where the first key continues the run of the chunk before
    const long long first = (long long)c * kChunk;
    if (c == 0 || first >= n || keys[first - 1] != s.key[0]) return;  // the whole workgroup
    const bool mine = i < n && s.key[t] == s.key[0];  // sorted: the first `len` positions
    if (mine) stage_point(s, b, t, vals[i], rgb != 0, nrm != 0);
    unsigned len;
    excl_scan(mine ? 1u : 0u, len);  // its barriers also cover the staging
    // lane q of wave 0 adds sum q left to right; lane kSums adds the weights
    if (t <= kSums) {
        const int q = t < kSums ? t : 0;
        const bool used = t == kSums || q < 3 || (q < 6 ? rgb != 0 : nrm != 0);
        double acc = 0.0;
        long long W = 0;
        if (used) {
            for (unsigned u = 0; u < len; ++u) {
                const int wu = s.w[u];
                const double term = (double)wu * (double)s.v[q][u];
                acc = acc + term;
                W += wu;
            }
        }
        if (t == kSums) b.leadw[c] = W;
        else b.lead[(size_t)c * kSums + q] = acc;
    }
}

__global__ __launch_bounds__(kT) void vox_scan(Buffers b, int nchunks, int* __restrict__ stats) {
    const int per = (nchunks + kT - 1) / kT;
    const int lo = min((int)threadIdx.x * per, nchunks), hi = min(lo + per, nchunks);
    unsigned sum = 0;
    for (int i = lo; i < hi; ++i) sum += b.chunkcnt[i];
    unsigned total;
    unsigned run = excl_scan(sum, total);
    for (int i = lo; i < hi; ++i) {
        b.chunkbase[i] = run;
        run += b.chunkcnt[i];
    }
    if (threadIdx.x == 0) stats[0] = (int)total;
}

__global__ __launch_bounds__(kT) void vox_combine(const unsigned* __restrict__ keys, const unsigned* __restrict__ vals,
                                                  Buffers b, VoxelArgs a) {
#pragma clang fp contract(off)
    __shared__ Stage s;
    const int c = (int)blockIdx.x, t = (int)threadIdx.x, n = b.nin[0];
    const long long first = (long long)c * kChunk, i = first + t;
    if (first >= n) return;  // the whole workgroup
    const bool rgb = a.rgb != nullptr, nrm = a.nrm != nullptr;
    s.key[t] = i < n ? keys[i] : 0u;
    if (i < n) stage_point(s, b, t, vals[i], rgb, nrm);
    __syncthreads();
    const bool head = run_head(s, keys, i, t, n);
    unsigned tmp;
    const long long m = (long long)b.chunkbase[c] + excl_scan(head ? 1u : 0u, tmp);
    if (!head) return;
    const unsigned key = s.key[t];
    const int limit = n - first < kChunk ? (int)(n - first) : kChunk;
    double acc[kSums];
#pragma unroll
    for (int q = 0; q < kSums; ++q) acc[q] = 0.0;
    long long W = 0;
    int u = t;
    for (; u < limit && s.key[u] == key; ++u) {  // the run inside this chunk, left to right
        const int wu = s.w[u];
        const double dw = (double)wu;
        W += wu;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const double term = dw * (double)s.v[q][u];
            acc[q] = acc[q] + term;
        }
        if (rgb) {
#pragma unroll
            for (int q = 3; q < 6; ++q) {
                const double term = dw * (double)s.v[q][u];
                acc[q] = acc[q] + term;
            }
        }
        if (nrm) {
#pragma unroll
            for (int q = 6; q < 9; ++q) {
                const double term = dw * (double)s.v[q][u];
                acc[q] = acc[q] + term;
            }
        }
    }
    if (u == kChunk) {  // the run reaches the chunk's end: the leading pieces of the chunks it goes on in
        for (long long cc = c + 1; cc * kChunk < n && keys[cc * kChunk] == key; ++cc) {
            W += b.leadw[cc];
#pragma unroll
            for (int q = 0; q < kSums; ++q) {
                if (q < 3 || (q < 6 ? rgb : nrm)) acc[q] = acc[q] + b.lead[(size_t)cc * kSums + q];
            }
        }
    }
    if (m >= a.cap) return;
    const double dW = (double)W;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double mean = acc[k] / dW;
        a.oxyz[m * 3 + k] = (float)mean;
    }
    if (rgb) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double mean = acc[3 + k] / dW;
            a.orgb[m * 3 + k] = (unsigned char)rint(mean);  // half to even; inside [0, 255]
        }
    }
    if (nrm) {
        float nv[3];
        const bool unit = unit_vector((float)acc[6], (float)acc[7], (float)acc[8], nv);
#pragma unroll
        for (int k = 0; k < 3; ++k) a.onrm[m * 3 + k] = unit ? nv[k] : 0.f;
    }
    a.ocount[m] = W > 0x7fffffffLL ? 0x7fffffff : (int)W;
    a.okey[m] = (int)key;
}

int passes_of(int nx, int ny, int nz) { return radix::passes_for((unsigned)((long long)nx * ny * nz - 1)); }

}  // namespace

size_t voxel_merge_workspace_bytes(long long N) { return layout_of(N).bytes; }

int launch_voxel_merge(const VoxelArgs& a, void* workspace, hipStream_t st, const char** why) {
    const Layout l = layout_of(a.N);
    char* ws = (char*)workspace;
    Buffers w;
    w.lead = (double*)(ws + l.lead), w.leadw = (long long*)(ws + l.leadw);
    w.keys0 = (unsigned*)(ws + l.keys0), w.vals0 = (unsigned*)(ws + l.vals0);
    w.keys1 = (unsigned*)(ws + l.keys1), w.vals1 = (unsigned*)(ws + l.vals1);
    w.wp = (float*)(ws + l.wp), w.wn = (float*)(ws + l.wn);
    w.wt = (int*)(ws + l.wt), w.col = (unsigned*)(ws + l.col);
    w.hist = (unsigned*)(ws + l.hist), w.tilecnt = (unsigned*)(ws + l.tilecnt);
    w.chunkcnt = (unsigned*)(ws + l.chunkcnt), w.chunkbase = (unsigned*)(ws + l.chunkbase);
    w.nin = (int*)(ws + l.nin);
    // every grid is at most ceil(N / kT) < 2^23 (N < 2^31)
    const dim3 blk(kT), gprep((unsigned)l.ntiles), gsort((unsigned)l.nblk), gchunk((unsigned)l.nchunks);
    hipLaunchKernelGGL(vox_count, gprep, blk, 0, st, a, w.tilecnt);
    hipLaunchKernelGGL(vox_prepare, gprep, blk, 0, st, a, w, l.ntiles);
    unsigned *kin = w.keys0, *vin = w.vals0, *kout = w.keys1, *vout = w.vals1;
    const int passes = passes_of(a.nx, a.ny, a.nz);
    for (int j = 0; j < passes; ++j) {
        hipLaunchKernelGGL(vox_hist, gsort, blk, 0, st, kin, w.nin, w.hist, l.nblk, j * radix::kDigitBits);
        hipLaunchKernelGGL(vox_scatter, gsort, blk, 0, st, kin, vin, kout, vout, w.nin, w.hist, l.nblk,
                           j * radix::kDigitBits);
        std::swap(kin, kout), std::swap(vin, vout);
    }
    hipLaunchKernelGGL(vox_heads, gchunk, blk, 0, st, kin, vin, w, a.rgb ? 1 : 0, a.nrm ? 1 : 0);
    hipLaunchKernelGGL(vox_scan, dim3(1), blk, 0, st, w, l.nchunks, a.stats);
    hipLaunchKernelGGL(vox_combine, gchunk, blk, 0, st, kin, vin, w, a);
    return launch_status(why);
}

}  // namespace nconv
