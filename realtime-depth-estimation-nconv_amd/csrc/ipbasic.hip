// ipbasic.hip — classical depth completion of a sparse depth plane (nconv_depth_ipbasic): IP-Basic's
// fill_in_fast (Ku, Harakeh, Waslander, CRV 2018), the non-learned baseline beside the NConv networks.
// include/nconv.h states the rule as the contract; T = 0.1f, valid v > T, empty v < T:
//   0 invert   v0 = sample(d) ? max_depth - d : 0       sample: d finite, d > T, max_depth - d > T
//   1 dilate   v1 = max of v0 over the custom footprint (full / cross / diamond, size 3, 5 or 7)
//   2 close    v2 = erode5(dilate5(v1))
//   3 fill     v3 = empty(v2) ? dilate7(v2) : v2
//   4 extrapolate (optional)  v3e = the column's top valid value above it; v4 = empty(v3e) ? dilate31(v3e) : v3e
//   5 median   v5 = the 13th smallest of the 5 x 5 window of v4, replicate border
//   6 blur     v6 = valid(v5) ? gauss5(v5), reflect-101 border, horizontal pass first : v5
//   7 back     out = valid(v6) ? max_depth - v6 : 0; keep_samples: sample(d) ? d : out
// Pixels outside the image take no part in a dilation or an erosion.
//
//   ipbasic_tile<kAll>     without extrapolate, the whole chain in one launch. A workgroup takes a tile of
//     kTH x kTW pixels, stages v0 of the tile and a halo of 14 (3 + 2 + 2 + 3 + 2 + 2) once through the
//     strided view of plane_io.h and runs every stage between two LDS buffers, each stage on the tile
//     grown by the radius the later stages still need; it writes the tile once. The regions are sized
//     for the largest custom kernel (7), so every extent is a compile-time constant.
//   ipbasic_top_reset, ipbasic_tile<kFront>, ipbasic_tile<kBack>     with extrapolate: top(x) is
//     column-global. kFront is stages 0 to 3 (halo 10) into the workspace plane; each workgroup finds the
//     first valid row of its tile's columns and merges it into top with an integer atomicMin on the row
//     number, whose result does not depend on the order. kBack stages the extrapolated read of the
//     workspace with a halo of 19 (15 + 2 + 2), fills with the 31 x 31 dilation and runs stages 5 to 7.
//
// All values are finite and >= 0 from stage 0 on (+inf stands outside the image before the erosion), so
// their order is the order of their bit patterns as unsigned integers: the dilations, the erosion and the
// median work on the bits with integer min / max. The full-kernel dilations and the erosion are
// separable: a row pass into the other buffer, then a column pass. Outside the image a stage writes the
// next stage's neutral element (0 before a dilation, +inf before the erosion); the median and the blur
// read only in-image coordinates (clamped or reflected), which lie inside the staged region.
// The median is forgetful selection over registers: of 14 values the smallest and the largest cannot be
// the median of 25, so they are dropped and the next value taken in, down to three; every index is a
// compile-time constant (no scratch).
#include <limits.h>
#include "nconv_internal.h"
#include "plane_io.h"

namespace nconv {

namespace {

constexpr int kT = 512;             // threads: eight waves
constexpr int kTH = 64, kTW = 64;   // the tile
constexpr float kThr = 0.1f;        // T
constexpr unsigned kInfBits = 0x7f800000u;
enum { kAll = 0, kFront = 1, kBack = 2 };

__device__ __forceinline__ unsigned bits_of(float v) { return __builtin_bit_cast(unsigned, v); }
__device__ __forceinline__ float float_of(unsigned u) { return __builtin_bit_cast(float, u); }
__device__ __forceinline__ bool valid_bits(unsigned u) { return float_of(u) > kThr; }
__device__ __forceinline__ bool empty_bits(unsigned u) { return float_of(u) < kThr; }

// stage 0: the inverted value of a source pixel, +0.0 where it is no sample
__device__ __forceinline__ bool is_sample(float d, float max_depth) {
    return __builtin_isfinite(d) && d > kThr && (max_depth - d) > kThr;
}
__device__ __forceinline__ unsigned invert(float d, float max_depth) {
    return is_sample(d, max_depth) ? bits_of(max_depth - d) : 0u;
}

// reflect-101 folded until inside [0, n)
__device__ __forceinline__ int reflect101(int i, int n) {
    if (n == 1) return 0;
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * (n - 1) - i;
    return i;
}

// one pass of the blur: (((w0 a0 + w1 a1) + w2 a2) + w3 a3) + w4 a4, every product and sum rounded on its
// own. 0.375 a is not exact in general (3 a needs two more bits), so a fused multiply-add would differ.
__device__ __forceinline__ float gauss5(float a0, float a1, float a2, float a3, float a4) {
#pragma clang fp contract(off)
    const float p0 = 0.0625f * a0, p1 = 0.25f * a1, p2 = 0.375f * a2, p3 = 0.25f * a3, p4 = 0.0625f * a4;
    return (((p0 + p1) + p2) + p3) + p4;
}

__device__ __forceinline__ void order2(unsigned& lo, unsigned& hi) {
    const unsigned a = min(lo, hi), b = max(lo, hi);
    lo = a, hi = b;
}

// The median of w[0 .. 25): forgetful selection, see the head of the file.
__device__ __forceinline__ unsigned median25(const unsigned (&w)[25]) {
    unsigned a[14];
#pragma unroll
    for (int i = 0; i < 14; ++i) a[i] = w[i];
#pragma unroll
    for (int k = 14; k >= 3; --k) {
        // the largest of a[0 .. k) to a[k - 1], then the smallest to a[0]
#pragma unroll
        for (int i = 0; i + 1 < k; ++i) order2(a[i], a[i + 1]);
#pragma unroll
        for (int i = k - 2; i >= 1; --i) order2(a[i - 1], a[i]);
        if (k > 3) a[0] = w[14 + (14 - k)];  // the next value replaces the smallest; a[k - 1] is dropped
    }
    return a[1];
}

// Local coordinates (ly, lx) of the staged buffers over the tile grown by ER rows and EC columns.
#define IPB_REGION(ER, EC, ly, lx)                                                       \
    for (int i_ = tid; i_ < (kTH + 2 * (ER)) * (kTW + 2 * (EC)); i_ += kT)              \
        if (const int ly = HALO - (ER) + i_ / (kTW + 2 * (EC)), lx = HALO - (EC) + i_ % (kTW + 2 * (EC)); true)

// out = max (MAX) or min over the row window of radius R of in, on the tile grown by (ER, EC)
template <int HALO, int ER, int EC, int R, bool MAX>
__device__ __forceinline__ void row_pass(const unsigned* in, unsigned* out, int tid) {
    constexpr int P = kTW + 2 * HALO;
    static_assert(EC + R <= HALO && ER <= HALO, "the window stays inside the staged buffer");
    IPB_REGION(ER, EC, ly, lx) {
        const unsigned* p = in + ly * P + lx;
        unsigned m = p[-R];
#pragma unroll
        for (int d = -R + 1; d <= R; ++d) m = MAX ? max(m, p[d]) : min(m, p[d]);
        out[ly * P + lx] = m;
    }
}

// the same over the column window of radius R, at one position
template <int P, int R, bool MAX>
__device__ __forceinline__ unsigned col_window(const unsigned* p) {
    unsigned m = p[-R * P];
#pragma unroll
    for (int d = -R + 1; d <= R; ++d) m = MAX ? max(m, p[d * P]) : min(m, p[d * P]);
    return m;
}

template <int MODE>
struct Geo {
    static constexpr int R3 = MODE == kFront ? 0 : 4;           // what the stages after v3 still need
    static constexpr int HALO = MODE == kBack ? 19 : R3 + 10;   // 3 + 2 + 2 + 3 before v3; 15 + 4 for kBack
    static constexpr int P = kTW + 2 * HALO, ROWS = kTH + 2 * HALO;
};

__global__ __launch_bounds__(256) void ipbasic_top_reset(int* __restrict__ top, unsigned n) {
    const unsigned t = blockIdx.x * 256u + threadIdx.x;  // n = B * W < 2^31
    if (t < n) top[t] = INT_MAX;
}

template <int MODE>
__global__ __launch_bounds__(kT) void ipbasic_tile(IpbasicArgs a) {
    constexpr int R3 = Geo<MODE>::R3, HALO = Geo<MODE>::HALO, P = Geo<MODE>::P, ROWS = Geo<MODE>::ROWS;
    __shared__ unsigned sA[ROWS * P], sB[ROWS * P];
    const int tid = (int)threadIdx.x;
    const int H = a.H, W = a.W;
    const TileOrigin o = tile_origin<kTH, kTW>(H, W);
    const int b = o.b, oy = o.i0 - HALO, ox = o.j0 - HALO;  // the image coordinates of local (0, 0)
    const __amdgpu_buffer_rsrc_t r = plane_rsrc(a.s.image<float>(b), view_bytes(H, a.s.rs, W, 4));
    auto inside = [&](int ly, int lx) {
        return (unsigned)(oy + ly) < (unsigned)H && (unsigned)(ox + lx) < (unsigned)W;
    };
    auto src_off = [&](int ly, int lx) {  // below 2^31: the view's extent is
        return (unsigned)((long long)(oy + ly) * a.s.rs + (ox + lx)) * 4u;
    };

    if constexpr (MODE != kBack) {
        constexpr int E1 = R3 + 7, E2A = R3 + 5, E2 = R3 + 3;
        // 0. invert: v0 of the tile and its halo to sA, 0 outside the image
        IPB_REGION(HALO, HALO, ly, lx) {
            const bool in = inside(ly, lx);
            const float d = ld_f32(r, in ? src_off(ly, lx) : kOOB);
            sA[ly * P + lx] = in ? invert(d, a.max_depth) : 0u;
        }
        __syncthreads();
        // 1. the custom dilation: v1 to sB
        {
            const int r1 = a.r1, shape = a.shape;
            IPB_REGION(E1, E1, ly, lx) {
                unsigned m = 0u;
                for (int dy = -r1; dy <= r1; ++dy) {
                    const int ext = shape == NCONV_IPBASIC_FULL    ? r1
                                    : shape == NCONV_IPBASIC_CROSS ? (dy == 0 ? r1 : 0)
                                                                   : r1 - (dy < 0 ? -dy : dy);
                    const unsigned* p = sA + (ly + dy) * P + lx;
                    for (int dx = -ext; dx <= ext; ++dx) m = max(m, p[dx]);
                }
                sB[ly * P + lx] = inside(ly, lx) ? m : 0u;
            }
        }
        __syncthreads();
        // 2. close: dilate 5 (+inf outside the image for the erosion), erode 5
        row_pass<HALO, E1, E2A, 2, true>(sB, sA, tid);
        __syncthreads();
        IPB_REGION(E2A, E2A, ly, lx)
            sB[ly * P + lx] = inside(ly, lx) ? col_window<P, 2, true>(sA + ly * P + lx) : kInfBits;
        __syncthreads();
        row_pass<HALO, E2A, E2, 2, false>(sB, sA, tid);
        __syncthreads();
        IPB_REGION(E2, E2, ly, lx)
            sB[ly * P + lx] = inside(ly, lx) ? col_window<P, 2, false>(sA + ly * P + lx) : 0u;
        __syncthreads();
        // 3. fill: v3 in place in sB (a position reads sB at itself only)
        row_pass<HALO, E2, R3, 3, true>(sB, sA, tid);
        __syncthreads();
        IPB_REGION(R3, R3, ly, lx) {
            const unsigned v = sB[ly * P + lx];
            const unsigned m = col_window<P, 3, true>(sA + ly * P + lx);
            sB[ly * P + lx] = !inside(ly, lx) ? 0u : empty_bits(v) ? m : v;
        }
        __syncthreads();
    }

    if constexpr (MODE == kFront) {
        // v3 of the tile to the workspace plane, and the first valid row of each of its columns to top
        IPB_REGION(0, 0, ly, lx)
            if (inside(ly, lx)) a.work[((size_t)b * H + (oy + ly)) * W + (ox + lx)] = float_of(sB[ly * P + lx]);
        if (tid < kTW && ox + HALO + tid < W) {
            const int rows = min(kTH, H - (oy + HALO));
            int y = 0;
            while (y < rows && !valid_bits(sB[(HALO + y) * P + HALO + tid])) ++y;
            if (y < rows) atomicMin(&a.top[(size_t)b * W + ox + HALO + tid], oy + HALO + y);
        }
        return;
    }

    unsigned* const v4 = MODE == kBack ? sA : sB;  // the median's source
    unsigned* const v5 = MODE == kBack ? sB : sA;  // the median; v4's buffer then takes the horizontal blur

    if constexpr (MODE == kBack) {
        // 4. the extrapolated read of v3, 0 outside the image; the 31 x 31 fill in place in sA
        const float* work = a.work + (size_t)b * H * W;
        const int* top = a.top + (size_t)b * W;
        IPB_REGION(HALO, HALO, ly, lx) {
            unsigned v = 0u;
            if (inside(ly, lx)) {
                const int gy = oy + ly, gx = ox + lx;
                int tp = top[gx];
                if (tp == INT_MAX) tp = 0;
                v = bits_of(work[(size_t)(gy < tp ? tp : gy) * W + gx]);
            }
            sA[ly * P + lx] = v;
        }
        __syncthreads();
        row_pass<HALO, HALO, 4, 15, true>(sA, sB, tid);
        __syncthreads();
        IPB_REGION(4, 4, ly, lx) {
            const unsigned v = sA[ly * P + lx];
            if (inside(ly, lx) && empty_bits(v)) sA[ly * P + lx] = col_window<P, 15, true>(sB + ly * P + lx);
        }
        __syncthreads();
    }

    // 5. median: v5 on the tile grown by 2, in-image positions only (no other is read below)
    IPB_REGION(2, 2, ly, lx) {
        if (!inside(ly, lx)) continue;
        unsigned m = v4[ly * P + lx];
        if (a.median) {
            const int gy = oy + ly, gx = ox + lx;
            int yy[5], xx[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                yy[k] = (min(max(gy + k - 2, 0), H - 1) - oy) * P;
                xx[k] = min(max(gx + k - 2, 0), W - 1) - ox;
            }
            unsigned w[25];
#pragma unroll
            for (int k = 0; k < 25; ++k) w[k] = v4[yy[k / 5] + xx[k % 5]];
            m = median25(w);
        }
        v5[ly * P + lx] = m;
    }
    __syncthreads();

    // 6. the horizontal pass of the blur into v4's buffer, rows of the tile grown by 2
    const bool blur = a.blur == NCONV_IPBASIC_BLUR_GAUSSIAN;
    if (blur) {
        IPB_REGION(2, 0, ly, lx) {
            if (!inside(ly, lx)) continue;
            const int gx = ox + lx;
            const unsigned* p = v5 + ly * P - ox;
            v4[ly * P + lx] = bits_of(gauss5(float_of(p[reflect101(gx - 2, W)]), float_of(p[reflect101(gx - 1, W)]),
                                             float_of(p[gx]), float_of(p[reflect101(gx + 1, W)]),
                                             float_of(p[reflect101(gx + 2, W)])));
        }
        __syncthreads();
    }

    // 6, 7. the vertical pass, v6 and the way back
    IPB_REGION(0, 0, ly, lx) {
        if (!inside(ly, lx)) continue;
        const int gy = oy + ly, gx = ox + lx;
        float v = float_of(v5[ly * P + lx]);
        if (blur && v > kThr) {
            const unsigned* p = v4 + lx - oy * P;
            v = gauss5(float_of(p[reflect101(gy - 2, H) * P]), float_of(p[reflect101(gy - 1, H) * P]),
                       float_of(p[gy * P]), float_of(p[reflect101(gy + 1, H) * P]),
                       float_of(p[reflect101(gy + 2, H) * P]));
        }
        float o = v > kThr ? a.max_depth - v : 0.f;
        if (a.keep_samples) {
            const float d = ld_f32(r, src_off(ly, lx));
            if (is_sample(d, a.max_depth)) o = d;
        }
        a.dst[(long long)b * a.dbs + (long long)gy * a.drs + gx] = o;
    }
}

#undef IPB_REGION

}  // namespace

int launch_depth_ipbasic(const IpbasicArgs& a, hipStream_t st, const char** why) {
    static_assert(2 * Geo<kAll>::ROWS * Geo<kAll>::P * 4 <= 160 * 1024 / 2, "two workgroups per CU without extrapolate");
    static_assert(2 * Geo<kBack>::ROWS * Geo<kBack>::P * 4 <= 160 * 1024, "the extrapolation's tile fits the LDS");
    const long long tiles = tiles_per_image<kTH, kTW>(a.H, a.W);
    const dim3 grid((unsigned)(a.B * tiles));  // <= B * H * W < 2^31
    if (!a.extrapolate) {
        hipLaunchKernelGGL(ipbasic_tile<kAll>, grid, dim3(kT), 0, st, a);
    } else {
        const unsigned n = (unsigned)a.B * (unsigned)a.W;
        hipLaunchKernelGGL(ipbasic_top_reset, dim3((n - 1) / 256 + 1), dim3(256), 0, st, a.top, n);
        hipLaunchKernelGGL(ipbasic_tile<kFront>, grid, dim3(kT), 0, st, a);
        hipLaunchKernelGGL(ipbasic_tile<kBack>, grid, dim3(kT), 0, st, a);
    }
    return launch_status(why);
}

}  // namespace nconv
