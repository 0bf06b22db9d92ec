// dense_wgrad.hip — weight gradients of the dense convolutions (dense_conv.hip) on the gfx950
// matrix cores.
//
// Training (dense.py's autograd functions): the input gradient of every kind is the forward kernel
// on re-arranged weights — 3x3 / 1x1 stride 1: transposed (+ flipped) kernel; stride 2: the
// transposed 4x4 convolution with the 3x3 / 1x1 kernel embedded; ConvTranspose 4x4: the 4x4 s2
// convolution with the same weights — and the weight gradient is dense_wgrad_mfma below (split-bf16
// maths: dense_wgrad_bf9 for the 3x3).
#include <stdlib.h>

#include "dense_common.h"

namespace nconv {

// ------------------------------------------------------------------------------------------------
// Weight gradients (training):  gW[m][n] = sum over images and pixels p of
//     D[m][p] * P[n / TAPS][patch(p, n % TAPS)]
//   Conv2d 3x3 pad 1 / 1x1, stride S:  pixels = output grid, D = dL/dy (m = co),
//       P = the input x (n = ci*TAPS + kh*KS + kw) at (oy*S + kh - PAD, ox*S + kw - PAD);
//   ConvTranspose2d 4x4 s2 p1:         pixels = input grid, D = the input x (m = ci),
//       P = dL/dy (n = co*16 + kh*4 + kw) at (2 iy - 1 + kh, 2 ix - 1 + kw)
// so gW's own layout (Conv2d (Cout, Cin, k, k) / ConvTranspose2d (Cin, Cout, 4, 4)) is [m][n].
// Implicit GEMM on v_mfma_f32_32x32x2_f32 with K = pixels (2 per MFMA). The (M, N) plane is cut
// into groups of one 32-row m-tile x NT 32-column n-tiles (NT x 32 columns = whole input
// channels: 32 x 9 taps, 16 x 16 taps, 64 x 1); a workgroup owns the GM groups of GM m-tiles over
// one run of n-tiles (the patch channels staged once for all of them) and walks a contiguous range
// of TH x 32 pixel tiles. Wave w takes group w % GM on the pixels of its row share (1/4 or 1/2 of
// the tile), so every wave does the same MFMA work and every loaded byte feeds up to 4 waves. Per
// tile, D and the patch planes are staged in LDS with buffer loads (the next tile's loads in
// flight during the MFMAs); pixel q = q0 + 2j + kk of k-step j sits at a compile-time offset
// from a per-wave base. The waves of a group are summed in LDS and the block writes its partial
// [GM*32][NT*32] to slice ks; dense_wgrad_reduce adds the slices in a fixed order (deterministic,
// no float atomics).
// ------------------------------------------------------------------------------------------------
// pixel tile rows of the weight gradient: 4 x 32, 2 x 32 where the strided patch is tall (3x3 s2,
// transposed). (8 x 32 for the stride-1 3x3 with one m-tile per workgroup measured 1-2 % slower:
// profiles/r5_ab_dense_wgrad_tall_tiles.log)
__host__ __device__ constexpr int wgd_th(int kind, int s) {
    return (kind == NCONV_DENSE_TRANSPOSED_4X4 || (kind == NCONV_DENSE_3X3 && s == 2)) ? 2 : 4;
}
__host__ __device__ constexpr int wgd_ntb(int kind) {
    return kind == NCONV_DENSE_3X3 ? 9 : (kind == NCONV_DENSE_1X1 ? 2 : 8);
}
// column tiles per group for a GEMM of N columns: wgd_ntb, or 1 when N fits one tile
// (the 1- and 3-channel inputs of depth_conv / rgb_encoder0, a 1x1 of <= 32 channels)
constexpr int wgd_nt(int kind, int N) { return N <= 32 ? 1 : wgd_ntb(kind); }

template <int KIND, int S, int NT, int GM>
struct WgdCfg {
    static constexpr bool TR = KIND == NCONV_DENSE_TRANSPOSED_4X4;
    static constexpr int TAPS = KIND == NCONV_DENSE_3X3 ? 9 : (KIND == NCONV_DENSE_1X1 ? 1 : 16);
    static constexpr int KS = KIND == NCONV_DENSE_3X3 ? 3 : (KIND == NCONV_DENSE_1X1 ? 1 : 4);
    static constexpr int NCOLS = 32 * NT;  // columns per group
    // patch channels staged per workgroup: whole channels (wgd_ntb), or every channel a one-tile
    // group may touch
    static constexpr int CPG = NCOLS % TAPS == 0 ? NCOLS / TAPS : (NCOLS - 1) / TAPS + 2;
    static constexpr int RG = 4 / GM;  // row-groups (waves per group; GM groups per workgroup)
    // pixel tile: wgd_th x 32
    static constexpr int TH = wgd_th(KIND, S), TW = 32, NPX = TH * TW;
    static constexpr int PPW = NPX / RG;   // pixels per wave per tile (a multiple of 16)
    // patch geometry: LDS step between neighbouring pixels (1x1 stages only the sampled
    // positions), global step between neighbouring LDS columns, patch origin = pixel * OS - PAD
    static constexpr int LS = KIND == NCONV_DENSE_1X1 ? 1 : (TR ? 2 : S);
    static constexpr int GS = KIND == NCONV_DENSE_1X1 ? S : 1;
    static constexpr int OS = TR ? 2 : S;
    static constexpr int PAD = KIND == NCONV_DENSE_1X1 ? 0 : 1;
    static constexpr int PR = (TH - 1) * LS + KS, PC = (TW - 1) * LS + KS;
    static constexpr int PPLANE = PR * PC;
    static constexpr int DP = NPX + 2;     // D row pitch: rows m, m+1 two banks apart
    static constexpr int D_OFF = (CPG * PPLANE + 3) & ~3;
    static constexpr int BUF = (D_OFF + GM * 32 * DP + 3) & ~3;  // one tile's staging (patch, then D)
    static constexpr int LDS = BUF > 4 * 16 * 64 ? BUF : 4 * 16 * 64;  // (+ the wave-partial sums)
    static constexpr int NDE = GM * 32 * NPX / kDT;  // D elements per thread
    static constexpr int NPG = (CPG * PPLANE + kDT - 1) / kDT;  // patch elements per thread
    static_assert(PPW % 16 == 0 && (GM * 32 * NPX) % kDT == 0, "wave / thread shares");
};

struct WgdArgs {
    const float* d0;
    const float* d1;
    int dC0, dC1;  // direct operand: M = dC0 + dC1 channels on the pixel grid
    int Hp, Wp;    // pixel grid
    const float* p0;
    const float* p1;
    int pC0, pC1;  // patch operand channels
    int Hs, Ws;    // patch source planes
    int M, N;      // N = (pC0 + pC1) * TAPS
    int ntx, nty, nbm, nbn, nks;  // tiles; workgroups along M and N; K slices
    long long ntiles;
};

template <int KIND, int S, int NT, int GM>
__global__ __launch_bounds__(kDT) void dense_wgrad_mfma(WgdArgs a, float* __restrict__ part) {
    using C = WgdCfg<KIND, S, NT, GM>;
    __shared__ __attribute__((aligned(16))) float lds[C::LDS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    int blk = blockIdx.x;
    const int bn = blk % a.nbn;
    blk /= a.nbn;
    const int bm = blk % a.nbm, ks = blk / a.nbm;
    const int m0 = bm * GM * 32, n0 = bn * C::NCOLS;  // the workgroup's first row / column
    const int Cp = a.pC0 + a.pC1;
    const int c_lo = n0 / C::TAPS;
    const long long t0 = a.ntiles * ks / a.nks, t1 = a.ntiles * (ks + 1) / a.nks;
    const size_t HWp = (size_t)a.Hp * a.Wp, HWs = (size_t)a.Hs * a.Ws;

    // this wave's group (m-tile gmi) and pixel share [q0, q0 + PPW) of each tile
    const int gmi = w % GM, rg = w / GM;
    const int q0 = rg * C::PPW;
    const int kk = lane >> 5, li = lane & 31;
    const int abase = C::D_OFF + (gmi * 32 + li) * C::DP + kk;  // + q
    int bbase[NT];
#pragma unroll
    for (int u = 0; u < NT; ++u) {
        const int nl = 32 * u + li;  // column within the workgroup
        const int ci = nl / C::TAPS, tap = nl % C::TAPS;
        const int kh = tap / C::KS, kw = tap % C::KS;
        bbase[u] = ci * C::PPLANE + kh * C::PC + kw + kk * C::LS;  // + r*LS*PC + c*LS
    }

    f16v acc[NT];
#pragma unroll
    for (int u = 0; u < NT; ++u) acc[u] = (f16v){};

    // Staging loads are buffer loads: the image's planes sit behind one SGPR resource per
    // source, elements outside the image / channel range carry an offset past it and read 0
    // (no per-element masks or 64-bit addresses live across the load latency). The source of the
    // workgroup's patch channels is uniform whenever the concatenation boundary is a multiple of
    // 32 channels (16 for the transposed kernel) — every concatenation of the guided model;
    // otherwise each element is read from the source its channel belongs to.
    constexpr unsigned OOB = 0x80000000u;
    // LDS-DMA staging (buffer_load ... lds): every staged element goes from HBM straight into its
    // LDS slot -- no staging registers, so the weight-gradient accumulators (NT x 16 per lane) and
    // the rest fit two waves per SIMD, and one workgroup's loads hide behind the other's MFMAs.
    // A wave's 64 elements of one load are consecutive in the LDS image (the DMA writes wave base
    // + lane x 4): the patch planes are unpadded and a D row (NPX >= 64 pixels) never splits a wave.
    typedef __attribute__((address_space(3))) void* lds_ptr_t;
    auto glds = [&](__amdgpu_buffer_rsrc_t r, float* dst, unsigned off) __attribute__((always_inline)) {
        __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (lds_ptr_t)dst, 4, off, 0, 0, 0);
    };
    const int wb = 64 * w;  // the wave's first element of each load
    // Per-block constants of the staging (the element -> LDS slot map is the same for every tile):
    // each patch element's byte offset from its tile's patch origin (channel plane included;
    // 0x80000000 for the channels past the input, which then reads 0 whatever the tile), and each
    // D element's pixel offset. An interior tile then costs one add per element; tiles touching
    // the image border take the general path with per-element bounds.
    constexpr unsigned OOB_REL = 0x80000000u;
    // the patch channels c_lo .. c_lo + CPG - 1: their source (hi: the second), first channel there
    const bool hi = a.p1 != nullptr && c_lo >= a.pC0;
    const bool gwhole = !(a.p1 != nullptr && c_lo < a.pC0 && c_lo + C::CPG > a.pC0);  // one source
    const int cb = hi ? a.pC0 : 0;
    unsigned prel[C::NPG];
#pragma unroll
    for (int k = 0; k < C::NPG; ++k) {
        const int e = tid + kDT * k;
        const int ci = e / C::PPLANE, rem = e % C::PPLANE;
        const int r = rem / C::PC, c = rem % C::PC;
        prel[k] = (c_lo + ci < Cp && e < C::CPG * C::PPLANE)
                      ? ((unsigned)(c_lo + ci - cb) * (unsigned)HWs + (unsigned)(r * C::GS * a.Ws + c * C::GS)) * 4u
                      : OOB_REL;
    }
    const int dq = tid % C::NPX;
    const unsigned drel = (unsigned)((dq / C::TW) * a.Wp + dq % C::TW) * 4u;
    // the block's tiles walk (tx, ty, b) in order from t0
    int tx_c = (int)(t0 % a.ntx), ty_c = (int)((t0 / a.ntx) % a.nty), b_c = (int)(t0 / ((long long)a.ntx * a.nty));
    auto stage = [&](int tx, int ty, int b, float* lds) __attribute__((always_inline)) {
        int tq = tid;
        asm volatile("" : "+v"(tq));
        const int py0 = ty * C::TH, px0 = tx * C::TW;
        const int iy0 = py0 * C::OS - C::PAD, ix0 = px0 * C::OS - C::PAD;
        const bool dfull = py0 + C::TH <= a.Hp && px0 + C::TW <= a.Wp;
        const bool pfull = iy0 >= 0 && ix0 >= 0 && iy0 + (C::PR - 1) * C::GS < a.Hs && ix0 + (C::PC - 1) * C::GS < a.Ws;
        {
            unsigned ob;
            if (dfull) {
                ob = (unsigned)(py0 * a.Wp + px0) * 4u + drel;
            } else {
                const int py = py0 + dq / C::TW, px = px0 + dq % C::TW;
                ob = (py < a.Hp && px < a.Wp) ? (unsigned)(py * a.Wp + px) * 4u : OOB;
            }
            const __amdgpu_buffer_rsrc_t rd0 = plane_rsrc(a.d0 + (size_t)b * a.dC0 * HWp, (int)(a.dC0 * HWp * 4));
            const __amdgpu_buffer_rsrc_t rd1 =
                plane_rsrc(a.d1 ? a.d1 + (size_t)b * a.dC1 * HWp : a.d0, (int)((a.d1 ? a.dC1 : 0) * HWp * 4));
            const int mw = __builtin_amdgcn_readfirstlane(m0 + tid / C::NPX);  // NPX >= 64: per wave
#pragma unroll
            for (int k = 0; k < C::NDE; ++k) {
                const int m = mw + (kDT / C::NPX) * k;
                const bool s1 = m >= a.dC0;
                const int mm = s1 ? m - a.dC0 : m;
                const unsigned off = (m < a.M && ob != OOB) ? (unsigned)(mm * HWp) * 4u + ob : OOB;
                const int e0 = wb + kDT * k;
                glds(s1 ? rd1 : rd0, lds + C::D_OFF + (e0 / C::NPX) * C::DP + e0 % C::NPX, off);
            }
        }
        const __amdgpu_buffer_rsrc_t rp0 = plane_rsrc(a.p0 + (size_t)b * a.pC0 * HWs, (int)(a.pC0 * HWs * 4));
        const __amdgpu_buffer_rsrc_t rp1 =
            plane_rsrc(a.p1 ? a.p1 + (size_t)b * a.pC1 * HWs : a.p0, (int)((a.p1 ? a.pC1 : 0) * HWs * 4));
        const unsigned pbase = (unsigned)(iy0 * a.Ws + ix0) * 4u;  // used by interior tiles only
        const __amdgpu_buffer_rsrc_t rp = hi ? rp1 : rp0;
        if (pfull && gwhole) {
#pragma unroll
            for (int k = 0; k < C::NPG; ++k)
                if ((k + 1) * kDT <= C::CPG * C::PPLANE || tq + kDT * k < C::CPG * C::PPLANE)
                    glds(rp, lds + wb + kDT * k, pbase + prel[k]);
            return;
        }
#pragma unroll
        for (int k = 0; k < C::NPG; ++k) {
            const int e = tq + kDT * k;
            if ((k + 1) * kDT <= C::CPG * C::PPLANE || e < C::CPG * C::PPLANE) {
                const int ci = e / C::PPLANE, rem = e % C::PPLANE;
                const int r = rem / C::PC, c = rem % C::PC;
                const int gc = c_lo + ci, iy = iy0 + r * C::GS, ix = ix0 + c * C::GS;
                const bool ok = gc < Cp && (unsigned)iy < (unsigned)a.Hs && (unsigned)ix < (unsigned)a.Ws;
                const unsigned pix = (unsigned)(iy * a.Ws + ix);
                float* dst = lds + wb + kDT * k;
                if (gwhole) {
                    glds(rp, dst, ok ? ((unsigned)(gc - cb) * (unsigned)HWs + pix) * 4u : OOB);
                } else if (gc < a.pC0) {  // the channels come from both sources: each lane one
                    glds(rp0, dst, ok ? ((unsigned)gc * (unsigned)HWs + pix) * 4u : OOB);
                } else {
                    glds(rp1, dst, ok ? ((unsigned)(gc - a.pC0) * (unsigned)HWs + pix) * 4u : OOB);
                }
            }
        }
    };

    auto next_tile = [&]() __attribute__((always_inline)) {
        if (++tx_c == a.ntx) {
            tx_c = 0;
            if (++ty_c == a.nty) {
                ty_c = 0;
                ++b_c;
            }
        }
    };
    // one buffer: the loads of one workgroup hide behind the MFMAs of the CU's other workgroup (a
    // double-buffered single workgroup per CU measured slower, 704.6 against 614.0 us for the
    // 32-channel 3x3: profiles/r5_ab_dense_wgrad_db.log; removed in round 6)
#pragma unroll 1
    for (long long t = t0; t < t1; ++t) {
        const float* lb = lds;
        __syncthreads();  // the previous tile's MFMAs are done with the LDS
        stage(tx_c, ty_c, b_c, lds);
        next_tile();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        // the wave's pixels in segments of 16 (8 k-steps) inside one tile row
#pragma unroll 1
        for (int sg = 0; sg < C::PPW / 16; ++sg) {
            const int q = q0 + 16 * sg, r = q / C::TW, c = q % C::TW;
            const int aoff = abase + q, boff = r * C::LS * C::PC + c * C::LS;
#pragma unroll 2
            for (int j = 0; j < 8; ++j) {
                const float av = lb[aoff + 2 * j];
#pragma unroll
                for (int u = 0; u < NT; ++u) {
                    const float bv = lb[bbase[u] + boff + 2 * j * C::LS];
                    acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[u], 0, 0, 0);
                }
            }
        }
    }

    // ---- the block's partial [GM*32][NT*32] -> slice ks: C[row = m][col = n]. The RG waves of
    //      a group hold the same tile over different pixels: summed here in LDS (fixed order, one
    //      n-tile at a time), so the block writes one slice, not RG (RG x less partial traffic
    //      for dense_wgrad_reduce) ----
    float* out = part + (size_t)ks * a.M * a.N;
#pragma unroll
    for (int u = 0; u < NT; ++u) {
        __syncthreads();  // the LDS is free (after the MFMAs / the previous tile)
#pragma unroll
        for (int q = 0; q < 16; ++q) lds[(w * 16 + q) * 64 + lane] = acc[u][q];
        __syncthreads();
        for (int e = tid; e < GM * 1024; e += kDT) {
            const int g2 = e >> 10, q = (e >> 6) & 15, l = e & 63;
            float v = lds[(g2 * 16 + q) * 64 + l];
#pragma unroll
            for (int r2 = 1; r2 < C::RG; ++r2) v += lds[((g2 + GM * r2) * 16 + q) * 64 + l];
            const int n = n0 + 32 * u + (l & 31);
            const int m = m0 + g2 * 32 + (q & 3) + 8 * (q >> 2) + 4 * (l >> 5);
            if (n < a.N && m < a.M) out[(size_t)m * a.N + n] = v;
        }
    }
}

// gw[e] = sum over the nsl slices of part[slice][e]: 64 elements x 4 slice phases per block,
// each phase summing every 4th slice in order, the phases combined in a fixed order. Summed in T
// (float; double for dense_wgrad_tr_rows' fp64 partials), rounded once on the store.
template <typename T>
__global__ __launch_bounds__(kDT) void dense_wgrad_reduce(const T* __restrict__ part, int nsl, int mn,
                                                          float* __restrict__ gw) {
    __shared__ T red[4][64];
    const int col = threadIdx.x & 63, ph = threadIdx.x >> 6;
    const int e = blockIdx.x * 64 + col;
    T s = 0;
    if (e < mn) {
#pragma unroll 8
        for (int k = ph; k < nsl; k += 4) s += part[(size_t)k * mn + e];
    }
    red[ph][col] = s;
    __syncthreads();
    if (ph == 0 && e < mn) gw[e] = (float)(((red[0][col] + red[1][col]) + red[2][col]) + red[3][col]);
}

// ---- the transposed convolution's weight-gradient rows of the few channels concatenated beside
//      whole 32-channel groups (UpCat's depth channel and 32 / 64 features, step2.py:173) ----
// On the matrix cores those rows would take a whole 32-row m-tile each (M = 33 / 65 padded to 64 /
// 96: half or a third of the tile work wasted); here they are a GEMV on the vector ALU that
// streams dL/dy once:
//   out[j][co*16 + kh*4 + kw] = sum over (b, oy, ox) with oy + 1 - kh, ox + 1 - kw even of
//       gy[b][co][oy][ox] * x1[b][j][(oy + 1 - kh) / 2][(ox + 1 - kw) / 2]
// Each dL/dy element meets two kernel rows (kh of its row parity) and two columns. Workgroup =
// one channel co of one image over a 16-row x 256-column block of dL/dy: thread = column, its 16
// rows read coalesced, the x1 window (10 rows x 130 columns per channel) staged in LDS; the 16
// tap sums of the workgroup reduced over its threads in a fixed order into its partial slot
// part[slice][co * 16 + tap], slice = (image, row block, column block); dense_wgrad_reduce adds
// the slices in a fixed order (deterministic).
constexpr int kTrRows = 16, kTrCols = 256;
constexpr int kTrXH = kTrRows / 2 + 2, kTrXW = kTrCols / 2 + 2;  // x1 window
constexpr int kTrMaxC1 = 2, kTrMaxG = 6;                          // channels; Cout <= 16 * kTrMaxG
__global__ __launch_bounds__(256) void dense_wgrad_tr_rows(const float* __restrict__ x1, int C1, int H, int W,
                                                           const float* __restrict__ gy, int Cout, int Ho, int Wo,
                                                           int nry, int nrx, double* __restrict__ part) {
    __shared__ float sx[kTrMaxC1 * kTrXH * kTrXW];
    __shared__ double red[4][kTrMaxC1 * 16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int blk = blockIdx.x;
    const int co = blk % Cout;
    blk /= Cout;
    const int rx = blk % nrx;
    blk /= nrx;
    const int ry = blk % nry, b = blk / nry;
    const int oy0 = ry * kTrRows, ox0 = rx * kTrCols;
    const int iy0 = oy0 / 2 - 1, ix0 = ox0 / 2 - 1;
    for (int e = tid; e < C1 * kTrXH * kTrXW; e += 256) {
        const int j = e / (kTrXH * kTrXW), r = (e / kTrXW) % kTrXH, c = e % kTrXW;
        const int iy = iy0 + r, ix = ix0 + c;
        sx[e] = ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) ? x1[(((size_t)b * C1 + j) * H + iy) * W + ix]
                                                                         : 0.f;
    }
    const int ox = ox0 + tid;
    float gv[kTrRows];
    const float* gp = gy + (((size_t)b * Cout + co) * Ho + oy0) * Wo + ox;
#pragma unroll
    for (int r = 0; r < kTrRows; ++r) gv[r] = (ox < Wo && oy0 + r < Ho) ? gp[(size_t)r * Wo] : 0.f;
    __syncthreads();
    // this column's two kernel columns (kw of the parity of ox + 1) and their x1 columns
    const int kwa = (ox + 1) & 1;                  // kw in {kwa, kwa + 2}
    const int xca = (ox + 1 - kwa) / 2 - ix0;      // x1 column of kw = kwa; kw = kwa + 2: xca - 1
    // acc[j][kh][i]: kernel column kw = kwa + 2 i (the thread's column parity; kh is the row's,
    // known per unrolled row since the block's first row is even). Exact products summed in fp64,
    // the partials kept in fp64 down to the final reduction: dL/dy of the BatchNorm after this
    // convolution has zero mean per channel while the depth channel has a large mean (0..80 m), so
    // the sum is a small difference of large terms -- in fp32 its rounding reached 1.4e-3 of the
    // largest gradient (golden f9, fuse1.upcat.upf.conv.weight; the reference's own: 5e-6)
    double acc[kTrMaxC1][4][2];
#pragma unroll
    for (int j = 0; j < kTrMaxC1; ++j)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[j][t][0] = acc[j][t][1] = 0.0;
#pragma unroll
    for (int r = 0; r < kTrRows; ++r) {
        const int kha = (r + 1) & 1;                    // oy0 even: kh in {kha, kha + 2}
        const int xra = (oy0 + r + 1 - kha) / 2 - iy0;  // x1 row of kh = kha; kh = kha + 2: xra - 1
#pragma unroll
        for (int j = 0; j < kTrMaxC1; ++j) {
            if (j >= C1) continue;
            const float* xs = sx + j * kTrXH * kTrXW;
            const float x00 = xs[xra * kTrXW + xca], x01 = xs[xra * kTrXW + xca - 1];
            const float x10 = xs[(xra - 1) * kTrXW + xca], x11 = xs[(xra - 1) * kTrXW + xca - 1];
            const double g = (double)gv[r];
            acc[j][kha][0] = __builtin_fma(g, (double)x00, acc[j][kha][0]);
            acc[j][kha][1] = __builtin_fma(g, (double)x01, acc[j][kha][1]);
            acc[j][kha + 2][0] = __builtin_fma(g, (double)x10, acc[j][kha + 2][0]);
            acc[j][kha + 2][1] = __builtin_fma(g, (double)x11, acc[j][kha + 2][1]);
        }
    }
    // the workgroup's 16 (x C1) tap sums in wave_ops.h's order
#pragma unroll
    for (int j = 0; j < kTrMaxC1; ++j) {
        if (j >= C1) continue;
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int kh = t >> 2, kw = t & 3;
            const double v = wave_sum((kw & 1) == kwa ? acc[j][kh][kw >> 1] : 0.0);
            if (lane == 0) red[wv][j * 16 + t] = v;
        }
    }
    __syncthreads();
    if (tid < C1 * 16) {
        const int j = tid >> 4, t = tid & 15;
        const size_t slice = ((size_t)b * nry + ry) * nrx + rx;
        part[(slice * C1 + j) * (size_t)(Cout * 16) + co * 16 + t] = waves_in_order(&red[0][tid], kTrMaxC1 * 16);
    }
}

// ------------------------------------------------------------------------------------------------
// Weight gradient of the 3x3 stride-1 convolution on the bf16 matrix cores (split-bf16 maths):
//   gW[co][ci][tap] = sum over pixels p of D[co][p] * X[ci][p + tap]
// as nine GEMMs C_tap[co][ci] (M = 32 output channels, N = 32 input channels, K = pixels) on
// v_mfma_f32_32x32x16_bf16, both operands split into three bf16 parts (nine or six terms, as the
// forward). A = D[co][16 pixels]: 8 consecutive pixels per lane half, one ds_read_b128 of a
// [part][co][pixel] image. B = X[16 pixels + tap][ci]: the patch image is channel-innermost
// ([part][position][32 channels]), so a lane's 8 pixels of one channel are a column of it, read
// with two ds_read_b64_tr_b16 (4 rows x 16 channels per 16-lane group, delivered column-major):
// the tap shift moves whole 64-byte rows, so every address stays aligned (pixel-contiguous
// images would put 7 of 9 taps' fragments off the 16-byte alignment ds_read_b128 needs).
// Tiles, split-K slices and the partial layout are dense_wgrad_mfma<3x3, 1, 9, 1>'s: a workgroup
// owns 32 output channels x 32 input channels x 9 taps and walks a contiguous range of 4 x 32
// pixel tiles; wave w takes tile row w; the four waves' tiles are summed in LDS in a fixed order
// and the block writes one slice (dense_wgrad_reduce adds the slices in a fixed order).
// ------------------------------------------------------------------------------------------------
typedef short dv4s __attribute__((ext_vector_type(4)));
typedef short dv8s __attribute__((ext_vector_type(8)));
template <int S>
struct Wb9 {  // tiles as dense_wgrad_mfma's: 4 x 32 pixels (stride 2: 2 x 32, its patch is twice as wide)
    static constexpr int TH = S == 1 ? 4 : 2, TW = 32, NPX = TH * TW;
    static constexpr int PR = (TH - 1) * S + 3, PC = (TW - 1) * S + 3, NPOS = PR * PC;
    static constexpr int PPW = NPX / 4, NKW = PPW / 16;  // pixels and 16-pixel k-steps per wave
    static constexpr int NDI = 32 * NPX / 8 / kDT;      // D items (channel, 8 pixels) per thread
    static constexpr int PPART = NPOS * 64;          // bytes of one part's patch image (32 channels)
    static constexpr int PDUMP = 3 * PPART;          // slots of positions past the patch
    static constexpr int DB = NPX * 2 + 16;          // bytes per D row (16-byte pad: conflict-free A reads)
    static constexpr int DOFF = PDUMP + 64;
    static constexpr int DPART = 32 * DB;
    static constexpr int LDSB = DOFF + 3 * DPART;    // (the epilogue reuses the first 16 KB)
    static constexpr int NPW = (NPOS + 63) / 64;     // positions per lane (wave = one 8-channel group)
};

template <int NTERM, int S>
__global__ __launch_bounds__(kDT, 2) void dense_wgrad_bf9(WgdArgs a, float* __restrict__ part) {
    using C = Wb9<S>;
    __shared__ __attribute__((aligned(16))) unsigned char lds[C::LDSB];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    int blk = blockIdx.x;
    const int bn = blk % a.nbn;
    blk /= a.nbn;
    const int bm = blk % a.nbm, ks = blk / a.nbm;
    const int m0 = bm * 32, c_lo = bn * 32;  // first output channel, first input channel
    const int Cp = a.pC0 + a.pC1;
    const long long t0 = a.ntiles * ks / a.nks, t1 = a.ntiles * (ks + 1) / a.nks;
    const int HWp = a.Hp * a.Wp, HWs = a.Hs * a.Ws;
    constexpr unsigned OOB = 0x80000000u;

    // staging registers: wave w stages input channels c_lo + 8w .. + 7 at NPW positions per lane,
    // and 2 (output channel, 8-pixel segment) items of D per thread
    float xv[C::NPW][8], dv[C::NDI][8];
    int tx_c = (int)(t0 % a.ntx), ty_c = (int)((t0 / a.ntx) % a.nty), b_c = (int)(t0 / ((long long)a.ntx * a.nty));
    auto load_tile = [&](int tx, int ty, int b) {
        const int py0 = ty * C::TH, px0 = tx * C::TW, iy0 = py0 * S - 1, ix0 = px0 * S - 1;
        const __amdgpu_buffer_rsrc_t rp0 = plane_rsrc(a.p0 + (size_t)b * a.pC0 * HWs, a.pC0 * HWs * 4);
        const __amdgpu_buffer_rsrc_t rp1 =
            plane_rsrc(a.pC1 > 0 ? a.p1 + (size_t)b * a.pC1 * HWs : a.p0, a.pC1 > 0 ? a.pC1 * HWs * 4 : 0);
        unsigned po[C::NPW];
#pragma unroll
        for (int k = 0; k < C::NPW; ++k) {
            const int pos = lane + 64 * k, r = pos / C::PC, c = pos - r * C::PC;
            const int iy = iy0 + r, ix = ix0 + c;
            po[k] = pos < C::NPOS && (unsigned)iy < (unsigned)a.Hs && (unsigned)ix < (unsigned)a.Ws
                        ? (unsigned)(iy * a.Ws + ix) * 4u : OOB;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int ci = c_lo + 8 * w + j;  // wave-uniform
            const bool s0 = ci < a.pC0;
            const __amdgpu_buffer_rsrc_t rs = s0 ? rp0 : rp1;
            const int so = (s0 ? ci : ci - a.pC0) * HWs * 4;  // past Cp: out of range, reads 0
#pragma unroll
            for (int k = 0; k < C::NPW; ++k) xv[k][j] = ld_f32s(rs, po[k], so);
        }
        const __amdgpu_buffer_rsrc_t rd = plane_rsrc(a.d0 + (size_t)b * a.dC0 * HWp, a.dC0 * HWp * 4);
#pragma unroll
        for (int k = 0; k < C::NDI; ++k) {
            const int it = tid + kDT * k, col = it / (C::NPX / 8), seg = it % (C::NPX / 8);
            const int py = py0 + (seg >> 2), px = px0 + (seg & 3) * 8, co = m0 + col;
            const bool ok = co < a.M && py < a.Hp;
            const unsigned base = (unsigned)(co * HWp + py * a.Wp + px) * 4u;
#pragma unroll
            for (int j = 0; j < 8; ++j) dv[k][j] = ld_f32(rd, ok && px + j < a.Wp ? base + 4u * j : OOB);
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int k = 0; k < C::NPW; ++k) {
            const int pos = lane + 64 * k;
            dbf16x8 sp[3];
            dsplit3(xv[k], sp);
            const bool in = pos < C::NPOS;
            const int at = in ? pos * 64 + w * 16 : C::PDUMP + w * 16, da = in ? C::PPART : 0;
#pragma unroll
            for (int i = 0; i < 3; ++i) *reinterpret_cast<dbf16x8*>(lds + at + i * da) = sp[i];
        }
#pragma unroll
        for (int k = 0; k < C::NDI; ++k) {
            const int it = tid + kDT * k, col = it / (C::NPX / 8), seg = it % (C::NPX / 8);
            dbf16x8 sp[3];
            dsplit3(dv[k], sp);
#pragma unroll
            for (int i = 0; i < 3; ++i)
                *reinterpret_cast<dbf16x8*>(lds + C::DOFF + i * C::DPART + col * C::DB + seg * 16) = sp[i];
        }
    };
    auto next_tile = [&]() {
        if (++tx_c == a.ntx) {
            tx_c = 0;
            if (++ty_c == a.nty) {
                ty_c = 0;
                ++b_c;
            }
        }
    };

    const int kk = lane >> 5, li = lane & 31;
    const int g = lane >> 4, il = lane & 15, q = il >> 2, pq = il & 3;
    // the wave's pixels: tile row prow, columns pcol0 .. + PPW - 1
    const int prow = w * C::PPW / C::TW, pcol0 = w * C::PPW % C::TW;
    // A: D row li, pixels (the k-step's 16) + 8 kk
    const int abase = C::DOFF + li * C::DB + (w * C::PPW + 8 * kk) * 2;
    // B (transposed reads): block row q = pixel 8 kk + 4 h + q of the k-step (patch column S x its
    // column), channels 16 (g & 1) + 4 pq .. + 3
    const int bbase = (prow * S * C::PC + (pcol0 + 8 * kk + q) * S) * 64 + (16 * (g & 1) + 4 * pq) * 2;

    f16v acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[t] = (f16v){};
    typedef __attribute__((address_space(3))) dv4s* lds4_t;
    auto trd = [&](int off) { return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4_t)(lds + off)); };

    if (t0 < t1) load_tile(tx_c, ty_c, b_c);
#pragma unroll 1
    for (long long t = t0; t < t1; ++t) {
        store_tile();
        next_tile();
        __syncthreads();
        if (t + 1 < t1) load_tile(tx_c, ty_c, b_c);  // the next tile's loads in flight during the MFMAs
#pragma unroll
        for (int s2 = 0; s2 < C::NKW; ++s2) {  // the wave's 16-pixel k-steps
            dbf16x8 av[3];
#pragma unroll
            for (int i = 0; i < 3; ++i)
                av[i] = *reinterpret_cast<const dbf16x8*>(lds + abase + i * C::DPART + s2 * 32);
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const int kh = tap / 3, kw = tap % 3;
                const int bo = bbase + (kh * C::PC + s2 * 16 * S + kw) * 64;
                dbf16x8 bv[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const dv4s lo = trd(bo + i * C::PPART), hi = trd(bo + i * C::PPART + 4 * S * 64);
                    const dv8s v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
                    bv[i] = __builtin_bit_cast(dbf16x8, v);
                }
                constexpr int ti[9] = {2, 2, 1, 2, 1, 0, 1, 0, 0}, tj[9] = {2, 1, 2, 0, 1, 2, 0, 1, 0};
#pragma unroll
                for (int qq = 9 - NTERM; qq < 9; ++qq)
                    acc[tap] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[ti[qq]], bv[tj[qq]], acc[tap], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        __syncthreads();  // this tile's MFMAs are done with the LDS
    }

    // ---- the four waves' C_tap summed in LDS (fixed order), one slice per block: C[row = co][col = ci],
    //      col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5) for register r ----
    float* lf = reinterpret_cast<float*>(lds);
    float* out = part + (size_t)ks * a.M * a.N;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 16; ++r) lf[(w * 16 + r) * 64 + lane] = acc[tap][r];
        __syncthreads();
        for (int e = tid; e < 1024; e += kDT) {
            const int r = (e >> 6) & 15, l = e & 63;
            const float v = ((lf[r * 64 + l] + lf[(16 + r) * 64 + l]) + lf[(32 + r) * 64 + l]) + lf[(48 + r) * 64 + l];
            const int co = m0 + (r & 3) + 8 * (r >> 2) + 4 * (l >> 5), ci = c_lo + (l & 31);
            if (co < a.M && ci < Cp) out[(size_t)co * a.N + ci * 9 + tap] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Plan and launchers
// ------------------------------------------------------------------------------------------------
struct WgdPlan {
    WgdArgs a;
    int nt, gm;  // n-tiles per group; m-tiles (groups) per workgroup
    bool bf9;    // dense_wgrad_bf9
};
// the split-bf16 weight gradient: 3x3 (stride 1 or 2) with 32-channel x 9-tap n-groups (Cin >= 4)
static bool wgrad_bf9(const nconv_dense_wgrad& g, int nt) {
    return g.math != NCONV_DENSE_MATH_FP32 && g.kind == NCONV_DENSE_3X3 && nt == 9;
}

static WgdPlan wgrad_plan(const nconv_dense_wgrad& g) {
    WgdPlan pl{};
    WgdArgs& a = pl.a;
    const int cin = g.C0 + g.C1;
    const bool tr = g.kind == NCONV_DENSE_TRANSPOSED_4X4;
    if (!tr) {  // Conv2d: D = dL/dy, patch = x
        a.d0 = g.gy;
        a.d1 = nullptr;
        a.dC0 = g.Cout;
        a.dC1 = 0;
        a.Hp = g.Ho;
        a.Wp = g.Wo;
        a.p0 = g.x0;
        a.p1 = g.x1;
        a.pC0 = g.C0;
        a.pC1 = g.C1;
        a.Hs = g.H;
        a.Ws = g.W;
        a.M = g.Cout;
        a.N = cin * dense_taps(g.kind);
    } else {  // ConvTranspose2d: D = x, patch = dL/dy
        a.d0 = g.x0;
        a.d1 = g.x1;
        a.dC0 = g.C0;
        a.dC1 = g.C1;
        a.Hp = g.H;
        a.Wp = g.W;
        a.p0 = g.gy;
        a.p1 = nullptr;
        a.pC0 = g.Cout;
        a.pC1 = 0;
        a.Hs = g.Ho;
        a.Ws = g.Wo;
        a.M = cin;
        a.N = g.Cout * 16;
    }
    pl.nt = wgd_nt(g.kind, a.N);
    const int nmg = (a.M + 31) / 32, nng = (a.N + 32 * pl.nt - 1) / (32 * pl.nt);
    // groups per workgroup: pairs along M where they divide evenly (one n-group per workgroup:
    // with LDS-DMA staging two workgroups then fit a CU's LDS); dense_wgrad_bf9 takes one m-tile
    pl.bf9 = wgrad_bf9(g, pl.nt);
    pl.gm = (pl.nt > 1 && nmg % 2 == 0 && !pl.bf9) ? 2 : 1;
    const int th = wgd_th(g.kind, g.stride);
    a.ntx = (a.Wp + 31) / 32;
    a.nty = (a.Hp + th - 1) / th;
    a.ntiles = (long long)g.B * a.ntx * a.nty;
    a.nbm = nmg / pl.gm;
    a.nbn = nng;
    long long nks = 512 / (a.nbm * a.nbn);  // two workgroups per CU
    if (nks < 1) nks = 1;
    if (nks > a.ntiles) nks = a.ntiles;
    a.nks = (int)nks;
    return pl;
}

// The transposed kind with one source of a few channels beside one of whole 32-channel groups:
// the matrix cores take the large source's rows, dense_wgrad_tr_rows the small one's
// (NCONV_WGD_TR_ROWS=0: all on the matrix cores). Returns 0 (no split), 1 (x1 small), 2 (x0 small).
static int tr_rows_split(const nconv_dense_wgrad& g) {
    const char* e = getenv("NCONV_WGD_TR_ROWS");
    if ((e && e[0] == '0') || g.kind != NCONV_DENSE_TRANSPOSED_4X4 || !g.x1 || g.C0 <= 0 || g.C1 <= 0 ||
        g.Cout % 16 != 0 || g.Cout > 16 * kTrMaxG)
        return 0;
    if (g.C1 <= kTrMaxC1 && g.C0 % 32 == 0) return 1;
    if (g.C0 <= kTrMaxC1 && g.C1 % 32 == 0) return 2;
    return 0;
}
// the large source alone, its gradient rows where they sit in gw
static nconv_dense_wgrad tr_rows_main(const nconv_dense_wgrad& g) {
    nconv_dense_wgrad m = g;
    if (tr_rows_split(g) == 2) {
        m.x0 = g.x1;
        m.C0 = g.C1;
        m.gw = g.gw + (size_t)g.C0 * g.Cout * 16;
    }
    m.x1 = nullptr;
    m.C1 = 0;
    return m;
}
struct TrRowsGrid {
    int nry, nrx, nslice;
};
static TrRowsGrid tr_rows_grid(const nconv_dense_wgrad& g) {
    TrRowsGrid r;
    r.nry = (g.Ho + kTrRows - 1) / kTrRows;
    r.nrx = (g.Wo + kTrCols - 1) / kTrCols;
    r.nslice = g.B * r.nry * r.nrx;
    return r;
}

static size_t main_wgrad_bytes(const nconv_dense_wgrad& g) {
    const WgdPlan pl = wgrad_plan(g);
    return (size_t)pl.a.nks * pl.a.M * pl.a.N * sizeof(float);
}

size_t dense_wgrad_workspace_bytes(const nconv_dense_wgrad& g) {
    if (!tr_rows_split(g)) return main_wgrad_bytes(g);
    const size_t a = (main_wgrad_bytes(tr_rows_main(g)) + 255) & ~(size_t)255;
    const int cs = tr_rows_split(g) == 1 ? g.C1 : g.C0;
    return a + (size_t)tr_rows_grid(g).nslice * cs * g.Cout * 16 * sizeof(double);
}

// dense_wgrad_mfma of the plan's grouping: one m-tile per workgroup, or a pair (never with NT = 1)
template <int KIND, int S, int NT>
static bool go_wgrad(const WgdPlan& pl, float* ws, hipStream_t st) {
    const dim3 grid(pl.a.nbm * pl.a.nbn * pl.a.nks), blk(kDT);
    if (pl.gm == 1)
        hipLaunchKernelGGL((dense_wgrad_mfma<KIND, S, NT, 1>), grid, blk, 0, st, pl.a, ws);
    else if constexpr (NT > 1)
        hipLaunchKernelGGL((dense_wgrad_mfma<KIND, S, NT, 2>), grid, blk, 0, st, pl.a, ws);
    else
        return false;
    return true;
}
template <int KIND, int S>
static bool go_wgrad_nt(const WgdPlan& pl, float* ws, hipStream_t st) {
    return pl.nt == 1 ? go_wgrad<KIND, S, 1>(pl, ws, st) : go_wgrad<KIND, S, wgd_ntb(KIND)>(pl, ws, st);
}
static void go_wgrad_bf9(const nconv_dense_wgrad& g, const WgdPlan& pl, float* ws, hipStream_t st) {
    const dim3 grid(pl.a.nbm * pl.a.nbn * pl.a.nks), blk(kDT);
    const bool x9 = g.math == NCONV_DENSE_MATH_BF16X9;
    if (g.stride == 1 && x9)
        hipLaunchKernelGGL((dense_wgrad_bf9<9, 1>), grid, blk, 0, st, pl.a, ws);
    else if (g.stride == 1)
        hipLaunchKernelGGL((dense_wgrad_bf9<6, 1>), grid, blk, 0, st, pl.a, ws);
    else if (x9)
        hipLaunchKernelGGL((dense_wgrad_bf9<9, 2>), grid, blk, 0, st, pl.a, ws);
    else
        hipLaunchKernelGGL((dense_wgrad_bf9<6, 2>), grid, blk, 0, st, pl.a, ws);
}

// the partial slices of one GEMM (dense_wgrad_bf9, else dense_wgrad_mfma by kind and stride) and
// their reduction into g.gw
static int launch_dense_wgrad_main(const nconv_dense_wgrad& g, float* ws, hipStream_t st, const char** why) {
    const WgdPlan pl = wgrad_plan(g);
    bool ok = false;
    if (pl.bf9) {
        go_wgrad_bf9(g, pl, ws, st);
        ok = true;
    } else if (g.kind == NCONV_DENSE_3X3 && g.stride == 1) {
        ok = go_wgrad_nt<NCONV_DENSE_3X3, 1>(pl, ws, st);
    } else if (g.kind == NCONV_DENSE_3X3 && g.stride == 2) {
        ok = go_wgrad_nt<NCONV_DENSE_3X3, 2>(pl, ws, st);
    } else if (g.kind == NCONV_DENSE_1X1 && g.stride == 1) {
        ok = go_wgrad_nt<NCONV_DENSE_1X1, 1>(pl, ws, st);
    } else if (g.kind == NCONV_DENSE_1X1 && g.stride == 2) {
        ok = go_wgrad_nt<NCONV_DENSE_1X1, 2>(pl, ws, st);
    } else if (g.kind == NCONV_DENSE_TRANSPOSED_4X4 && g.stride == 2) {
        ok = go_wgrad_nt<NCONV_DENSE_TRANSPOSED_4X4, 2>(pl, ws, st);
    }
    if (!ok) {
        *why = "no weight-gradient kernel for this (kind, stride, grouping)";
        return -95;
    }
    const int mn = pl.a.M * pl.a.N;
    hipLaunchKernelGGL(dense_wgrad_reduce<float>, dim3((mn + 63) / 64), dim3(kDT), 0, st, ws, pl.a.nks, mn, g.gw);
    return launch_status(why);
}

int launch_dense_wgrad(const nconv_dense_wgrad& g, float* ws, size_t ws_bytes, hipStream_t st, const char** why) {
    if (ws_bytes < dense_wgrad_workspace_bytes(g)) {
        *why = "workspace too small (see nconv_dense_wgrad_workspace_bytes)";
        return -22;
    }
    const int sp = tr_rows_split(g);
    if (!sp) return launch_dense_wgrad_main(g, ws, st, why);
    const nconv_dense_wgrad m = tr_rows_main(g);  // the large source's rows
    if (int rc = launch_dense_wgrad_main(m, ws, st, why)) return rc;
    const TrRowsGrid r = tr_rows_grid(g);
    double* part = reinterpret_cast<double*>(ws + ((main_wgrad_bytes(m) + 255) & ~(size_t)255) / sizeof(float));
    const float* xs = sp == 1 ? g.x1 : g.x0;
    const int cs = sp == 1 ? g.C1 : g.C0;
    hipLaunchKernelGGL(dense_wgrad_tr_rows, dim3(r.nslice * g.Cout), dim3(256), 0, st, xs, cs, g.H, g.W, g.gy, g.Cout,
                       g.Ho, g.Wo, r.nry, r.nrx, part);
    const int mn = cs * g.Cout * 16;
    hipLaunchKernelGGL(dense_wgrad_reduce<double>, dim3((mn + 63) / 64), dim3(kDT), 0, st, part, r.nslice, mn,
                       sp == 1 ? g.gw + (size_t)g.C0 * g.Cout * 16 : g.gw);
    return launch_status(why);
}

}  // namespace nconv
