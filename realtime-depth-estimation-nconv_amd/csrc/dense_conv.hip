// dense_conv.hip — dense convolutions of the RGB-guided model on the gfx950 matrix cores: the
// forward path (weight packing: dense_pack.hip; weight gradients: dense_wgrad.hip).
//
// The RGB encoder (models/step2.py:134-154) and the fusion decoder (step2.py:156-297) are plain
// K x C x R x S contractions, so they run as implicit GEMMs on v_mfma_f32_32x32x2_f32 (fp32 in,
// fp32 accumulate: exact f32 products, the precision of the reference's fp32 convolutions):
//   A = weights  [Cout][k]        (M = output channels, 32 or 64 per tile)
//   B = im2col   [k][pixel]       (N = 32 output columns of one output row)
//   k = (tap, input channel)      (K, input channels staged 8 at a time)
// A workgroup (4 waves) owns an output tile of TH rows x 32 columns x one output-channel tile of
// one image; each wave owns TH/4 rows. Per 8-channel chunk the input patch (with halo) and the
// chunk's packed weights are staged in LDS (loads for the next chunk issued before this chunk's
// MFMAs); an MFMA k-step pairs two input channels (lane half kk = lane >> 5 takes channel 2p + kk),
// so every operand read is one ds_read_b32 at a compile-time offset from a per-lane base. The
// epilogue applies bias (eval BatchNorm folded in by nconv_dense_pack), ReLU and the RGBEncoder
// 1x1 shortcut (computed from the centre tap of the same patch) and writes a channel range of the
// output tensor, so torch.cat of the decoder never materialises: convolutions write their half
// of the concatenated tensor and the next one reads two sources.
//
// Kinds: 3x3 pad 1 stride 1|2; 1x1 stride 1|2; ConvTranspose 4x4 stride 2 pad 1 as four
// output-parity classes, each a 2x2 gather over the input's 3x3 neighbourhood (output 2H or,
// cropped, 2H-1); Conv 4x4 stride 2 pad 1. Output channels are tiled by 32 or 64
// (dense_cout_tile), one tile per workgroup, so any Cout runs.
#include "dense_common.h"

namespace nconv {

constexpr int kDenseTh32 = 1;  // row multiplier of the 32-output-channel tiles (2: 8-12 % slower)

int dense_cout_tile(int Cout) {
    if (Cout <= 32) return 32;
    const int p32 = (Cout + 31) / 32 * 32, p64 = (Cout + 63) / 64 * 64;
    return p32 < p64 ? 32 : 64;  // less padding; ties: 64 (the patch is staged once, not twice)
}

template <int COUT, int KIND, int S>
struct DcCfg {
    static constexpr bool TR = KIND == NCONV_DENSE_TRANSPOSED_4X4;
    static constexpr int TAPS = dense_taps(KIND);
    static constexpr int SP = TR ? 1 : S;                 // patch stride
    static constexpr int KS = KIND == NCONV_DENSE_1X1 ? 1 : (KIND == NCONV_DENSE_CONV4X4_S2 ? 4 : 3);
    static constexpr int PAD = KIND == NCONV_DENSE_1X1 ? 0 : 1;
    // rows per wave: 4 (2 strided) with 32 output channels, 2 (1) with 64: 4 MFMAs per 4-5 LDS reads
    static constexpr int TH = (SP == 1 ? 8 : 4) * (COUT == 32 ? kDenseTh32 : 1), RW = TH / 4, TW = 32;
    static constexpr int PR = (TH - 1) * SP + KS, PC = (TW - 1) * SP + KS;
    static constexpr int ROW = PC;
    // B reads (ds_read_b32): 32 lanes on the columns of one patch row form one bank group, lane
    // half kk (the other group) the next channel plane, so the planes need no padding and the
    // patch image is the linear element order: element e of the chunk lands at lds[e].
    static constexpr int PLANE = PR * ROW;
    static constexpr int MT = COUT / 32;
    static constexpr int COP = COUT == 32 ? 32 : 96;      // A reads: kk * COP == 32 (mod 64)
    static constexpr int W_OFF = (kCK * PLANE + 3) & ~3;  // 16-byte aligned weight rows
    static constexpr int WS_OFF = W_OFF + TAPS * kCK * COP;  // shortcut weights [ci][COP]
    static constexpr int LDS = WS_OFF + kCK * COP;
    static constexpr int NP = (kCK * PR * PC + kDT - 1) / kDT;        // patch elements per thread
    static constexpr int NW4 = (TAPS * kCK * COUT / 4 + kDT - 1) / kDT;  // weight float4s per thread
    static constexpr int NS4 = (kCK * COUT / 4 + kDT - 1) / kDT;
    static constexpr int CENTER = KIND == NCONV_DENSE_3X3 ? 4 : 0;   // tap of the 1x1 shortcut
};

template <int COUT, int KIND, int S, bool SC, bool STR = false>
__global__ __launch_bounds__(kDT) void dense_conv_mfma(nconv_dense_conv p, int ntx, int nty, int ncot) {
    using C = DcCfg<COUT, KIND, S>;
    __shared__ __attribute__((aligned(16))) float lds[C::LDS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    int blk = blockIdx.x;
    const int tx = blk % ntx;
    blk /= ntx;
    const int ty = blk % nty;
    blk /= nty;
    const int cot = blk % ncot;  // output-channel tile
    blk /= ncot;
    const int cls = C::TR ? blk % 4 : 0;  // output parity class (transposed)
    const int b = C::TR ? blk / 4 : blk;
    const int pa = cls >> 1, pb = cls & 1;
    const int oy0 = ty * C::TH, ox0 = tx * C::TW;  // tile origin (output grid, or class grid)
    const int iy0 = oy0 * C::SP - C::PAD, ix0 = ox0 * C::SP - C::PAD;  // patch origin in the input
    const int Cin = p.C0 + p.C1;
    const int nchunk = (Cin + kCK - 1) / kCK;
    const int HW = p.H * p.W;

    // ---- staging: patch (8 channels x PR x PC, zero outside the image / past Cin) + weights ----
    // Each thread's patch elements keep one byte offset each within a channel plane of the source
    // (out-of-image elements: past the buffer's end, read as 0), computed once; a chunk's loads are
    // buffer loads of that offset from a per-chunk resource (the chunk's first channel) -- no
    // address arithmetic per chunk. Channels past Cin read past the resource's end (0) as well.
    constexpr unsigned OOB = 0x80000000u;
    unsigned poff[C::NP];
#pragma unroll
    for (int k = 0; k < C::NP; ++k) {
        const int e = tid + kDT * k;
        const int ci = e / (C::PR * C::PC), rem = e - ci * (C::PR * C::PC);
        const int r = rem / C::PC, c = rem - r * C::PC;
        const int iy = iy0 + r, ix = ix0 + c;
        const bool in = e < kCK * C::PR * C::PC && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
        poff[k] = in ? (unsigned)(ci * HW + iy * p.W + ix) * 4u : OOB;
    }
    const int bytes0 = p.C0 * HW * 4, bytes1 = p.C1 * HW * 4;
    float pv[C::NP], pv1[STR ? C::NP : 1];
    unsigned pshift = 0;
    f4 wv[C::NW4], sv[C::NS4];
    // Branch-free (a branch here made the compiler wait for the chunk's loads at the join, right
    // after issuing them, instead of behind the chunk's MFMAs): with STR == false (the host found
    // no chunk straddling the two sources) one load per element from a per-chunk resource chosen
    // by uniform selects; with STR, two loads per element, the wrong source's out of range.
    auto load_chunk = [&](int ch) {
        const int g0 = ch * kCK;  // first channel of the chunk
        if constexpr (!STR) {
            const bool a = g0 < p.C0;
            const float* base = a ? p.x0 + ((size_t)b * p.C0 + g0) * HW
                                  : p.x1 + ((size_t)b * p.C1 + (g0 - p.C0)) * HW;
            const int nbytes = a ? bytes0 - g0 * HW * 4 : bytes1 - (g0 - p.C0) * HW * 4;
            const __amdgpu_buffer_rsrc_t rs = plane_rsrc(base, nbytes);
#pragma unroll
            for (int k = 0; k < C::NP; ++k) pv[k] = ld_f32(rs, poff[k]);
        } else {  // a chunk may straddle the two sources: both loads, the wrong one out of range
            // x0's part: channels g0 .. C0-1 (none once g0 >= C0); x1's channel 0 sits at chunk
            // offset `shift` (negative once g0 > C0: the resource then starts at x1's channel g0 - C0)
            const bool a0 = g0 < p.C0;
            const __amdgpu_buffer_rsrc_t r0 = plane_rsrc(p.x0 + ((size_t)b * p.C0 + (a0 ? g0 : 0)) * HW,
                                                         a0 ? bytes0 - g0 * HW * 4 : 0);
            const int c1 = a0 ? 0 : g0 - p.C0;
            const __amdgpu_buffer_rsrc_t r1 = plane_rsrc(p.x1 + ((size_t)b * p.C1 + c1) * HW, bytes1 - c1 * HW * 4);
            const unsigned shift = a0 ? (unsigned)(p.C0 - g0) * HW * 4u : 0u;
            pshift = shift;  // the two values are selected at store time, not here (no wait)
#pragma unroll
            for (int k = 0; k < C::NP; ++k) {
                const bool in1 = poff[k] != OOB && poff[k] >= shift;
                pv[k] = ld_f32(r0, poff[k]);
                pv1[k] = ld_f32(r1, in1 ? poff[k] - shift : OOB);
            }
        }
        const f4* wg = reinterpret_cast<const f4*>(
            p.wpack + (((size_t)cls * ncot + cot) * nchunk + ch) * C::TAPS * kCK * COUT);
#pragma unroll
        for (int k = 0; k < C::NW4; ++k) {
            const int e = tid + kDT * k;
            if (e < C::TAPS * kCK * COUT / 4) wv[k] = wg[e];
        }
        if constexpr (SC) {
            const f4* sg = reinterpret_cast<const f4*>(p.wshort + ((size_t)cot * nchunk + ch) * kCK * COUT);
#pragma unroll
            for (int k = 0; k < C::NS4; ++k) {
                const int e = tid + kDT * k;
                if (e < kCK * COUT / 4) sv[k] = sg[e];
            }
        }
    };
    auto store_chunk = [&]() {
#pragma unroll
        for (int k = 0; k < C::NP; ++k) {
            const int e = tid + kDT * k;
            float v = pv[k];
            if constexpr (STR) v = (poff[k] != OOB && poff[k] >= pshift) ? pv1[k] : v;
            if (e < kCK * C::PR * C::PC) lds[e] = v;
        }
#pragma unroll
        for (int k = 0; k < C::NW4; ++k) {
            const int e = tid + kDT * k;
            if (e < C::TAPS * kCK * COUT / 4) {
                const int row = e / (COUT / 4), c4 = e - row * (COUT / 4);
                *reinterpret_cast<f4*>(&lds[C::W_OFF + row * C::COP + 4 * c4]) = wv[k];
            }
        }
        if constexpr (SC) {
#pragma unroll
            for (int k = 0; k < C::NS4; ++k) {
                const int e = tid + kDT * k;
                if (e < kCK * COUT / 4) {
                    const int row = e / (COUT / 4), c4 = e - row * (COUT / 4);
                    *reinterpret_cast<f4*>(&lds[C::WS_OFF + row * C::COP + 4 * c4]) = sv[k];
                }
            }
        }
    };

    // ---- per-lane operand bases ----
    const int kk = lane >> 5, li = lane & 31;
    const int abase = C::W_OFF + kk * C::COP + li;               // + (tap*8 + 2p)*COP + mt*32
    const int sbase = C::WS_OFF + kk * C::COP + li;
    const int bbase = kk * C::PLANE + (w * C::RW * C::SP + (C::TR ? pa : 0)) * C::ROW + li * C::SP + (C::TR ? pb : 0);

    f16v acc[C::MT][C::RW], acs[SC ? C::MT : 1][SC ? C::RW : 1];
#pragma unroll
    for (int m = 0; m < C::MT; ++m)
#pragma unroll
        for (int r = 0; r < C::RW; ++r) {
            acc[m][r] = (f16v){};
            if constexpr (SC) acs[m][r] = (f16v){};
        }

    load_chunk(0);
#pragma unroll 1
    for (int ch = 0; ch < nchunk; ++ch) {
        if (ch) __syncthreads();  // the previous chunk's MFMAs are done with the LDS
        store_chunk();
        __syncthreads();
        load_chunk(ch + 1 < nchunk ? ch + 1 : ch);  // next chunk in flight during the MFMAs
        // taps one per iteration (not unrolled: unrolling all 9 x 4 k-steps lets the scheduler
        // hoist every operand read of the chunk into registers); the 4 channel pairs unrolled
#pragma unroll 1
        for (int t = 0; t < C::TAPS; ++t) {
            // patch offset of this tap: (kh, kw); transposed: the parity class picks rows
            // (1 - tr) + pa and columns (1 - tc) + pb (pa, pb folded into bbase)
            const int dr = C::TR ? 1 - t / 2 : t / C::KS;
            const int dc = C::TR ? 1 - t % 2 : t % C::KS;
            const float* ap = lds + abase + t * kCK * C::COP;
            const float* bp = lds + bbase + dr * C::ROW + dc;
#pragma unroll
            for (int pp = 0; pp < kCK / 2; ++pp) {
                float av[C::MT], bv[C::RW];
#pragma unroll
                for (int m = 0; m < C::MT; ++m) av[m] = ap[2 * pp * C::COP + 32 * m];
#pragma unroll
                for (int r = 0; r < C::RW; ++r) bv[r] = bp[2 * pp * C::PLANE + r * C::SP * C::ROW];
#pragma unroll
                for (int m = 0; m < C::MT; ++m)
#pragma unroll
                    for (int r = 0; r < C::RW; ++r)
                        acc[m][r] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m], bv[r], acc[m][r], 0, 0, 0);
                if constexpr (SC) {
                    if (t == C::CENTER) {
#pragma unroll
                        for (int m = 0; m < C::MT; ++m) {
                            const float sa = lds[sbase + 2 * pp * C::COP + 32 * m];
#pragma unroll
                            for (int r = 0; r < C::RW; ++r)
                                acs[m][r] = __builtin_amdgcn_mfma_f32_32x32x2f32(sa, bv[r], acs[m][r], 0, 0, 0);
                        }
                    }
                }
            }
        }
    }
    // ---- epilogue: bias, ReLU, shortcut; C[row = co][col = pixel]: col = lane & 31,
    //      row = (q & 3) + 8 (q >> 2) + 4 (lane >> 5) for register q. Stores through one
    //      resource over the image's output channel range: the lane's byte offset (its pixel and
    //      lane-half channel) once, each register's channel offset a uniform soffset; pixels and
    //      channels outside the output are dropped by the range check ----
    const int Hc = C::TR ? p.H : p.Ho, Wc = C::TR ? p.W : p.Wo;  // (class) grid
    const int ox = ox0 + li;
    const int HWo = p.Ho * p.Wo;
    const int co0 = cot * COUT;  // first output channel of this tile
    const int nco = p.Cout - co0 < COUT ? p.Cout - co0 : COUT;
    const __amdgpu_buffer_rsrc_t ro =
        plane_rsrc(p.out + ((size_t)b * p.out_C + p.out_c0 + co0) * HWo, nco * HWo * 4);
#pragma unroll
    for (int r = 0; r < C::RW; ++r) {
        const int oy = oy0 + w * C::RW + r;
        const int oyo = C::TR ? 2 * oy + pa : oy, oxo = C::TR ? 2 * ox + pb : ox;
        const bool in = oy < Hc && ox < Wc && oyo < p.Ho && oxo < p.Wo;  // (cropped transposed output)
        const unsigned lo = in ? (unsigned)(4 * kk * HWo + oyo * p.Wo + oxo) * 4u : OOB;
#pragma unroll
        for (int m = 0; m < C::MT; ++m)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int cr = 32 * m + (q & 3) + 8 * (q >> 2);  // channel in the tile, lane half 0
                const int co = co0 + cr + 4 * kk;
                float v = acc[m][r][q] + ((p.bias && co < p.Cout) ? p.bias[co] : 0.f);
                if (p.relu) v = fmaxf(v, 0.f);
                if constexpr (SC) v += acs[m][r][q];
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), ro, (int)lo, cr * HWo * 4, 0);
            }
    }
}

// ------------------------------------------------------------------------------------------------
// 3x3 stride-1 convolution with exact products on the bf16 matrix cores (NCONV_DENSE_MATH_BF16X9;
// NCONV_DENSE_MATH_BF16X6: the six largest partial products).
// Every fp32 operand v is split into three bf16 parts v = v0 + v1 + v2 (v0 = bf16(v),
// v1 = bf16(v - v0), v2 = v - v0 - v1: at most 8 significant bits, exact), so each of the nine
// partial products vi*wj is exact in fp32 and their sum is v*w exactly; the only rounding is the
// fp32 accumulation, as in the fp32-MFMA kernel above (which is an fmaf chain, bitwise; this one
// sums in another order, so results agree to fp32 accumulation error, not bitwise). Nine
// v_mfma_f32_32x32x16_bf16 (32 cycles each) per 32x32x16 block against eight
// v_mfma_f32_32x32x2_f32 (64 cycles each): 288 against 512 cycles.
// GEMM as above (A = weights, B = patch, C[co][pixel]), with k = (tap pair, 8 input channels): a
// k-step takes taps 2s (lane half 0) and 2s + 1 (lane half 1) of one 8-channel chunk; the tenth
// tap is zero (A rows zero, B fragment zeroed). LDS images, every fragment one ds_read_b128 of 32
// consecutive 16-byte entries:
//   patch   [part 3][position PR x PC][8 channels]         (bf16x8 per position and part)
//   weights [k-step 5][part 3][lane half 2][co COUT][8 ci]  (bf16x8 per row)
// ------------------------------------------------------------------------------------------------
template <int COUT, int KIND = NCONV_DENSE_3X3, int S = 1, bool SC = false>
struct Db9Cfg {  // (16 rows for the 32-channel tiles, 2 waves/SIMD: not faster)
    static constexpr bool TR = KIND == NCONV_DENSE_TRANSPOSED_4X4;  // four output-parity classes
    static constexpr int TAPS = dense_taps(KIND), NKS = (TAPS + 1) / 2;  // k-steps: tap pairs
    static constexpr int KS = KIND == NCONV_DENSE_CONV4X4_S2 ? 4 : 3;    // patch extent per pixel
    static constexpr int SP = TR ? 1 : S;                            // patch stride
    static constexpr int TH = SP == 1 ? 8 : 4, RW = TH / 4, TW = 32, MT = COUT / 32;
    static constexpr int PR = (TH - 1) * SP + KS, PC = (TW - 1) * SP + KS, ROW = PC, NPOS = PR * PC;
    static constexpr int PLANEB = NPOS * 16;                         // bytes of one part's image
    static constexpr int DUMP = 3 * PLANEB;                          // slot of positions past the tile
    static constexpr int WOFF = DUMP + 3 * 16;                       // weight image (bytes)
    static constexpr int WROWS = NKS * 3 * 2 * COUT;                 // 16-byte rows per chunk
    static constexpr int NWL = (WROWS + kDT - 1) / kDT;              // rows per thread (the last
    static constexpr int SOFF = WOFF + NWL * kDT * 16;               //  round's excess: zeros, past the image)
    static constexpr int SROWS = SC ? 3 * 2 * COUT : 0;              // shortcut image rows per chunk
    static constexpr int NSL = (SROWS + kDT - 1) / kDT;
    static constexpr int LDSB = SOFF + NSL * kDT * 16;
    static constexpr int NPP = (NPOS + kDT - 1) / kDT;               // positions per thread
    // tap t's patch offset (row, column) from the pixel's patch origin (transposed: the parity
    // class's (pa, pb) added at run time)
    static constexpr int tr_(int t) { return TR ? 1 - t / 2 : t / KS; }
    static constexpr int tc_(int t) { return TR ? 1 - t % 2 : t % KS; }
    static constexpr int off(int t) { return tr_(t) * ROW + tc_(t); }
    // lane half 1's offset from lane half 0's in k-step s (the padded tenth tap of a 3x3: 0)
    static constexpr int delta(int s) { return 2 * s + 1 < TAPS ? off(2 * s + 1) - off(2 * s) : 0; }
};

constexpr int kDb9KUnroll = 5;                  // k-steps per unrolled body (1: 4 % slower)
constexpr int kDb9Waves64 = 2, kDb9Waves32 = 3;  // waves per SIMD asked for, 64- / 32-channel tiles

template <int COUT, int NTERM, int KIND, int S, bool SC>
__global__ __launch_bounds__(kDT) __attribute__((amdgpu_waves_per_eu(COUT == 64 ? kDb9Waves64 : kDb9Waves32)))
void dense_conv_bf9(nconv_dense_conv p, int ntx, int nty, int ncot) {
    using C = Db9Cfg<COUT, KIND, S, SC>;
    __shared__ __attribute__((aligned(16))) unsigned char lds[C::LDSB];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    int blk = blockIdx.x;
    const int tx = blk % ntx;
    blk /= ntx;
    const int ty = blk % nty;
    blk /= nty;
    const int cot = blk % ncot;
    blk /= ncot;
    const int cls = C::TR ? blk % 4 : 0;  // output parity class (transposed)
    const int b = C::TR ? blk / 4 : blk;
    const int pa = cls >> 1, pb = cls & 1;
    const int oy0 = ty * C::TH, ox0 = tx * C::TW;  // tile origin (output grid, or class grid)
    const int iy0 = oy0 * C::SP - 1, ix0 = ox0 * C::SP - 1;
    const int Cin = p.C0 + p.C1;
    const int nchunk = (Cin + kCK - 1) / kCK;
    const int HW = p.H * p.W;

    constexpr unsigned OOB = 0x80000000u;
    unsigned poff[C::NPP];
#pragma unroll
    for (int k = 0; k < C::NPP; ++k) {
        const int e = tid + kDT * k;
        const int r = e / C::PC, c = e - r * C::PC;
        const int iy = iy0 + r, ix = ix0 + c;
        const bool in = e < C::NPOS && (unsigned)iy < (unsigned)p.H && (unsigned)ix < (unsigned)p.W;
        poff[k] = in ? (unsigned)(iy * p.W + ix) * 4u : OOB;
    }
    // each source's planes of image b behind one resource; a chunk's channel c comes from x0 or
    // x1 by a uniform select (a chunk may straddle the two), channels past Cin read past x1's end
    const __amdgpu_buffer_rsrc_t rs0 = plane_rsrc(p.x0 + (size_t)b * p.C0 * HW, p.C0 * HW * 4);
    const __amdgpu_buffer_rsrc_t rs1 =
        plane_rsrc(p.C1 > 0 ? p.x1 + (size_t)b * p.C1 * HW : p.x0, p.C1 > 0 ? p.C1 * HW * 4 : 0);
    // the pre-split weight image of (class, cot, chunk) behind the fp32 one (nconv_dense_pack)
    const size_t fp32_floats = (size_t)(C::TR ? 4 : 1) * ncot * nchunk * C::TAPS * kCK * COUT;
    const unsigned char* wimg = reinterpret_cast<const unsigned char*>(p.wpack + fp32_floats) +
                                ((size_t)cls * ncot + cot) * nchunk * C::WROWS * 16;
    // the shortcut's pre-split image (a 1x1 nconv_dense_pack: [cot][chunk][part][half][co], half 1 zero)
    const unsigned char* simg = SC ? reinterpret_cast<const unsigned char*>(p.wshort + (size_t)ncot * nchunk * kCK * COUT) +
                                         (size_t)cot * nchunk * C::SROWS * 16
                                   : nullptr;
    float pv[C::NPP][8];
    du4 wv[C::NWL], sv[SC ? C::NSL : 1];
    auto load_chunk = [&](int ch) {
        const int g0 = ch * kCK;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int g = g0 + c;
            const bool a = g < p.C0;
            const __amdgpu_buffer_rsrc_t rs = a ? rs0 : rs1;
            const int so = (a ? g : g - p.C0) * HW * 4;
#pragma unroll
            for (int k = 0; k < C::NPP; ++k) pv[k][c] = ld_f32s(rs, poff[k], so);
        }
        const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(
            (void*)(wimg + (size_t)ch * C::WROWS * 16), (short)0, C::WROWS * 16, 0x00020000);
#pragma unroll
        for (int k = 0; k < C::NWL; ++k) wv[k] = __builtin_amdgcn_raw_buffer_load_b128(rw, (tid + kDT * k) * 16, 0, 0);
        if constexpr (SC) {
            const __amdgpu_buffer_rsrc_t rsc = __builtin_amdgcn_make_buffer_rsrc(
                (void*)(simg + (size_t)ch * C::SROWS * 16), (short)0, C::SROWS * 16, 0x00020000);
#pragma unroll
            for (int k = 0; k < C::NSL; ++k) sv[k] = __builtin_amdgcn_raw_buffer_load_b128(rsc, (tid + kDT * k) * 16, 0, 0);
        }
    };
    auto store_chunk = [&](unsigned char* L) {
#pragma unroll
        for (int k = 0; k < C::NPP; ++k) {
            const int e = tid + kDT * k;
            dbf16x8 sp[3];
            dsplit3(pv[k], sp);
            const bool in = e < C::NPOS;  // past the tile: the dump slots (no branch)
            const int a = in ? e * 16 : C::DUMP, da = in ? C::PLANEB : 16;
#pragma unroll
            for (int i = 0; i < 3; ++i) *reinterpret_cast<dbf16x8*>(L + a + i * da) = sp[i];
        }
#pragma unroll
        for (int k = 0; k < C::NWL; ++k) *reinterpret_cast<du4*>(L + C::WOFF + (tid + kDT * k) * 16) = wv[k];
        if constexpr (SC) {
#pragma unroll
            for (int k = 0; k < C::NSL; ++k) *reinterpret_cast<du4*>(L + C::SOFF + (tid + kDT * k) * 16) = sv[k];
        }
    };

    const int kk = lane >> 5, li = lane & 31;
    const int abase = C::WOFF + (kk * COUT + li) * 16;
    const int sbase = C::SOFF + (kk * COUT + li) * 16;
    const int bbase = ((w * C::RW * C::SP + (C::TR ? pa : 0)) * C::ROW + li * C::SP + (C::TR ? pb : 0)) * 16;

    f16v acc[C::MT][C::RW], acs[SC ? C::MT : 1][SC ? C::RW : 1];
#pragma unroll
    for (int m = 0; m < C::MT; ++m)
#pragma unroll
        for (int r = 0; r < C::RW; ++r) {
            acc[m][r] = (f16v){};
            if constexpr (SC) acs[m][r] = (f16v){};
        }

    auto mma_chunk = [&](const unsigned char* L) {
#pragma unroll kDb9KUnroll
        for (int s = 0; s < C::NKS; ++s) {
            // lane half 0: tap 2s, lane half 1: tap 2s + 1 (C::delta(s) positions further)
            const int bb = bbase + (kk ? C::delta(s) * 16 : 0) + C::off(2 * s) * 16;
            dbf16x8 av[3][C::MT], bv[3][C::RW];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int m = 0; m < C::MT; ++m)
                    av[i][m] = *reinterpret_cast<const dbf16x8*>(L + abase + (s * 3 + i) * 2 * COUT * 16 + 32 * m * 16);
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int r = 0; r < C::RW; ++r) {
                    bv[i][r] = *reinterpret_cast<const dbf16x8*>(L + bb + i * C::PLANEB + r * C::SP * C::ROW * 16);
                    if (2 * s + 1 == C::TAPS && kk) bv[i][r] = (dbf16x8){};  // the padded tap
                }
            // smallest terms first; NTERM 6 (bf16x6) drops the three below ~2^-23 |v w|
            constexpr int ti[9] = {2, 2, 1, 2, 1, 0, 1, 0, 0}, tj[9] = {2, 1, 2, 0, 1, 2, 0, 1, 0};
#pragma unroll
            for (int q = 9 - NTERM; q < 9; ++q)
#pragma unroll
                for (int m = 0; m < C::MT; ++m)
#pragma unroll
                    for (int r = 0; r < C::RW; ++r)
                        acc[m][r] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[ti[q]][m], bv[tj[q]][r], acc[m][r], 0, 0, 0);
            if constexpr (SC) {
                if (s == 2) {  // the 1x1 shortcut: the centre tap (lane half 0 of k-step 2; half 1's rows zero)
                    dbf16x8 as[3][C::MT];
#pragma unroll
                    for (int i = 0; i < 3; ++i)
#pragma unroll
                        for (int m = 0; m < C::MT; ++m)
                            as[i][m] = *reinterpret_cast<const dbf16x8*>(L + sbase + i * 2 * COUT * 16 + 32 * m * 16);
#pragma unroll
                    for (int q = 9 - NTERM; q < 9; ++q)
#pragma unroll
                        for (int m = 0; m < C::MT; ++m)
#pragma unroll
                            for (int r = 0; r < C::RW; ++r)
                                acs[m][r] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as[ti[q]][m], bv[tj[q]][r], acs[m][r], 0, 0, 0);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    };

    // (two LDS images, the next chunk stored under this one's MFMAs with one barrier per chunk,
    // measured 7-13 % slower for the 32-channel tiles: two workgroups per CU instead of three)
    load_chunk(0);
#pragma unroll 1
    for (int ch = 0; ch < nchunk; ++ch) {
        store_chunk(lds);
        __syncthreads();
        load_chunk(ch + 1 < nchunk ? ch + 1 : ch);  // next chunk in flight during the MFMAs
        mma_chunk(lds);
        __syncthreads();  // this chunk's MFMAs are done with the LDS
    }
    const int Hc = C::TR ? p.H : p.Ho, Wc = C::TR ? p.W : p.Wo;  // (class) grid
    const int ox = ox0 + li;
    const int HWo = p.Ho * p.Wo;
    const int co0 = cot * COUT;
    const int nco = p.Cout - co0 < COUT ? p.Cout - co0 : COUT;
    const __amdgpu_buffer_rsrc_t ro = plane_rsrc(p.out + ((size_t)b * p.out_C + p.out_c0 + co0) * HWo, nco * HWo * 4);
#pragma unroll
    for (int r = 0; r < C::RW; ++r) {
        const int oy = oy0 + w * C::RW + r;
        const int oyo = C::TR ? 2 * oy + pa : oy, oxo = C::TR ? 2 * ox + pb : ox;
        const bool in = oy < Hc && ox < Wc && oyo < p.Ho && oxo < p.Wo;  // (cropped transposed output)
        const unsigned lo = in ? (unsigned)(4 * kk * HWo + oyo * p.Wo + oxo) * 4u : OOB;
#pragma unroll
        for (int m = 0; m < C::MT; ++m)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int cr = 32 * m + (q & 3) + 8 * (q >> 2);
                const int co = co0 + cr + 4 * kk;
                float v = acc[m][r][q] + ((p.bias && co < p.Cout) ? p.bias[co] : 0.f);
                if (p.relu) v = fmaxf(v, 0.f);
                if constexpr (SC) v += acs[m][r][q];
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), ro, (int)lo, cr * HWo * 4, 0);
            }
    }
}

// ---- 3x3 convolution to ONE output channel + residual (the depth heads, step2.py:259,278):
//      out = conv3x3(x, pad 1) + res. Thread = 4 adjacent pixels of a 16 x 64 tile; input
//      channels staged CB planes per barrier (the next group's loads in flight during
//      this group's FMAs; the sums in the same channel order as one plane at a time, bitwise);
//      weights are wave-uniform (SGPR). ---------------------------------------------------------
__global__ __launch_bounds__(kDT) void conv3x3_c1(const float* __restrict__ x, int Cin, int H, int W,
                                                 const float* __restrict__ wt, const float* __restrict__ res,
                                                 float* __restrict__ out, int ntx, int nty) {
    constexpr int TW = 64, TH = 16, PW = TW + 2, PH = TH + 2, CB = 4;
    constexpr int NE = (PH * PW + kDT - 1) / kDT;
    __shared__ float pl[2][CB][PH * PW];
    int blk = blockIdx.x;
    const int tx = blk % ntx;
    blk /= ntx;
    const int ty = blk % nty, b = blk / nty;
    const int tid = threadIdx.x;
    const int r = tid >> 4, c0 = (tid & 15) * 4;
    const int y0 = ty * TH, x0 = tx * TW;
    const size_t HW = (size_t)H * W;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    float st[CB][NE];
    unsigned off[NE];  // each staged element's offset in its plane (0x80000000: outside, reads 0)
#pragma unroll
    for (int k = 0; k < NE; ++k) {
        const int e = tid + kDT * k;
        const int pr = e / PW, pc = e - pr * PW;
        const int iy = y0 - 1 + pr, ix = x0 - 1 + pc;
        const bool in = e < PH * PW && (unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W;
        off[k] = in ? (unsigned)(iy * W + ix) * 4u : 0x80000000u;
    }
    const __amdgpu_buffer_rsrc_t rx = plane_rsrc(x + (size_t)b * Cin * HW, (int)(Cin * HW * 4));
    auto load = [&](int c) {  // channels c .. c + CB - 1 (past Cin: out of range, 0)
#pragma unroll
        for (int q = 0; q < CB; ++q)
#pragma unroll
            for (int k = 0; k < NE; ++k) st[q][k] = ld_f32s(rx, off[k], (c + q) * (int)HW * 4);
    };
    load(0);
#pragma unroll 1
    for (int cg = 0; cg < Cin; cg += CB) {
        float(*t)[PH * PW] = pl[(cg / CB) & 1];
#pragma unroll
        for (int q = 0; q < CB; ++q)
#pragma unroll
            for (int k = 0; k < NE; ++k) {
                const int e = tid + kDT * k;
                if (e < PH * PW) t[q][e] = st[q][k];
            }
        __syncthreads();
        load(cg + CB < Cin ? cg + CB : cg);
#pragma unroll
        for (int q = 0; q < CB; ++q) {
            if (cg + q >= Cin) break;
            const float* wr = wt + (cg + q) * 9;
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
                float v[6];
#pragma unroll
                for (int m = 0; m < 6; ++m) v[m] = t[q][(r + kh) * PW + c0 + m];
#pragma unroll
                for (int kw = 0; kw < 3; ++kw)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[j] = fmaf(wr[kh * 3 + kw], v[j + kw], acc[j]);
            }
        }
    }
    const int y = y0 + r;
    if (y >= H) return;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int xx = x0 + c0 + j;
        if (xx < W) {
            const size_t i = (size_t)b * HW + (size_t)y * W + xx;
            out[i] = acc[j] + (res ? res[i] : 0.f);
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Launchers
// ------------------------------------------------------------------------------------------------
template <int COUT, int KIND, int S, bool SC>
static void go_dense(const nconv_dense_conv& p, hipStream_t st) {
    using C = DcCfg<COUT, KIND, S>;
    const int Hc = C::TR ? p.H : p.Ho, Wc = C::TR ? p.W : p.Wo;
    const int ntx = (Wc + C::TW - 1) / C::TW, nty = (Hc + C::TH - 1) / C::TH;
    const int ncot = (p.Cout + COUT - 1) / COUT;
    const int blocks = ntx * nty * ncot * p.B * (C::TR ? 4 : 1);
    if (p.C1 > 0 && p.C0 % kCK != 0)  // a chunk holds channels of both sources
        hipLaunchKernelGGL((dense_conv_mfma<COUT, KIND, S, SC, true>), dim3(blocks), dim3(kDT), 0, st, p, ntx, nty,
                           ncot);
    else
        hipLaunchKernelGGL((dense_conv_mfma<COUT, KIND, S, SC, false>), dim3(blocks), dim3(kDT), 0, st, p, ntx,
                           nty, ncot);
}
// the fp32 kernel of (kind, stride, shortcut): 3x3 stride 1|2 with or without the fused shortcut,
// 1x1 stride 1|2, transposed 4x4 and 4x4 stride 2; false: no such kernel
template <int COUT>
static bool go_dense_k(const nconv_dense_conv& p, bool sc, hipStream_t st) {
    if (p.stride != 1 && p.stride != 2) return false;
    switch (p.kind) {
    case NCONV_DENSE_3X3:
        if (p.stride == 1)
            sc ? go_dense<COUT, NCONV_DENSE_3X3, 1, true>(p, st) : go_dense<COUT, NCONV_DENSE_3X3, 1, false>(p, st);
        else
            sc ? go_dense<COUT, NCONV_DENSE_3X3, 2, true>(p, st) : go_dense<COUT, NCONV_DENSE_3X3, 2, false>(p, st);
        return true;
    case NCONV_DENSE_1X1:
        if (sc) return false;
        p.stride == 1 ? go_dense<COUT, NCONV_DENSE_1X1, 1, false>(p, st) : go_dense<COUT, NCONV_DENSE_1X1, 2, false>(p, st);
        return true;
    case NCONV_DENSE_TRANSPOSED_4X4:
        if (sc || p.stride != 2) return false;
        go_dense<COUT, NCONV_DENSE_TRANSPOSED_4X4, 2, false>(p, st);
        return true;
    case NCONV_DENSE_CONV4X4_S2:
        if (sc || p.stride != 2) return false;
        go_dense<COUT, NCONV_DENSE_CONV4X4_S2, 2, false>(p, st);
        return true;
    }
    return false;
}

template <int COUT, int NTERM, int KIND, int S, bool SC>
static void go_dense_bf9(const nconv_dense_conv& p, hipStream_t st) {
    using C = Db9Cfg<COUT, KIND, S, SC>;
    const int Hc = C::TR ? p.H : p.Ho, Wc = C::TR ? p.W : p.Wo;
    const int ntx = (Wc + C::TW - 1) / C::TW, nty = (Hc + C::TH - 1) / C::TH;
    const int ncot = (p.Cout + COUT - 1) / COUT;
    hipLaunchKernelGGL((dense_conv_bf9<COUT, NTERM, KIND, S, SC>), dim3(ntx * nty * ncot * p.B * (C::TR ? 4 : 1)),
                       dim3(kDT), 0, st, p, ntx, nty, ncot);
}
template <int COUT, int NTERM>
static void go_dense_bf9_k(const nconv_dense_conv& p, bool sc, hipStream_t st) {
    if (p.kind == NCONV_DENSE_TRANSPOSED_4X4)
        go_dense_bf9<COUT, NTERM, NCONV_DENSE_TRANSPOSED_4X4, 2, false>(p, st);
    else if (p.kind == NCONV_DENSE_CONV4X4_S2)
        go_dense_bf9<COUT, NTERM, NCONV_DENSE_CONV4X4_S2, 2, false>(p, st);
    else if (p.stride == 1)
        sc ? go_dense_bf9<COUT, NTERM, NCONV_DENSE_3X3, 1, true>(p, st) : go_dense_bf9<COUT, NTERM, NCONV_DENSE_3X3, 1, false>(p, st);
    else
        sc ? go_dense_bf9<COUT, NTERM, NCONV_DENSE_3X3, 2, true>(p, st) : go_dense_bf9<COUT, NTERM, NCONV_DENSE_3X3, 2, false>(p, st);
}

// p.math BF16X9 / BF16X6: every kind but the 1x1 (3x3 stride 1 or 2 with or without the fused
// shortcut, the transposed 4x4 and the 4x4 stride 2) on dense_conv_bf9; the 1x1 (half of each
// k-step would be padding) keeps the fp32 MFMA kernel
int launch_dense_conv(const nconv_dense_conv& p, hipStream_t st, const char** why) {
    const bool sc = p.wshort != nullptr;
    const int co = dense_cout_tile(p.Cout);
    if (p.math != NCONV_DENSE_MATH_FP32 && p.kind != NCONV_DENSE_1X1) {
        const int nt = p.math == NCONV_DENSE_MATH_BF16X9 ? 9 : 6;
        if (co == 32)
            nt == 9 ? go_dense_bf9_k<32, 9>(p, sc, st) : go_dense_bf9_k<32, 6>(p, sc, st);
        else
            nt == 9 ? go_dense_bf9_k<64, 9>(p, sc, st) : go_dense_bf9_k<64, 6>(p, sc, st);
        return launch_status(why);
    }
    if (!(co == 32 ? go_dense_k<32>(p, sc, st) : go_dense_k<64>(p, sc, st))) {
        *why = "no dense-conv kernel for this (kind, stride, shortcut) combination";
        return -95;
    }
    return launch_status(why);
}

int launch_conv3x3_c1(const float* x, int B, int Cin, int H, int W, const float* w, const float* res, float* out,
                      hipStream_t st, const char** why) {
    const int ntx = (W + 63) / 64, nty = (H + 15) / 16;
    hipLaunchKernelGGL(conv3x3_c1, dim3(ntx * nty * B), dim3(kDT), 0, st, x, Cin, H, W, w, res, out, ntx, nty);
    return launch_status(why);
}

}  // namespace nconv
