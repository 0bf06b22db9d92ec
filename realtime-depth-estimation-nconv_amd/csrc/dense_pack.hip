// dense_pack.hip — weight packing of the dense convolutions (dense_conv.hip): the fp32 image
// dense_conv_mfma stages, then the pre-split bf16 image of dense_conv_bf9.
#include "dense_common.h"

namespace nconv {

// ---- weight packing: (Cout, Cin, kh, kw) [conv] / (Cin, Cout, 4, 4) [transposed] ->
//      [class][cout tile][chunk][tap][ci 8][T], times an optional per-Cout scale (eval
//      BatchNorm); channels past Cin / Cout are zero ----------------------------------------------
// 3x3: one wave per (output-channel tile, input chunk, 8 output channels): their 8 x 8 x 9
// weights (72 contiguous floats per output channel) read coalesced into LDS, then both images'
// entries of those channels written from there (32-byte / 128-byte runs)
template <int T>
__global__ __launch_bounds__(64) void dense_pack3x3(int Cin, int Cout, const float* w, const float* scale,
                                                    float* wp) {
    constexpr int G = 8;  // output channels per wave
    __shared__ float wt[G * 73];
    const int nchunk = (Cin + kCK - 1) / kCK, ncot = (Cout + T - 1) / T;
    int blk = blockIdx.x;
    const int sub = blk % (T / G);
    blk /= T / G;
    const int ch = blk % nchunk, cot = blk / nchunk;
    const int tid = threadIdx.x, c0 = sub * G;
    float v[G * 72 / 64], sc[G * 72 / 64];  // all loads in flight together
#pragma unroll
    for (int k = 0; k < G * 72 / 64; ++k) {
        const int e = tid + 64 * k, col = e / 72, rem = e - col * 72;
        const int o = cot * T + c0 + col, ci = ch * kCK + rem / 9;
        const bool in = o < Cout && ci < Cin;
        v[k] = in ? w[((size_t)o * Cin + ch * kCK) * 9 + rem] : 0.f;
        sc[k] = in && scale ? scale[o] : 1.f;
    }
#pragma unroll
    for (int k = 0; k < G * 72 / 64; ++k) {
        const int e = tid + 64 * k, col = e / 72, rem = e - col * 72;
        wt[col * 73 + rem] = v[k] * sc[k];
    }
    __syncthreads();
    float* f = wp + ((size_t)cot * nchunk + ch) * 9 * kCK * T;  // [tap][ci][T]
    for (int e = tid; e < 72 * G; e += 64) {
        const int col = e % G, r = e / G, cil = r % kCK, t = r / kCK;
        f[r * T + c0 + col] = wt[col * 73 + cil * 9 + t];
    }
    unsigned char* img = reinterpret_cast<unsigned char*>(wp + (size_t)ncot * nchunk * 9 * kCK * T) +
                         ((size_t)cot * nchunk + ch) * 30 * T * 16;
    for (int e = tid; e < 30 * G; e += 64) {
        const int col = e % G, r = e / G, kk = r % 2, part = (r / 2) % 3, s = r / 6, tap = 2 * s + kk;
        float v[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = tap < 9 ? wt[col * 73 + c * 9 + tap] : 0.f;
        dbf16x8 sp[3];
        dsplit3(v, sp);
        *reinterpret_cast<dbf16x8*>(img + ((size_t)r * T + c0 + col) * 16) = part == 0 ? sp[0] : part == 1 ? sp[1] : sp[2];
    }
}

// the other kinds: one thread per element of the fp32 image
__global__ __launch_bounds__(kDT) void dense_pack(int kind, int Cin, int Cout, int T, const float* w,
                                                  const float* scale, float* wp) {
    const int taps = dense_taps(kind);
    const int ncls = kind == NCONV_DENSE_TRANSPOSED_4X4 ? 4 : 1;
    const int nchunk = (Cin + kCK - 1) / kCK;
    const int ncot = (Cout + T - 1) / T;
    const size_t n = (size_t)ncls * ncot * nchunk * taps * kCK * T;
    for (size_t e = (size_t)blockIdx.x * kDT + threadIdx.x; e < n; e += (size_t)gridDim.x * kDT) {
        const int col = (int)(e % T);
        size_t r = e / T;
        const int cil = (int)(r % kCK);
        r /= kCK;
        const int t = (int)(r % taps);
        r /= taps;
        const int ch = (int)(r % nchunk);
        r /= nchunk;
        const int cot = (int)(r % ncot);
        const int cls = (int)(r / ncot);
        const int ci = ch * kCK + cil, co = cot * T + col;
        float v = 0.f;
        if (ci < Cin && co < Cout) {
            if (kind == NCONV_DENSE_3X3) {
                v = w[((size_t)co * Cin + ci) * 9 + t];
            } else if (kind == NCONV_DENSE_1X1) {
                v = w[(size_t)co * Cin + ci];
            } else if (kind == NCONV_DENSE_CONV4X4_S2) {
                v = w[((size_t)co * Cin + ci) * 16 + t];
            } else {  // ConvTranspose2d weight (Cin, Cout, 4, 4): class (pa, pb), tap (tr, tc)
                const int pa = cls >> 1, pb = cls & 1, tr = t >> 1, tc = t & 1;
                const int kh = 1 - pa + 2 * tr, kw = 1 - pb + 2 * tc;
                v = w[(((size_t)ci * Cout + co) * 4 + kh) * 4 + kw];
            }
            if (scale) v *= scale[co];
        }
        wp[e] = v;
    }
}

// the pre-split image of the other kinds (1x1, transposed 4x4, 4x4 stride 2), one row per thread
// (3x3: dense_pack3x3); values as dense_pack's, then split
__global__ __launch_bounds__(kDT) void dense_pack_bf9(int kind, int Cin, int Cout, int T, const float* w,
                                                      const float* scale, unsigned char* img, size_t rows) {
    const int taps = dense_taps(kind), nks = (taps + 1) / 2;
    const int nchunk = (Cin + kCK - 1) / kCK, ncot = (Cout + T - 1) / T;
    for (size_t e = (size_t)blockIdx.x * kDT + threadIdx.x; e < rows; e += (size_t)gridDim.x * kDT) {
        const int col = (int)(e % T);
        size_t r = e / T;
        const int kk = (int)(r % 2);
        r /= 2;
        const int part = (int)(r % 3);
        r /= 3;
        const int s = (int)(r % nks);
        r /= nks;
        const int ch = (int)(r % nchunk);
        r /= nchunk;
        const int cot = (int)(r % ncot), cls = (int)(r / ncot);
        const int t = 2 * s + kk, co = cot * T + col;
        float v[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const int ci = ch * kCK + c;
            float x = 0.f;
            if (t < taps && ci < Cin && co < Cout) {
                if (kind == NCONV_DENSE_1X1) {
                    x = w[(size_t)co * Cin + ci];
                } else if (kind == NCONV_DENSE_CONV4X4_S2) {
                    x = w[((size_t)co * Cin + ci) * 16 + t];
                } else {  // ConvTranspose2d weight (Cin, Cout, 4, 4): class (pa, pb), tap (tr, tc)
                    const int pa = cls >> 1, pb = cls & 1, tr = t >> 1, tc = t & 1;
                    x = w[(((size_t)ci * Cout + co) * 4 + (1 - pa + 2 * tr)) * 4 + (1 - pb + 2 * tc)];
                }
                if (scale) x *= scale[co];
            }
            v[c] = x;
        }
        dbf16x8 sp[3];
        dsplit3(v, sp);
        *reinterpret_cast<dbf16x8*>(img + e * 16) = part == 0 ? sp[0] : part == 1 ? sp[1] : sp[2];
    }
}

// ---- sizes and launcher ----
static size_t dense_fp32_floats(int kind, int Cin, int Cout) {
    const int ncls = kind == NCONV_DENSE_TRANSPOSED_4X4 ? 4 : 1;
    const int T = dense_cout_tile(Cout);
    return (size_t)ncls * ((Cout + T - 1) / T) * ((Cin + kCK - 1) / kCK) * dense_taps(kind) * kCK * T;
}
// the fp32 image, then dense_conv_bf9's pre-split one: rows of 8 bf16 (16 bytes) in
// [class][cot][chunk][k-step][part][half][co] order, NKS k-steps of two taps (a padded odd tap and
// the 1x1's second half zero): 6 NKS T rows = 24 NKS T floats per (class, cot, chunk)
static size_t dense_bf9_floats(int kind, int Cin, int Cout) {
    const int ncls = kind == NCONV_DENSE_TRANSPOSED_4X4 ? 4 : 1;
    const int T = dense_cout_tile(Cout), nks = (dense_taps(kind) + 1) / 2;
    return (size_t)ncls * ((Cout + T - 1) / T) * ((Cin + kCK - 1) / kCK) * 24 * nks * T;
}
size_t dense_packed_floats(int kind, int Cin, int Cout) {
    return dense_fp32_floats(kind, Cin, Cout) + dense_bf9_floats(kind, Cin, Cout);
}

int launch_dense_pack(int kind, int Cin, int Cout, const float* w, const float* scale, float* wp, hipStream_t st,
                      const char** why) {
    if (kind == NCONV_DENSE_3X3) {
        const int T = dense_cout_tile(Cout);
        const int nb = ((Cout + T - 1) / T) * ((Cin + kCK - 1) / kCK) * (T / 8);
        if (T == 32)
            hipLaunchKernelGGL(dense_pack3x3<32>, dim3(nb), dim3(64), 0, st, Cin, Cout, w, scale, wp);
        else
            hipLaunchKernelGGL(dense_pack3x3<64>, dim3(nb), dim3(64), 0, st, Cin, Cout, w, scale, wp);
        return launch_status(why);
    }
    const size_t n = dense_fp32_floats(kind, Cin, Cout);
    size_t blocks = (n + kDT - 1) / kDT;
    if (blocks > 4096) blocks = 4096;
    if (blocks)
        hipLaunchKernelGGL(dense_pack, dim3(blocks), dim3(kDT), 0, st, kind, Cin, Cout, dense_cout_tile(Cout), w,
                           scale, wp);
    if (const size_t rows = dense_bf9_floats(kind, Cin, Cout) / 4) {
        size_t b9 = (rows + kDT - 1) / kDT;
        if (b9 > 4096) b9 = 4096;
        hipLaunchKernelGGL(dense_pack_bf9, dim3(b9), dim3(kDT), 0, st, kind, Cin, Cout, dense_cout_tile(Cout), w,
                           scale, reinterpret_cast<unsigned char*>(wp + n), rows);
    }
    return launch_status(why);
}

}  // namespace nconv
