// ssim_common.h — the 3 x 3 window pieces of the structural photometric term, shared by photo_ssim.hip (one
// source) and photo_min.hip (the minimum over several sources): the regions a 16 x 64 tile stages with its
// halo, the staging of one region pixel, the window test, SSIM of a window and the three coefficients of its
// derivative. The rule is stated operation by operation in include/nconv.h (nconv_photo_ssim_loss_*); every
// operation here is fp32 in that order, no contraction.
#pragma once
#include "warp_common.h"

namespace nconv {

constexpr int kFH = kLossTH + 2, kFW = kLossTW + 2;      // the forward's region: the tile and a one-pixel halo
constexpr int kFN = kFH * kFW;
constexpr int kGH = kLossTH + 4, kGW = kLossTW + 4;      // the backward's region: a two-pixel halo
constexpr int kGN = kGH * kGW;

// x, y (every channel) and validity of region pixel idx of an RH x RW region whose corner is (i0, j0)
template <int C, int RW, int RN>
__device__ __forceinline__ void stage_pixel(const WarpArgs& a, const Camera& cam, const Proj& q, int b, int i0,
                                            int j0, int idx, float (&sx)[C][RN], float (&sy)[C][RN],
                                            unsigned char (&sv)[RN]) {
    const int i = i0 + idx / RW, j = j0 + idx % RW;
    const bool inside = i >= 0 && i < a.H && j >= 0 && j < a.W;
    const Geo g = warp_geometry(a, cam, q, b, i, j, inside);
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        sx[ch][idx] = warp_sample(a, g, b, ch).s;
        sy[ch][idx] = tgt_load(a, b, ch, i, j, g.ok);
    }
    sv[idx] = g.ok ? 1 : 0;
}

// all nine pixels of the window centred at o are valid
template <int RW>
__device__ __forceinline__ bool window_valid(const unsigned char* sv, int o) {
    bool w = true;
#pragma unroll
    for (int di = -1; di <= 1; ++di)
#pragma unroll
        for (int dj = -1; dj <= 1; ++dj) w = w && sv[o + di * RW + dj] != 0;
    return w;
}

// SSIM of the window centred at o
struct Ssim {
    float mux, muy, A1, A2, B1, B2, den, ssim, t;
};
template <int RW>
__device__ __forceinline__ Ssim ssim_window(const float* x, const float* y, int o, float c1, float c2) {
#pragma clang fp contract(off)
    float Sx = 0.f, Sy = 0.f, Sxx = 0.f, Syy = 0.f, Sxy = 0.f;
#pragma unroll
    for (int di = -1; di <= 1; ++di) {
#pragma unroll
        for (int dj = -1; dj <= 1; ++dj) {
            const float xv = x[o + di * RW + dj], yv = y[o + di * RW + dj];
            const float xx = xv * xv, yy = yv * yv, xy = xv * yv;
            const bool first = di == -1 && dj == -1;
            Sx = first ? xv : Sx + xv, Sy = first ? yv : Sy + yv;
            Sxx = first ? xx : Sxx + xx, Syy = first ? yy : Syy + yy, Sxy = first ? xy : Sxy + xy;
        }
    }
    Ssim s;
    s.mux = Sx / 9.0f, s.muy = Sy / 9.0f;
    const float mxx = s.mux * s.mux, myy = s.muy * s.muy, mxy = s.mux * s.muy;
    const float exx = Sxx / 9.0f, eyy = Syy / 9.0f, exy = Sxy / 9.0f;
    const float vx = exx - mxx, vy = eyy - myy, vxy = exy - mxy;
    const float m2 = 2.0f * mxy, v2 = 2.0f * vxy;
    s.A1 = m2 + c1, s.A2 = v2 + c2;
    const float ms = mxx + myy, vs = vx + vy;
    s.B1 = ms + c1, s.B2 = vs + c2;
    const float num = s.A1 * s.A2;
    s.den = s.B1 * s.B2;
    s.ssim = num / s.den;
    const float d = 1.0f - s.ssim;
    s.t = d * 0.5f;
    return s;
}

// the term of a window: clamp(t, 0, 1), a NaN stays
__device__ __forceinline__ float ssim_term(const Ssim& s) { return s.t < 0.f ? 0.f : s.t > 1.f ? 1.f : s.t; }

// d ssim_p / d x_q = a + b x_q + c y_q for a pixel q of the window p
struct SsimCoef {
    float a, b, c;
};
__device__ __forceinline__ SsimCoef ssim_coef(const Ssim& s) {
#pragma clang fp contract(off)
    const float c_n = 2.0f * s.A1, d9 = 9.0f * s.den;
    const float cp = c_n / d9;
    const float b_n = 2.0f * s.ssim, b_d = 9.0f * s.B2;
    const float bq = b_n / b_d;
    const float sm = s.ssim * s.mux;
    const float dA = s.A2 - s.A1;
    const float p1n = s.muy * dA;
    const float p1 = p1n / s.den, p2 = sm / s.B1, p3 = sm / s.B2;
    const float p12 = p1 - p2;
    const float p123 = p12 + p3;
    const float a2 = 2.0f * p123;
    const float ap = a2 / 9.0f;
    return SsimCoef{ap, -bq, cp};
}

}  // namespace nconv
