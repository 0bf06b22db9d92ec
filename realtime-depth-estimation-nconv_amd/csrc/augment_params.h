/* augment_params.h — what nconv_frame_augment draws for one image: the crop window, the flip and the
 * jitter gains, from (state, b, geometry, modes, amplitudes), and the jitter of one RGB value. Plain C,
 * and __host__ __device__ under hipcc, so that a host program compiles the very code the kernel runs
 * (tests/host/augment_host.c). include/nconv.h states the rule operation by operation.
 *
 * Every product and sum below is one fp32 rounding: contraction is switched off under clang (hipcc); a C
 * compiler in ISO mode (gcc -std=c99) does not contract across statements either. */
#ifndef NCONV_AUGMENT_PARAMS_H
#define NCONV_AUGMENT_PARAMS_H

#include <stdint.h>
#include "philox.h"

/* enum nconv_augment_crop of include/nconv.h */
#define NCONV_AUGMENT_PARAMS_RANDOM 0
#define NCONV_AUGMENT_PARAMS_CENTER 1
#define NCONV_AUGMENT_PARAMS_MIN 2
#define NCONV_AUGMENT_PARAMS_MAX 3

typedef struct nconv_augment_draw {
    int y0, x0, flip;
    float g_b, g_c, gain[3];
} nconv_augment_draw;

/* the window's first row (column) on an axis of `full` source and `part` output pixels, 1 <= part <= full */
NCONV_PHILOX_FN int nconv_augment_offset(int mode, uint32_t word, int full, int part) {
    switch (mode) {
        case NCONV_AUGMENT_PARAMS_RANDOM: return (int)(uint32_t)(((uint64_t)word * (uint64_t)(full - part + 1)) >> 32);
        case NCONV_AUGMENT_PARAMS_CENTER: return (full - part) / 2;
        case NCONV_AUGMENT_PARAMS_MAX: return full - part;
        default: return 0;
    }
}

/* 1 + amp * s(x), s(x) = 2 u(x) - 1 and u(x) = (float)(x >> 8) * 2^-24 (both exact): a multiply, an add */
NCONV_PHILOX_FN float nconv_augment_gain(float amp, uint32_t x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const float u = (float)(x >> 8) * 0x1p-24f;
    const float s = 2.0f * u - 1.0f;
    const float t = amp * s;
    return 1.0f + t;
}

/* state = {seed_lo, seed_hi, draw}; jitter: any amplitude is non-zero (else the gains are 1) */
NCONV_PHILOX_FN void nconv_augment_params(const uint32_t* state, int b, int H, int W, int h, int w, int mode_y,
                                          int mode_x, uint64_t flip_threshold, float brightness, float contrast,
                                          float color, nconv_augment_draw* p) {
    const uint32_t key[2] = {state[0], state[1]};
    const uint32_t c0[4] = {(uint32_t)b, 0u, state[2], 1u}, c1[4] = {(uint32_t)b, 1u, state[2], 1u};
    uint32_t wd[4], jt[4];
    nconv_philox4x32_10(c0, key, wd);
    nconv_philox4x32_10(c1, key, jt);
    p->y0 = nconv_augment_offset(mode_y, wd[0], H, h);
    p->x0 = nconv_augment_offset(mode_x, wd[1], W, w);
    p->flip = (uint64_t)wd[2] < flip_threshold;
    if (brightness == 0.0f && contrast == 0.0f && color == 0.0f) {
        p->g_b = p->g_c = p->gain[0] = p->gain[1] = p->gain[2] = 1.0f;
    } else {
        p->g_b = nconv_augment_gain(brightness, jt[0]);
        p->g_c = nconv_augment_gain(contrast, jt[1]);
        p->gain[0] = nconv_augment_gain(color, wd[3]);
        p->gain[1] = nconv_augment_gain(color, jt[2]);
        p->gain[2] = nconv_augment_gain(color, jt[3]);
    }
}

/* one RGB value under the jitter: five roundings, then the clamp to [0, rgb_max] by comparisons (-0.0
 * comes out as +0.0, as does a NaN) */
NCONV_PHILOX_FN float nconv_augment_jitter(float v, float g_b, float gain, float g_c, float pivot, float rgb_max) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    float a = v * g_b;
    a = a * gain;
    a = a - pivot;
    a = a * g_c;
    a = a + pivot;
    a = a > 0.0f ? a : 0.0f;
    return a < rgb_max ? a : rgb_max;
}

#endif /* NCONV_AUGMENT_PARAMS_H */
