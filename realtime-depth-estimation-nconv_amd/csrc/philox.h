/* philox.h — Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11), the
 * counter-based generator behind nconv_depth_sparsify. Plain C, and __host__ __device__ under hipcc, so
 * that a host program compiles the very code the kernel runs (tests/host/sparsify_host.c).
 *
 * One round maps the counter (c0, c1, c2, c3) under the key (k0, k1) to
 *   (hi(M1 * c2) ^ c1 ^ k0,  lo(M1 * c2),  hi(M0 * c0) ^ c3 ^ k1,  lo(M0 * c0))
 * with hi / lo the halves of the 64-bit product, and then bumps the key by (W0, W1). Ten rounds.
 * Known answers (Random123's kat_vectors): zeros -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8; all ones ->
 * 408f276d 41c83b0e a20bc7c6 6d5451fd. */
#ifndef NCONV_PHILOX_H
#define NCONV_PHILOX_H

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NCONV_PHILOX_FN __host__ __device__ static inline
#else
#define NCONV_PHILOX_FN static inline
#endif

#define NCONV_PHILOX_M0 0xD2511F53u
#define NCONV_PHILOX_M1 0xCD9E8D57u
#define NCONV_PHILOX_W0 0x9E3779B9u
#define NCONV_PHILOX_W1 0xBB67AE85u

NCONV_PHILOX_FN void nconv_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
    int r;
    for (r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)NCONV_PHILOX_M0 * c0, p1 = (uint64_t)NCONV_PHILOX_M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1, c3 = (uint32_t)p0, c0 = n0, c2 = n2;
        k0 += NCONV_PHILOX_W0, k1 += NCONV_PHILOX_W1;
    }
    out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

#endif /* NCONV_PHILOX_H */
