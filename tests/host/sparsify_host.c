/* A non-Python host of nconv_depth_sparsify, compiled against include/nconv.h and csrc/philox.h (the very
 * code the kernels run) by tests/test_sparsify_cpu.py: prints the Philox known answers, the layout of
 * struct nconv_depth_sparsify for the comparison with the ctypes binding and the ABI pair, then makes
 * invalid calls that must fail with -EINVAL on the host (no GPU needed). Plain C99. */
#include <stddef.h>
#include <stdio.h>
#include "nconv.h"
#include "philox.h"

#define T nconv_depth_sparsify_desc
#define F(f) printf("\"nconv_depth_sparsify.%s\": [%zu, %zu],\n", #f, offsetof(T, f), sizeof(((T*)0)->f))

static void kat(const char* name, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    const uint32_t ctr[4] = {c0, c1, c2, c3}, key[2] = {k0, k1};
    uint32_t w[4];
    nconv_philox4x32_10(ctr, key, w);
    printf("\"%s\": \"%08x %08x %08x %08x\",\n", name, (unsigned)w[0], (unsigned)w[1], (unsigned)w[2], (unsigned)w[3]);
}

int main(void) {
    printf("{\n");
    kat("kat_zeros", 0u, 0u, 0u, 0u, 0u, 0u);
    kat("kat_ones", 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu);
    kat("kat_pi", 0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u);

    printf("\"nconv_depth_sparsify\": [0, %zu],\n", sizeof(T));
    F(B); F(H); F(W); F(mode); F(src); F(src_image_stride); F(src_row_stride); F(mask); F(mask_image_stride);
    F(mask_row_stride); F(state); F(n_dev); F(n); F(keep); F(all_pixels); F(floor); F(key_mask);
    F(noise_threshold); F(noise_amp);

    /* one NYU-sized frame; the pointers are never dereferenced */
    struct nconv_depth_sparsify d = {0};
    d.B = 1; d.H = 480; d.W = 640; d.mode = NCONV_SPARSIFY_COUNT; d.n = 500;
    d.src = (const float*)0x100000; d.src_row_stride = 640; d.state = (const unsigned*)0x1000;
    d.key_mask = 0xffffffffu;
    float* dst = (float*)0x800000;
    void* ws = (void*)0x2000;
    const size_t need = nconv_depth_sparsify_workspace_bytes(1, 480, 640);
    printf("\"workspace_bytes\": [%zu, %zu],\n", need, nconv_depth_sparsify_workspace_bytes(0, 480, 640));
    int rc = nconv_depth_sparsify(&d, dst, 0, 640, NULL, ws, need - 1, NULL);
    printf("\"rc_workspace\": [%d, \"%s\"],\n", rc, nconv_last_error());
    rc = nconv_depth_sparsify(&d, dst, 0, 639, NULL, ws, need, NULL);
    printf("\"rc_row_stride\": [%d, \"%s\"],\n", rc, nconv_last_error());
    d.state = NULL;
    rc = nconv_depth_sparsify(&d, dst, 0, 640, NULL, ws, need, NULL);
    printf("\"rc_state\": [%d, \"%s\"],\n", rc, nconv_last_error());
    d.state = (const unsigned*)0x1000;
    d.mode = 7;
    rc = nconv_depth_sparsify(&d, dst, 0, 640, NULL, ws, need, NULL);
    printf("\"rc_mode\": [%d, \"%s\"],\n", rc, nconv_last_error());
    d.mode = NCONV_SPARSIFY_COUNT;
    /* one row into src: neither src itself nor clear of it */
    rc = nconv_depth_sparsify(&d, (float*)(0x100000 + 640 * 4), 0, 640, NULL, ws, need, NULL);
    printf("\"rc_overlap\": [%d, \"%s\"],\n", rc, nconv_last_error());
    /* a batch of two: image strides one element short, a short mask row, a stride above 2^40 */
    const long long plane = 480LL * 640;
    const size_t need2 = nconv_depth_sparsify_workspace_bytes(2, 480, 640);
    d.B = 2; d.src_image_stride = plane;
    rc = nconv_depth_sparsify(&d, dst, plane - 1, 640, NULL, ws, need2, NULL);
    printf("\"rc_dst_image_stride\": [%d, \"%s\"],\n", rc, nconv_last_error());
    d.mask = (const unsigned char*)0x4000000; d.mask_row_stride = 639;
    rc = nconv_depth_sparsify(&d, dst, plane, 640, NULL, ws, need2, NULL);
    printf("\"rc_mask_row_stride\": [%d, \"%s\"],\n", rc, nconv_last_error());
    d.mask_row_stride = 640; d.mask_image_stride = plane - 1;
    rc = nconv_depth_sparsify(&d, dst, plane, 640, NULL, ws, need2, NULL);
    printf("\"rc_mask_image_stride\": [%d, \"%s\"],\n", rc, nconv_last_error());
    d.mask = NULL;
    rc = nconv_depth_sparsify(&d, dst, (1LL << 41) * 480, (1LL << 40) + 1, NULL, ws, need2, NULL);
    printf("\"rc_stride_cap\": [%d, \"%s\"],\n", rc, nconv_last_error());
    printf("\"abi\": [%d, %d]\n}\n", nconv_abi_version(), NCONV_ABI_VERSION);
    return 0;
}
