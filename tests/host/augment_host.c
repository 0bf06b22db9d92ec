/* A non-Python host of nconv_frame_augment, compiled against include/nconv.h and csrc/augment_params.h
 * (the very code the kernel runs) by tests/test_augment_cpu.py: prints what augment_params.h draws for a
 * table of (seed, draw, image, geometry, modes, amplitudes), the layout of struct nconv_frame_augment
 * for the comparison with the ctypes binding, the ABI pair, and the return code and error text of
 * invalid calls that must fail with -EINVAL on the host (no GPU needed; no valid call is made). Plain
 * C99. */
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include <string.h>
#include "nconv.h"
#include "augment_params.h"

#define T nconv_frame_augment_desc
#define F(f) printf("\"nconv_frame_augment.%s\": [%zu, %zu],\n", #f, offsetof(T, f), sizeof(((T*)0)->f))
#define P nconv_augment_plane
#define FP(f) printf("\"nconv_augment_plane.%s\": [%zu, %zu],\n", #f, offsetof(P, f), sizeof(((P*)0)->f))

static unsigned bits(float f) {
    unsigned u;
    memcpy(&u, &f, 4);
    return u;
}

static int first = 1;

static void draw(unsigned long long seed, unsigned dr, int b, int H, int W, int h, int w, int my, int mx,
                 unsigned long long thr, float bri, float con, float col) {
    const uint32_t state[3] = {(uint32_t)seed, (uint32_t)(seed >> 32), dr};
    nconv_augment_draw p;
    nconv_augment_params(state, b, H, W, h, w, my, mx, thr, bri, con, col, &p);
    printf("%s[%llu, %u, %d, %d, %d, %d, %d, %d, %d, %llu, %u, %u, %u, %d, %d, %d, %u, %u, %u, %u, %u]", first ? "" : ",\n",
           seed, dr, b, H, W, h, w, my, mx, thr, bits(bri), bits(con), bits(col), p.y0, p.x0, p.flip, bits(p.g_b),
           bits(p.g_c), bits(p.gain[0]), bits(p.gain[1]), bits(p.gain[2]));
    first = 0;
}

/* a valid B = 2 call, 6 x 16 -> 4 x 8, every tensor present; the pointers are never dereferenced */
static T base(void) {
    T d;
    memset(&d, 0, sizeof d);
    d.B = 2; d.H = 6; d.W = 16; d.h = 4; d.w = 8;
    d.mode_y = NCONV_AUGMENT_RANDOM; d.mode_x = NCONV_AUGMENT_MAX;
    d.flip_threshold = 1ULL << 31;
    d.state = (const unsigned*)0x1000;
    d.rgb = (const float*)0x100000; d.rgb_image_stride = 3 * 96; d.rgb_channel_stride = 96; d.rgb_row_stride = 16;
    d.rgb_out = (float*)0x200000;
    for (int i = 0; i < 3; ++i) {
        d.plane[i].src = (const float*)(size_t)(0x300000 + 0x100000 * i);
        d.plane[i].image_stride = 96; d.plane[i].row_stride = 16;
        d.plane[i].out = (float*)(size_t)(0x600000 + 0x100000 * i);
    }
    d.mask = (const unsigned char*)0x900001; d.mask_image_stride = 96; d.mask_row_stride = 16;
    d.mask_out = (unsigned char*)0xa00003;
    d.k = (const float*)0xb00000; d.k_out = (float*)0xc00000;
    d.params = (int*)0xd00000; d.gains = (float*)0xe00000;
    d.brightness = 0.2f; d.contrast = 0.2f; d.color = 0.2f; d.pivot = 127.5f; d.rgb_max = 255.0f;
    return d;
}

static void call(const char* name, const T* d) {
    const int rc = nconv_frame_augment(d, NULL);
    printf("\"%s\": [%d, \"%s\"],\n", name, rc, nconv_last_error());
}

#define BAD(name, change) do { T d = base(); change; call(name, &d); } while (0)

int main(void) {
    printf("{\n\"draws\": [\n");
    const unsigned long long seeds[3] = {0ULL, 0x9E3779B9C0FFEE01ULL, 0xFFFFFFFFFFFFFFFFULL};
    for (int s = 0; s < 3; ++s)
        for (unsigned dr = 0; dr < 3; ++dr)
            for (int b = 0; b < 4; ++b) {
                const unsigned dw = dr == 2 ? 0xFFFFFFFFu : dr;
                draw(seeds[s], dw, b, 352, 1216, 256, 1216, NCONV_AUGMENT_RANDOM, NCONV_AUGMENT_RANDOM, 1ULL << 31, 0.2f, 0.2f, 0.2f);
                draw(seeds[s], dw, b, 352, 1216, 256, 1024, NCONV_AUGMENT_MAX, NCONV_AUGMENT_RANDOM, 1ULL << 32, 0.f, 0.f, 0.f);
                draw(seeds[s], dw, b, 480, 640, 448, 608, NCONV_AUGMENT_RANDOM, NCONV_AUGMENT_CENTER, 0ULL, 0.4f, 0.f, 0.f);
                draw(seeds[s], dw, b, 7, 13, 5, 9, NCONV_AUGMENT_CENTER, NCONV_AUGMENT_MIN, 1288490188ULL, 0.f, 1.0f, 0.f);
                draw(seeds[s], dw, b, 7, 13, 7, 13, NCONV_AUGMENT_MIN, NCONV_AUGMENT_MAX, 1ULL << 31, 0.f, 0.f, 0.05f);
                draw(seeds[s], dw, b, 65536, 32767, 1, 1, NCONV_AUGMENT_RANDOM, NCONV_AUGMENT_RANDOM, 1ULL << 31, 1.0f, 1.0f, 1.0f);
            }
    printf("\n],\n");

    printf("\"nconv_frame_augment\": [0, %zu],\n", sizeof(T));
    F(B); F(H); F(W); F(h); F(w); F(mode_y); F(mode_x); F(flip_threshold); F(state); F(rgb); F(rgb_image_stride);
    F(rgb_channel_stride); F(rgb_row_stride); F(rgb_out); F(plane); F(mask); F(mask_image_stride); F(mask_row_stride);
    F(mask_out); F(k); F(k_out); F(params); F(gains); F(brightness); F(contrast); F(color); F(pivot); F(rgb_max);
    printf("\"nconv_augment_plane\": [0, %zu],\n", sizeof(P));
    FP(src); FP(image_stride); FP(row_stride); FP(out);
    printf("\"modes\": [%d, %d, %d, %d],\n", NCONV_AUGMENT_RANDOM, NCONV_AUGMENT_CENTER, NCONV_AUGMENT_MIN, NCONV_AUGMENT_MAX);

    call("null_descriptor", NULL);
    BAD("null_state", d.state = NULL);
    BAD("no_source", (d.rgb = NULL, d.rgb_out = NULL, d.mask = NULL, d.mask_out = NULL, d.k = NULL, d.k_out = NULL,
                      memset(d.plane, 0, sizeof d.plane)));
    BAD("rgb_without_out", d.rgb_out = NULL);
    BAD("out_without_rgb", d.rgb = NULL);
    BAD("plane_without_out", d.plane[1].out = NULL);
    BAD("out_without_plane", d.plane[2].src = NULL);
    BAD("mask_without_out", d.mask_out = NULL);
    BAD("out_without_mask", d.mask = NULL);
    BAD("k_without_k_out", d.k_out = NULL);
    BAD("k_out_without_k", d.k = NULL);
    BAD("B_zero", d.B = 0);
    BAD("H_zero", d.H = 0);
    BAD("W_negative", d.W = -1);
    BAD("h_zero", d.h = 0);
    BAD("w_negative", d.w = -3);
    BAD("h_above_H", d.h = 7);
    BAD("w_above_W", d.w = 17);
    BAD("too_large", (d.B = 1 << 12, d.H = 1 << 9, d.W = 1 << 9, d.rgb_row_stride = 1 << 9));
    BAD("rgb_row_stride", d.rgb_row_stride = 15);
    BAD("plane_row_stride", d.plane[0].row_stride = 15);
    BAD("mask_row_stride", d.mask_row_stride = 15);
    BAD("rgb_channel_overlap", d.rgb_channel_stride = 95);
    BAD("rgb_image_overlap", d.rgb_image_stride = 3 * 96 - 1);
    BAD("plane_image_overlap", d.plane[1].image_stride = 95);
    BAD("mask_image_overlap", d.mask_image_stride = 95);
    BAD("mode_y", d.mode_y = 4);
    BAD("mode_x", d.mode_x = -1);
    BAD("flip_threshold", d.flip_threshold = (1ULL << 32) + 1);
    BAD("brightness_negative", d.brightness = -0.1f);
    BAD("contrast_above_one", d.contrast = 1.5f);
    BAD("color_nan", d.color = NAN);
    BAD("pivot_nan", d.pivot = NAN);
    BAD("rgb_max_nan", d.rgb_max = NAN);
    BAD("rgb_max_negative", d.rgb_max = -1.0f);
    BAD("state_misaligned", d.state = (const unsigned*)0x1002);
    BAD("rgb_misaligned", d.rgb = (const float*)0x100002);
    BAD("rgb_out_misaligned", d.rgb_out = (float*)0x200001);
    BAD("plane_misaligned", d.plane[2].src = (const float*)0x500003);
    BAD("plane_out_misaligned", d.plane[0].out = (float*)0x600002);
    BAD("k_misaligned", d.k = (const float*)0xb00002);
    BAD("k_out_misaligned", d.k_out = (float*)0xc00001);
    BAD("params_misaligned", d.params = (int*)0xd00002);
    BAD("gains_misaligned", d.gains = (float*)0xe00002);
    /* an output inside its own source, an output inside another tensor's source, the last byte of one
     * on the first of another, and the small tensors */
    BAD("rgb_out_in_rgb", d.rgb_out = (float*)(0x100000 + 16 * 4));
    BAD("plane_out_in_mask", d.plane[0].out = (float*)(0x900000 + 64));
    BAD("mask_out_on_rgb_end", d.mask_out = (unsigned char*)(0x100000 + (2 * 3 * 96) * 4 - 1));
    BAD("gt_out_before_depth", d.plane[1].out = (float*)(0x300000 - (2 * 4 * 8) * 4 + 4));
    BAD("params_in_k", d.params = (int*)(0xb00000 + 68));
    BAD("k_out_on_state", d.k_out = (float*)(0x1000 + 8));
    BAD("gains_in_plane", d.gains = (float*)(0x500000 + 4 * (96 + 5 * 16 + 12)));

    printf("\"abi\": [%d, %d]\n}\n", nconv_abi_version(), NCONV_ABI_VERSION);
    return 0;
}
