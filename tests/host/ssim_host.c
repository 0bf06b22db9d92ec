/* A non-Python host of the SSIM photometric-loss entry points, compiled against include/nconv.h by
 * tests/test_ssim_cpu.py: prints the workspace sizes and makes every invalid call the header lists, each of
 * which must fail with -EINVAL on the host (no GPU needed; the pointers are never dereferenced). Plain C99. */
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include "nconv.h"

static const float* const DEPTH = (const float*)0x100000;
static const unsigned char* const MASK = (const unsigned char*)0x200000;
static const float* const SRC = (const float*)0x300000;
static const float* const K_ = (const float*)0x400000;
static const float* const M_ = (const float*)0x500000;
static const float* const TGT = (const float*)0x600000;
static float* const OUT = (float*)0x700000;
static void* const WS = (void*)0x900000;
static float* const LOSS = (float*)0xa00000;

typedef struct {
    struct nconv_view_warp d;
    const float* tgt;
    long long tbs, tcs, trs;
    float alpha, c1, c2;
    float *g_depth, *loss;
    void* ws;
    size_t ws_bytes;
} A;

/* B = 2, C = 3, a 4 x 8 target cropped out of 5 x 10 planes, a 6 x 9 source */
static A good(void) {
    A a;
    struct nconv_view_warp d = {2, 3, 4, 8, 6, 9, DEPTH, 50, 10, MASK, 32, 8, SRC, 162, 54, 9, K_, 9, M_, 12, 0.0f, 0.0f};
    a.d = d;
    a.tgt = TGT, a.tbs = 96, a.tcs = 32, a.trs = 8;
    a.alpha = 0.85f, a.c1 = 6.5025f, a.c2 = 58.5225f;
    a.g_depth = OUT, a.loss = LOSS;
    a.ws = WS, a.ws_bytes = nconv_photo_ssim_workspace_bytes(2, 4, 8);
    return a;
}

static void report(const char* side, const char* name, int rc) {
    printf("\"%s_%s\": [%d, \"%s\"],\n", side, name, rc, rc ? nconv_last_error() : "");
}

/* Every call here must be refused by the host checks: an accepted one would launch on these made-up pointers. */
static void call(const char* name, const A* a) {
    report("fwd", name, nconv_photo_ssim_loss_fwd(&a->d, a->tgt, a->tbs, a->tcs, a->trs, a->alpha, a->c1, a->c2,
                                                  a->loss, a->ws, a->ws_bytes, NULL));
    report("bwd", name, nconv_photo_ssim_loss_bwd(&a->d, a->tgt, a->tbs, a->tcs, a->trs, a->alpha, a->c1, a->c2, NULL,
                                                  a->ws, a->ws_bytes, a->g_depth, NULL));
}

#define BAD(name, defect) do { A a = good(); defect; call(name, &a); } while (0)

int main(void) {
    printf("{\n\"ws\": [%zu, %zu, %zu, %zu, %zu],\n", nconv_photo_ssim_workspace_bytes(2, 4, 8),
           nconv_photo_ssim_workspace_bytes(8, 352, 1216), nconv_photo_ssim_workspace_bytes(0, 4, 8),
           nconv_photo_ssim_workspace_bytes(1, 4, -1), nconv_photo_ssim_workspace_bytes(3, 17, 65));
    report("fwd", "null_descriptor",
           nconv_photo_ssim_loss_fwd(NULL, TGT, 96, 32, 8, 0.85f, 6.5f, 58.5f, LOSS, WS, 1 << 20, NULL));
    report("bwd", "null_descriptor",
           nconv_photo_ssim_loss_bwd(NULL, TGT, 96, 32, 8, 0.85f, 6.5f, 58.5f, NULL, WS, 1 << 20, OUT, NULL));
    /* everything the photometric entry points refuse */
    BAD("null_depth", a.d.depth = NULL);
    BAD("null_src", a.d.src = NULL);
    BAD("null_k", a.d.k = NULL);
    BAD("null_m", a.d.m = NULL);
    BAD("C_2", a.d.C = 2);
    BAD("C_0", a.d.C = 0);
    BAD("C_4", a.d.C = 4);
    BAD("B_zero", a.d.B = 0);
    BAD("H_negative", a.d.H = -1);
    BAD("Ws_zero", a.d.Ws = 0);
    BAD("W_above_2_24", (a.d.W = (1 << 24) + 1, a.d.B = 1, a.d.C = 1, a.d.H = 1, a.d.depth_row_stride = 1 << 25));
    BAD("batch_too_large", (a.d.B = 1 << 20, a.d.H = 64, a.d.W = 64, a.d.depth_row_stride = 64,
                            a.d.depth_image_stride = 4096));
    BAD("k_stride_negative", a.d.k_image_stride = -9);
    BAD("m_stride_negative", a.d.m_image_stride = -12);
    BAD("z_min_negative", a.d.z_min = -1.0f);
    BAD("z_min_nan", a.d.z_min = NAN);
    BAD("z_max_below_z_min", (a.d.z_min = 2.0f, a.d.z_max = 1.0f));
    BAD("z_max_nan", a.d.z_max = NAN);
    BAD("depth_misaligned", a.d.depth = (const float*)0x100002);
    BAD("depth_row_stride_short", a.d.depth_row_stride = 7);
    BAD("depth_row_stride_negative", a.d.depth_row_stride = -10);
    BAD("depth_image_stride_short", a.d.depth_image_stride = 39);
    BAD("mask_row_stride_short", a.d.mask_row_stride = 7);
    BAD("mask_image_stride_short", a.d.mask_image_stride = 31);
    BAD("src_row_stride_short", a.d.src_row_stride = 8);
    BAD("src_channel_stride_short", a.d.src_channel_stride = 53);
    BAD("src_image_stride_short", a.d.src_image_stride = 161);
    BAD("src_stride_negative", a.d.src_image_stride = -162);
    BAD("depth_plane_too_large", (a.d.B = 1, a.d.depth_row_stride = ((1LL << 29) - 8) / 3 + 1));
    BAD("src_plane_too_large", (a.d.B = 1, a.d.C = 1, a.d.src_row_stride = ((1LL << 29) - 9) / 5 + 1));
    BAD("mask_plane_too_large", (a.d.B = 1, a.d.mask_row_stride = ((1LL << 31) - 8) / 3 + 1));
    BAD("null_tgt", a.tgt = NULL);
    BAD("tgt_row_stride_short", a.trs = 7);
    BAD("tgt_channel_stride_short", a.tcs = 31);
    BAD("tgt_plane_too_large", (a.d.B = 1, a.d.C = 1, a.trs = ((1LL << 29) - 8) / 3 + 1));
    BAD("workspace_small", a.ws_bytes -= 1);
    BAD("workspace_null", a.ws = NULL);
    BAD("workspace_misaligned", a.ws = (void*)0x900004);
    { A a = good(); a.loss = NULL; a.g_depth = NULL; call("null_output", &a); }
    /* the SSIM term's own operands */
    BAD("alpha_negative", a.alpha = -0.01f);
    BAD("alpha_above_one", a.alpha = 1.5f);
    BAD("alpha_nan", a.alpha = NAN);
    BAD("c1_zero", a.c1 = 0.0f);
    BAD("c1_negative", a.c1 = -1.0f);
    BAD("c1_nan", a.c1 = NAN);
    BAD("c1_infinite", a.c1 = INFINITY);
    BAD("c2_zero", a.c2 = 0.0f);
    BAD("c2_nan", a.c2 = NAN);
    BAD("c2_infinite", a.c2 = INFINITY);
    printf("\"abi\": [%d, %d]\n}\n", nconv_abi_version(), NCONV_ABI_VERSION);
    return 0;
}
