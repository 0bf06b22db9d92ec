/* A non-Python host of the minimum-reprojection entry points, compiled against include/nconv.h by
 * tests/test_minreproj_cpu.py: prints the workspace sizes and makes every invalid call the header lists, each of
 * which must fail with -EINVAL on the host (no GPU needed; the pointers are never dereferenced). Plain C99. */
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include "nconv.h"

static const float* const DEPTH = (const float*)0x100000;
static const unsigned char* const MASK = (const unsigned char*)0x200000;
static const float* const SRC0 = (const float*)0x300000;
static const float* const SRC1 = (const float*)0x380000;
static const float* const K_ = (const float*)0x400000;
static const float* const M0 = (const float*)0x500000;
static const float* const M1 = (const float*)0x580000;
static const float* const TGT = (const float*)0x600000;
static float* const OUT = (float*)0x700000;
static unsigned char* const WINNER = (unsigned char*)0x780000;
static float* const ERROR_ = (float*)0x800000;
static void* const WS = (void*)0x900000;
static float* const LOSS = (float*)0xa00000;

typedef struct {
    struct nconv_view_warp d[4];
    int S, automask;
    const float* tgt;
    long long tbs, tcs, trs;
    float alpha, c1, c2;
    float *g_depth, *loss;
    void* ws;
    size_t ws_bytes;
} A;

/* two sources; B = 2, C = 3, a 4 x 8 target cropped out of 5 x 10 planes, 6 x 9 sources, no auto-masking */
static A good(void) {
    A a;
    struct nconv_view_warp d = {2, 3, 4, 8, 6, 9, DEPTH, 50, 10, MASK, 32, 8, SRC0, 162, 54, 9, K_, 9, M0, 12, 0.0f, 0.0f};
    a.d[0] = a.d[1] = a.d[2] = a.d[3] = d;
    a.d[1].src = SRC1, a.d[1].m = M1;
    a.S = 2, a.automask = 0;
    a.tgt = TGT, a.tbs = 96, a.tcs = 32, a.trs = 8;
    a.alpha = 0.85f, a.c1 = 6.5025f, a.c2 = 58.5225f;
    a.g_depth = OUT, a.loss = LOSS;
    a.ws = WS, a.ws_bytes = nconv_photo_min_workspace_bytes(2, 4, 8);
    return a;
}

/* the same with sources of the target's size, as auto-masking needs */
static A good_automask(void) {
    A a = good();
    int s;
    for (s = 0; s < 4; ++s) a.d[s].Hs = 4, a.d[s].Ws = 8, a.d[s].src_row_stride = 8, a.d[s].src_channel_stride = 32,
                            a.d[s].src_image_stride = 96;
    a.automask = 1;
    return a;
}

static void report(const char* side, const char* name, int rc) {
    printf("\"%s_%s\": [%d, \"%s\"],\n", side, name, rc, rc ? nconv_last_error() : "");
}

/* Every call here must be refused by the host checks: an accepted one would launch on these made-up pointers. */
static void call(const char* name, const A* a) {
    report("fwd", name, nconv_photo_min_loss_fwd(a->d, a->S, a->tgt, a->tbs, a->tcs, a->trs, a->alpha, a->c1, a->c2,
                                                 a->automask, a->loss, WINNER, ERROR_, a->ws, a->ws_bytes, NULL));
    report("bwd", name, nconv_photo_min_loss_bwd(a->d, a->S, a->tgt, a->tbs, a->tcs, a->trs, a->alpha, a->c1, a->c2,
                                                 a->automask, NULL, a->ws, a->ws_bytes, a->g_depth, NULL));
}

#define BAD(name, defect) do { A a = good(); defect; call(name, &a); } while (0)
/* a defect of one view, made in view 0 and in view 1 in turn: "v0_<name>", "v1_<name>" */
#define BADV(name, defect) do { int v; for (v = 0; v < 2; ++v) { A a = good(); struct nconv_view_warp* d = &a.d[v]; \
    defect; call(v ? "v1_" name : "v0_" name, &a); } } while (0)

int main(void) {
    printf("{\n\"ws\": [%zu, %zu, %zu, %zu, %zu],\n", nconv_photo_min_workspace_bytes(2, 4, 8),
           nconv_photo_min_workspace_bytes(8, 352, 1216), nconv_photo_min_workspace_bytes(0, 4, 8),
           nconv_photo_min_workspace_bytes(1, 4, -1), nconv_photo_min_workspace_bytes(3, 17, 65));
    { A a = good(); report("fwd", "null_descriptor", nconv_photo_min_loss_fwd(NULL, 2, TGT, 96, 32, 8, 0.85f, 6.5f, 58.5f,
                                                                         0, LOSS, NULL, NULL, WS, a.ws_bytes, NULL));
      report("bwd", "null_descriptor", nconv_photo_min_loss_bwd(NULL, 2, TGT, 96, 32, 8, 0.85f, 6.5f, 58.5f, 0, NULL, WS,
                                                                a.ws_bytes, OUT, NULL)); }
    /* everything the single-source entry points refuse, for each view */
    BADV("null_depth", d->depth = NULL);
    BADV("null_src", d->src = NULL);
    BADV("null_k", d->k = NULL);
    BADV("null_m", d->m = NULL);
    BADV("C_2", d->C = 2);
    BADV("C_0", d->C = 0);
    BADV("C_4", d->C = 4);
    BADV("B_zero", d->B = 0);
    BADV("H_negative", d->H = -1);
    BADV("Ws_zero", d->Ws = 0);
    BADV("W_above_2_24", (d->W = (1 << 24) + 1, d->B = 1, d->C = 1, d->H = 1, d->depth_row_stride = 1 << 25));
    BADV("batch_too_large", (d->B = 1 << 20, d->H = 64, d->W = 64, d->depth_row_stride = 64,
                             d->depth_image_stride = 4096));
    BADV("k_stride_negative", d->k_image_stride = -9);
    BADV("m_stride_negative", d->m_image_stride = -12);
    BADV("z_min_negative", d->z_min = -1.0f);
    BADV("z_min_nan", d->z_min = NAN);
    BADV("z_max_below_z_min", (d->z_min = 2.0f, d->z_max = 1.0f));
    BADV("z_max_nan", d->z_max = NAN);
    BADV("depth_misaligned", d->depth = (const float*)0x100002);
    BADV("depth_row_stride_short", d->depth_row_stride = 7);
    BADV("depth_row_stride_negative", d->depth_row_stride = -10);
    BADV("depth_image_stride_short", d->depth_image_stride = 39);
    BADV("mask_row_stride_short", d->mask_row_stride = 7);
    BADV("mask_image_stride_short", d->mask_image_stride = 31);
    BADV("src_row_stride_short", d->src_row_stride = 8);
    BADV("src_channel_stride_short", d->src_channel_stride = 53);
    BADV("src_image_stride_short", d->src_image_stride = 161);
    BADV("src_stride_negative", d->src_image_stride = -162);
    BADV("src_plane_too_large", (d->src_row_stride = ((1LL << 29) - 9) / 5 + 1, d->src_channel_stride = 1LL << 32,
                                 d->src_image_stride = 1LL << 34));
    /* the operands all views share */
    BAD("null_tgt", a.tgt = NULL);
    BAD("tgt_row_stride_short", a.trs = 7);
    BAD("tgt_channel_stride_short", a.tcs = 31);
    BAD("workspace_small", a.ws_bytes -= 1);
    BAD("workspace_ssim_sized", a.ws_bytes = nconv_photo_ssim_workspace_bytes(2, 4, 8));
    BAD("workspace_null", a.ws = NULL);
    BAD("workspace_misaligned", a.ws = (void*)0x900004);
    { A a = good(); a.loss = NULL; a.g_depth = NULL; call("null_output", &a); }
    BAD("alpha_negative", a.alpha = -0.01f);
    BAD("alpha_above_one", a.alpha = 1.5f);
    BAD("alpha_nan", a.alpha = NAN);
    BAD("c1_zero", a.c1 = 0.0f);
    BAD("c1_nan", a.c1 = NAN);
    BAD("c2_negative", a.c2 = -1.0f);
    BAD("c2_infinite", a.c2 = INFINITY);
    /* the number of sources */
    BAD("S_zero", a.S = 0);
    BAD("S_negative", a.S = -1);
    BAD("S_five", a.S = 5);
    /* views that disagree in what they must share (each view valid on its own) */
    BAD("differ_B", (a.d[1].B = 1));
    BAD("differ_C", (a.d[1].C = 1));
    BAD("differ_H", (a.d[1].H = 3));
    BAD("differ_W", (a.d[1].W = 7));
    BAD("differ_depth", (a.d[1].depth = DEPTH + 1));
    BAD("differ_depth_row_stride", (a.d[1].depth_row_stride = 11));
    BAD("differ_depth_image_stride", (a.d[1].depth_image_stride = 60));
    BAD("differ_mask", (a.d[1].mask = NULL));
    BAD("differ_mask_strides", (a.d[1].mask_row_stride = 9, a.d[1].mask_image_stride = 40));
    BAD("differ_k", (a.d[1].k = K_ + 9));
    BAD("differ_k_stride", (a.d[1].k_image_stride = 0));
    BAD("differ_z_min", (a.d[1].z_min = 1.0f));
    BAD("differ_z_max", (a.d[1].z_max = 5.0f));
    BAD("differ_in_third_view", (a.S = 3, a.d[2].z_max = 5.0f));
    /* auto-masking */
    BAD("automask_other_size", a.automask = 1);
    BAD("automask_two", a.automask = 2);
    { A a = good_automask(); a.d[1].Ws = 9, a.d[1].src_row_stride = 9, a.d[1].src_channel_stride = 36,
      a.d[1].src_image_stride = 108; call("automask_one_other_size", &a); }
    /* the good descriptors pass every check but the one made wrong here: a workspace one byte short */
    { A a = good_automask(); a.ws_bytes -= 1; call("automask_good_but_workspace", &a); }
    printf("\"abi\": [%d, %d]\n}\n", nconv_abi_version(), NCONV_ABI_VERSION);
    return 0;
}
