/* A non-Python host of the cross-view consistency entry points, compiled against include/nconv.h by
 * tests/test_consistency_cpu.py: prints the workspace sizes and makes every invalid call the header lists, each of
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
static const float* const KS = (const float*)0x480000;
static const float* const M0 = (const float*)0x500000;
static const float* const M1 = (const float*)0x580000;
static const float* const MB0 = (const float*)0x600000;
static const float* const MB1 = (const float*)0x680000;
static float* const FUSED = (float*)0x700000;
static unsigned char* const COUNT = (unsigned char*)0x780000;
static float* const G_DEPTH = (float*)0x800000;
static void* const WS = (void*)0x900000;
static float* const LOSS = (float*)0xa00000;

typedef struct {
    struct nconv_view_warp d[4];
    struct nconv_consistency_source e[4];
    int S, min_views;
    float px_tol, rel_tol;
    float *fused, *g_depth, *loss;
    unsigned char* count;
    void* ws;
    size_t ws_bytes;
} A;

/* two sources; B = 2, a 4 x 8 target cropped out of 5 x 10 planes, 6 x 9 source depth planes */
static A good(void) {
    A a;
    struct nconv_view_warp d = {2, 1, 4, 8, 6, 9, DEPTH, 50, 10, MASK, 32, 8, SRC0, 54, 54, 9, K_, 9, M0, 12, 0.001f, 0.0f};
    struct nconv_consistency_source e = {KS, 9, MB0, 12};
    a.d[0] = a.d[1] = a.d[2] = a.d[3] = d;
    a.e[0] = a.e[1] = a.e[2] = a.e[3] = e;
    a.d[1].src = SRC1, a.d[1].m = M1, a.e[1].m_back = MB1;
    a.S = 2, a.min_views = 1, a.px_tol = 1.0f, a.rel_tol = 0.01f;
    a.fused = FUSED, a.count = COUNT, a.g_depth = G_DEPTH, a.loss = LOSS;
    a.ws = WS, a.ws_bytes = nconv_geo_consistency_workspace_bytes(2, 4, 8);
    return a;
}

static void report(const char* side, const char* name, int rc) {
    printf("\"%s_%s\": [%d, \"%s\"],\n", side, name, rc, rc ? nconv_last_error() : "");
}

/* Every call here must be refused by the host checks: an accepted one would launch on these made-up pointers. */
static void call_check(const char* name, const A* a) {
    report("check", name, nconv_depth_consistency(a->d, a->e, a->S, a->px_tol, a->rel_tol, a->min_views, a->fused,
                                                  a->count, NULL, NULL, NULL, NULL));
}
/* the loss takes one view: view v of the set */
static void call_loss(const char* name, const A* a, int v) {
    report("fwd", name, nconv_geo_consistency_loss_fwd(&a->d[v], a->loss, NULL, a->ws, a->ws_bytes, NULL));
    report("bwd", name, nconv_geo_consistency_loss_bwd(&a->d[v], NULL, a->ws, a->ws_bytes, a->g_depth, NULL));
}

#define BADC(name, defect) do { A a = good(); defect; call_check(name, &a); } while (0)
#define BADL(name, defect) do { A a = good(); defect; call_loss(name, &a, 0); } while (0)
/* a defect of one view, made in view 0 and in view 1 in turn: "v0_<name>", "v1_<name>"; the loss is given that view */
#define BADV(name, defect) do { int v; for (v = 0; v < 2; ++v) { A a = good(); struct nconv_view_warp* d = &a.d[v]; \
    struct nconv_consistency_source* e = &a.e[v]; (void)d; (void)e; defect; \
    call_check(v ? "v1_" name : "v0_" name, &a); call_loss(v ? "v1_" name : "v0_" name, &a, v); } } while (0)
/* the same for what only the check reads */
#define BADE(name, defect) do { int v; for (v = 0; v < 2; ++v) { A a = good(); \
    struct nconv_consistency_source* e = &a.e[v]; defect; call_check(v ? "v1_" name : "v0_" name, &a); } } while (0)

int main(void) {
    printf("{\n\"ws\": [%zu, %zu, %zu, %zu, %zu, %zu],\n", nconv_geo_consistency_workspace_bytes(2, 4, 8),
           nconv_geo_consistency_workspace_bytes(8, 352, 1216), nconv_geo_consistency_workspace_bytes(0, 4, 8),
           nconv_geo_consistency_workspace_bytes(1, 4, -1), nconv_geo_consistency_workspace_bytes(3, 17, 65),
           nconv_photo_loss_workspace_bytes(3, 17, 65));
    { A a = good();
      report("check", "null_views", nconv_depth_consistency(NULL, a.e, 2, 1.0f, 0.01f, 1, FUSED, COUNT, NULL, NULL, NULL, NULL));
      report("check", "null_sources", nconv_depth_consistency(a.d, NULL, 2, 1.0f, 0.01f, 1, FUSED, COUNT, NULL, NULL, NULL, NULL));
      report("fwd", "null_descriptor", nconv_geo_consistency_loss_fwd(NULL, LOSS, NULL, WS, a.ws_bytes, NULL));
      report("bwd", "null_descriptor", nconv_geo_consistency_loss_bwd(NULL, NULL, WS, a.ws_bytes, G_DEPTH, NULL)); }
    /* everything the view warp's entry points refuse, for each view */
    BADV("null_depth", d->depth = NULL);
    BADV("null_src", d->src = NULL);
    BADV("null_k", d->k = NULL);
    BADV("null_m", d->m = NULL);
    BADV("C_3", (d->C = 3, d->src_channel_stride = 54, d->src_image_stride = 162));
    BADV("C_2", d->C = 2);
    BADV("C_0", d->C = 0);
    BADV("B_zero", d->B = 0);
    BADV("H_negative", d->H = -1);
    BADV("Ws_zero", d->Ws = 0);
    BADV("W_above_2_24", (d->W = (1 << 24) + 1, d->B = 1, d->H = 1, d->depth_row_stride = 1 << 25));
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
    BADV("src_image_stride_short", d->src_image_stride = 53);
    BADV("src_stride_negative", d->src_image_stride = -54);
    BADV("src_plane_too_large", (d->src_row_stride = ((1LL << 29) - 9) / 5 + 1, d->src_image_stride = 1LL << 34));
    /* the matrices of the way back */
    BADE("null_k_src", e->k_src = NULL);
    BADE("null_m_back", e->m_back = NULL);
    BADE("k_src_stride_negative", e->k_src_image_stride = -9);
    BADE("m_back_stride_negative", e->m_back_image_stride = -12);
    BADE("k_src_misaligned", e->k_src = (const float*)0x480002);
    /* the number of sources, the tolerances, the outputs */
    BADC("S_zero", a.S = 0);
    BADC("S_negative", a.S = -1);
    BADC("S_five", a.S = 5);
    BADC("px_tol_negative", a.px_tol = -0.5f);
    BADC("px_tol_nan", a.px_tol = NAN);
    BADC("rel_tol_negative", a.rel_tol = -0.01f);
    BADC("rel_tol_nan", a.rel_tol = NAN);
    BADC("min_views_negative", a.min_views = -1);
    BADC("min_views_above_S", a.min_views = 3);
    BADC("no_output", (a.fused = NULL, a.count = NULL));
    BADC("fused_misaligned", a.fused = (float*)0x700002);
    /* views that disagree in what they must share (each view valid on its own) */
    BADC("differ_B", (a.d[1].B = 1));
    BADC("differ_H", (a.d[1].H = 3));
    BADC("differ_W", (a.d[1].W = 7));
    BADC("differ_depth", (a.d[1].depth = DEPTH + 1));
    BADC("differ_depth_row_stride", (a.d[1].depth_row_stride = 11));
    BADC("differ_mask", (a.d[1].mask = NULL));
    BADC("differ_k", (a.d[1].k = K_ + 9));
    BADC("differ_z_min", (a.d[1].z_min = 1.0f));
    BADC("differ_in_third_view", (a.S = 3, a.d[2].z_max = 5.0f));
    /* the loss's own operands */
    BADL("workspace_small", a.ws_bytes -= 1);
    BADL("workspace_null", a.ws = NULL);
    BADL("workspace_misaligned", a.ws = (void*)0x900004);
    BADL("null_output", (a.loss = NULL, a.g_depth = NULL));
    BADL("output_misaligned", (a.loss = (float*)0xa00002, a.g_depth = (float*)0x800002));
    printf("\"abi\": [%d, %d]\n}\n", nconv_abi_version(), NCONV_ABI_VERSION);
    return 0;
}
