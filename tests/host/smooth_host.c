/* A non-Python host of the smoothness-loss and edge-weight entry points, compiled against include/nconv.h by
 * tests/test_smooth_cpu.py: prints the descriptors' layouts and the workspace sizes and makes every invalid
 * call the header lists, each of which must fail with -EINVAL on the host (no GPU needed; the pointers are
 * never dereferenced). Plain C99. */
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include "nconv.h"

static const float* const DEPTH = (const float*)0x100000;
static const unsigned char* const MASK = (const unsigned char*)0x200000;
static const float* const WEIGHTS = (const float*)0x300000;
static const float* const IMAGE = (const float*)0x400000;
static float* const OUT = (float*)0x700000;
static void* const WS = (void*)0x900000;
static float* const LOSS = (float*)0xa00000;

typedef struct {
    struct nconv_smooth_loss d;
    float *g_depth, *loss;
    void* ws;
    size_t ws_bytes;
} A;

/* B = 2, a 4 x 8 view cropped out of 5 x 10 planes, first differences, mask and weights */
static A good(void) {
    A a;
    struct nconv_smooth_loss d = {2, 4, 8, 1, DEPTH, 50, 10, MASK, 32, 8, WEIGHTS};
    a.d = d;
    a.g_depth = OUT, a.loss = LOSS;
    a.ws = WS, a.ws_bytes = nconv_smooth_loss_workspace_bytes(2, 4, 8);
    return a;
}

/* B = 2, C = 3, 4 x 8 planes cropped out of 5 x 10 ones */
static struct nconv_edge_weights good_edge(void) {
    struct nconv_edge_weights e = {2, 3, 4, 8, IMAGE, 150, 50, 10, 1.0f / 255.0f};
    return e;
}

static void report(const char* side, const char* name, int rc) {
    printf("\"%s_%s\": [%d, \"%s\"],\n", side, name, rc, rc ? nconv_last_error() : "");
}

/* Every call here must be refused by the host checks: an accepted one would launch on these made-up pointers. */
static void call(const char* name, const A* a) {
    report("fwd", name, nconv_smooth_loss_fwd(&a->d, a->loss, a->ws, a->ws_bytes, NULL));
    report("bwd", name, nconv_smooth_loss_bwd(&a->d, NULL, a->ws, a->ws_bytes, a->g_depth, NULL));
}

#define BAD(name, defect) do { A a = good(); defect; call(name, &a); } while (0)
#define BAD_EDGE(name, defect, out) do { struct nconv_edge_weights e = good_edge(); defect; \
                                         report("edge", name, nconv_edge_weights(&e, out, NULL)); } while (0)

#define FIELD(s, f) printf("\"" #s "." #f "\": [%zu, %zu],\n", offsetof(struct s, f), sizeof(((struct s*)0)->f))

int main(void) {
    printf("{\n\"nconv_smooth_loss\": [0, %zu],\n", sizeof(struct nconv_smooth_loss));
    FIELD(nconv_smooth_loss, B); FIELD(nconv_smooth_loss, H); FIELD(nconv_smooth_loss, W);
    FIELD(nconv_smooth_loss, order); FIELD(nconv_smooth_loss, depth); FIELD(nconv_smooth_loss, depth_image_stride);
    FIELD(nconv_smooth_loss, depth_row_stride); FIELD(nconv_smooth_loss, mask);
    FIELD(nconv_smooth_loss, mask_image_stride); FIELD(nconv_smooth_loss, mask_row_stride);
    FIELD(nconv_smooth_loss, weights);
    printf("\"nconv_edge_weights\": [0, %zu],\n", sizeof(struct nconv_edge_weights));
    FIELD(nconv_edge_weights, B); FIELD(nconv_edge_weights, C); FIELD(nconv_edge_weights, H);
    FIELD(nconv_edge_weights, W); FIELD(nconv_edge_weights, image); FIELD(nconv_edge_weights, image_stride);
    FIELD(nconv_edge_weights, channel_stride); FIELD(nconv_edge_weights, row_stride); FIELD(nconv_edge_weights, alpha);
    printf("\"ws\": [%zu, %zu, %zu, %zu, %zu],\n", nconv_smooth_loss_workspace_bytes(2, 4, 8),
           nconv_smooth_loss_workspace_bytes(8, 352, 1216), nconv_smooth_loss_workspace_bytes(0, 4, 8),
           nconv_smooth_loss_workspace_bytes(1, 4, -1), nconv_smooth_loss_workspace_bytes(3, 17, 65));
    report("fwd", "null_descriptor", nconv_smooth_loss_fwd(NULL, LOSS, WS, 1 << 20, NULL));
    report("bwd", "null_descriptor", nconv_smooth_loss_bwd(NULL, NULL, WS, 1 << 20, OUT, NULL));
    BAD("null_depth", a.d.depth = NULL);
    BAD("order_0", a.d.order = 0);
    BAD("order_3", a.d.order = 3);
    BAD("order_negative", a.d.order = -1);
    BAD("B_zero", a.d.B = 0);
    BAD("H_negative", a.d.H = -1);
    BAD("W_zero", a.d.W = 0);
    BAD("batch_too_large", (a.d.B = 1 << 20, a.d.H = 64, a.d.W = 64, a.d.depth_row_stride = 64,
                            a.d.depth_image_stride = 4096));
    BAD("depth_misaligned", a.d.depth = (const float*)0x100002);
    BAD("weights_misaligned", a.d.weights = (const float*)0x300002);
    BAD("depth_row_stride_short", a.d.depth_row_stride = 7);
    BAD("depth_row_stride_negative", a.d.depth_row_stride = -10);
    BAD("depth_image_stride_short", a.d.depth_image_stride = 39);
    BAD("mask_row_stride_short", a.d.mask_row_stride = 7);
    BAD("mask_image_stride_short", a.d.mask_image_stride = 31);
    /* an extent of 2^31 bytes: (rows - 1) * row stride + columns = 2^29 elements of 4 bytes */
    BAD("depth_plane_too_large", (a.d.B = 1, a.d.depth_row_stride = ((1LL << 29) - 8) / 3 + 1));
    BAD("mask_plane_too_large", (a.d.B = 1, a.d.mask_row_stride = ((1LL << 31) - 8) / 3 + 1));
    BAD("workspace_small", a.ws_bytes -= 1);
    BAD("workspace_null", a.ws = NULL);
    BAD("workspace_misaligned", a.ws = (void*)0x900004);
    BAD("null_output", (a.loss = NULL, a.g_depth = NULL));
    BAD("output_misaligned", (a.loss = (float*)0xa00002, a.g_depth = (float*)0x700002));
    { A a = good(); a.g_depth = (float*)(DEPTH + 20); report("bwd", "g_depth_overlaps_depth",
          nconv_smooth_loss_bwd(&a.d, NULL, a.ws, a.ws_bytes, a.g_depth, NULL)); }
    /* the edge weights */
    report("edge", "null_descriptor", nconv_edge_weights(NULL, OUT, NULL));
    BAD_EDGE("null_image", e.image = NULL, OUT);
    BAD_EDGE("null_weights", (void)e, NULL);
    BAD_EDGE("C_2", e.C = 2, OUT);
    BAD_EDGE("C_0", e.C = 0, OUT);
    BAD_EDGE("B_zero", e.B = 0, OUT);
    BAD_EDGE("W_negative", e.W = -8, OUT);
    BAD_EDGE("batch_too_large", (e.B = 1 << 20, e.H = 32, e.W = 32, e.row_stride = 32, e.channel_stride = 1024,
                                 e.image_stride = 3072), OUT);
    BAD_EDGE("alpha_negative", e.alpha = -1.0f, OUT);
    BAD_EDGE("alpha_nan", e.alpha = NAN, OUT);
    BAD_EDGE("alpha_infinite", e.alpha = INFINITY, OUT);
    BAD_EDGE("image_misaligned", e.image = (const float*)0x400002, OUT);
    BAD_EDGE("weights_misaligned", (void)e, (float*)0x700002);
    BAD_EDGE("row_stride_short", e.row_stride = 7, OUT);
    BAD_EDGE("channel_stride_short", e.channel_stride = 39, OUT);
    BAD_EDGE("image_stride_short", e.image_stride = 139, OUT);
    BAD_EDGE("stride_negative", e.image_stride = -150, OUT);
    BAD_EDGE("plane_too_large", (e.B = 1, e.C = 1, e.row_stride = ((1LL << 29) - 8) / 3 + 1), OUT);
    BAD_EDGE("weights_overlap_image", (void)e, (float*)(IMAGE + 40));
    printf("\"abi\": [%d, %d]\n}\n", nconv_abi_version(), NCONV_ABI_VERSION);
    return 0;
}
