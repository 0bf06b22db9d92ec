/* A non-Python host of the pose-alignment entry points, compiled against include/nconv.h by
 * tests/test_pose_host_cpu.py: prints the descriptor's layout and the workspace sizes and makes every invalid
 * call the header lists, each of which must fail with -EINVAL on the host (no GPU needed; the pointers are
 * never dereferenced). Plain C99. */
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include "nconv.h"

static const float* const DEPTH = (const float*)0x100000;
static const unsigned char* const MASK = (const unsigned char*)0x200000;
static const float* const SRC = (const float*)0x300000;
static const float* const K_ = (const float*)0x400000;
static float* const M_ = (float*)0x500000;
static const float* const TGT = (const float*)0x600000;
static const float* const KS = (const float*)0x700000;
static float* const POSE = (float*)0x800000;
static void* const WS = (void*)0x900000;
static int* const STATUS = (int*)0xa00000;
static float* const COST = (float*)0xb00000;
static int* const NH = (int*)0xc00000;

typedef struct {
    struct nconv_pose_align d;
    void* ws;
    size_t ws_bytes;
    int it;
} A;

/* B = 2, C = 3, a 4 x 8 target cropped out of 5 x 10 planes, a 6 x 9 source, a history of 9 */
static A good(void) {
    A a;
    struct nconv_pose_align d = {2, 3, 4, 8, 6, 9, DEPTH, 50, 10, MASK, 32, 8, SRC, 162, 54, 9, K_, 9, M_, 12, 0.001f, 0.0f,
                                 TGT, 96, 32, 8, KS, 9, POSE, STATUS, COST, NH, 9, 10.0f, 1e-4f, 32};
    a.d = d;
    a.ws = WS, a.ws_bytes = nconv_pose_workspace_bytes(2, 4, 8), a.it = 0;
    return a;
}

static void report(const char* side, const char* name, int rc) {
    printf("\"%s_%s\": [%d, \"%s\"],\n", side, name, rc, rc ? nconv_last_error() : "");
}

/* Every call here must be refused by the host checks: an accepted one would launch on these made-up pointers. */
static void call(const char* name, const A* a) {
    report("neq", name, nconv_pose_normal_eq(&a->d, a->ws, a->ws_bytes, NULL));
    report("upd", name, nconv_pose_update(&a->d, a->ws, a->ws_bytes, a->it, 1, NULL));
}

#define BAD(name, defect) do { A a = good(); defect; call(name, &a); } while (0)
#define BAD_UPDATE(name, defect) do { A a = good(); defect; \
    report("upd", name, nconv_pose_update(&a.d, a.ws, a.ws_bytes, a.it, 1, NULL)); } while (0)

#define FIELD(f) printf("\"nconv_pose_align." #f "\": [%zu, %zu],\n", offsetof(struct nconv_pose_align, f), \
                        sizeof(((struct nconv_pose_align*)0)->f))

int main(void) {
    printf("{\n\"nconv_pose_align\": [0, %zu],\n", sizeof(struct nconv_pose_align));
    FIELD(B); FIELD(C); FIELD(H); FIELD(W); FIELD(Hs); FIELD(Ws); FIELD(depth); FIELD(depth_image_stride);
    FIELD(depth_row_stride); FIELD(mask); FIELD(mask_image_stride); FIELD(mask_row_stride); FIELD(src);
    FIELD(src_image_stride); FIELD(src_channel_stride); FIELD(src_row_stride); FIELD(k); FIELD(k_image_stride);
    FIELD(m); FIELD(m_image_stride); FIELD(z_min); FIELD(z_max); FIELD(tgt); FIELD(tgt_image_stride);
    FIELD(tgt_channel_stride); FIELD(tgt_row_stride); FIELD(k_src); FIELD(k_src_image_stride); FIELD(pose);
    FIELD(status); FIELD(cost); FIELD(n_hist); FIELD(history); FIELD(huber); FIELD(damping); FIELD(min_points);
    printf("\"ws\": [%zu, %zu, %zu, %zu, %zu],\n", nconv_pose_workspace_bytes(2, 4, 8),
           nconv_pose_workspace_bytes(8, 352, 1216), nconv_pose_workspace_bytes(0, 4, 8),
           nconv_pose_workspace_bytes(1, 4, -1), nconv_pose_workspace_bytes(3, 17, 65));
    report("neq", "null_descriptor", nconv_pose_normal_eq(NULL, WS, 1 << 20, NULL));
    report("upd", "null_descriptor", nconv_pose_update(NULL, WS, 1 << 20, 0, 1, NULL));
    /* the fields shared with nconv_view_warp */
    BAD("null_depth", a.d.depth = NULL);
    BAD("null_src", a.d.src = NULL);
    BAD("null_k", a.d.k = NULL);
    BAD("null_m", a.d.m = NULL);
    BAD("C_2", a.d.C = 2);
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
    BAD("depth_image_stride_short", a.d.depth_image_stride = 39);
    BAD("mask_row_stride_short", a.d.mask_row_stride = 7);
    BAD("mask_image_stride_short", a.d.mask_image_stride = 31);
    BAD("src_row_stride_short", a.d.src_row_stride = 8);
    BAD("src_channel_stride_short", a.d.src_channel_stride = 53);
    BAD("src_image_stride_short", a.d.src_image_stride = 161);
    BAD("depth_plane_too_large", (a.d.B = 1, a.d.depth_row_stride = ((1LL << 29) - 8) / 3 + 1));
    BAD("src_plane_too_large", (a.d.B = 1, a.d.C = 1, a.d.src_row_stride = ((1LL << 29) - 9) / 5 + 1));
    /* the target frame */
    BAD("null_tgt", a.d.tgt = NULL);
    BAD("tgt_misaligned", a.d.tgt = (const float*)0x600002);
    BAD("tgt_row_stride_short", a.d.tgt_row_stride = 7);
    BAD("tgt_channel_stride_short", a.d.tgt_channel_stride = 31);
    BAD("tgt_plane_too_large", (a.d.B = 1, a.d.C = 1, a.d.tgt_row_stride = ((1LL << 29) - 8) / 3 + 1));
    /* the new fields */
    BAD("null_k_src", a.d.k_src = NULL);
    BAD("null_pose", a.d.pose = NULL);
    BAD("null_status", a.d.status = NULL);
    BAD("null_cost", a.d.cost = NULL);
    BAD("null_n_hist", a.d.n_hist = NULL);
    BAD("pose_misaligned", a.d.pose = (float*)0x800002);
    BAD("k_src_stride_negative", a.d.k_src_image_stride = -9);
    BAD("m_stride_shared", a.d.m_image_stride = 0);
    BAD("m_stride_below_12", a.d.m_image_stride = 11);
    BAD("huber_negative", a.d.huber = -1.0f);
    BAD("huber_nan", a.d.huber = NAN);
    BAD("damping_negative", a.d.damping = -1e-4f);
    BAD("damping_nan", a.d.damping = NAN);
    BAD("min_points_5", a.d.min_points = 5);
    BAD("history_zero", a.d.history = 0);
    BAD("workspace_small", a.ws_bytes -= 1);
    BAD("workspace_null", a.ws = NULL);
    BAD("workspace_misaligned", a.ws = (void*)0x900004);
    BAD_UPDATE("it_negative", a.it = -1);
    BAD_UPDATE("it_past_history", a.it = 9);
    printf("\"abi\": [%d, %d]\n}\n", nconv_abi_version(), NCONV_ABI_VERSION);
    return 0;
}
