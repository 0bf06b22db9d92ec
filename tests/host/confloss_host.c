/* A non-Python host of the confidence-loss entry points and nconv_bwd_tail_conf, compiled against
 * include/nconv.h by tests/test_confloss_cpu.py: makes every invalid call the header lists, each of which
 * must fail with -EINVAL on the host (no GPU needed; the pointers are never dereferenced), and checks that
 * nconv_bwd_tail_conf without the extra plane is nconv_bwd_ex. Plain C99. */
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include "nconv.h"

static const float* const R_ = (const float*)0x100000;
static const float* const C_ = (const float*)0x200000;
static const float* const T_ = (const float*)0x300000;
static const float* const LAM = (const float*)0x400000;
static float* const LOSS = (float*)0x500000;
static void* const WS = (void*)0x600000;
static float* const GR = (float*)0x700000;
static float* const GC = (float*)0x800000;

typedef struct {
    const float *r, *c, *t, *lam;
    long long rbs, rrs, cbs, crs, tbs, trs;
    int B, H, W, kind;
    float beta;
    float* loss;
    void* ws;
    size_t ws_bytes;
    float *g_r, *g_c;
} A;

static A good(void) {
    A a = {R_, C_, T_, LAM, 40, 10, 32, 8, 32, 8, 2, 4, 8, NCONV_CONF_LOSS_SMOOTH_L1, 1.0f, LOSS, WS, 0, GR, GC};
    a.ws_bytes = nconv_conf_loss_workspace_bytes(2, 4, 8);
    return a;
}

/* Every call here must be refused by the host checks: an accepted one would launch on these made-up
 * pointers. The backward takes no workspace, so the workspace defects go to the forward alone. */
static void call_fwd(const char* name, const A* a) {
    int rf = nconv_conf_loss_fwd(a->r, a->rbs, a->rrs, a->c, a->cbs, a->crs, a->t, a->tbs, a->trs, a->B, a->H, a->W,
                                 a->kind, a->beta, a->lam, a->loss, a->ws, a->ws_bytes, NULL);
    printf("\"fwd_%s\": [%d, \"%s\"],\n", name, rf, rf ? nconv_last_error() : "");
}

static void call(const char* name, const A* a) {
    call_fwd(name, a);
    int rb = nconv_conf_loss_bwd(a->r, a->rbs, a->rrs, a->c, a->cbs, a->crs, a->t, a->tbs, a->trs, a->B, a->H, a->W,
                                 a->kind, a->beta, a->lam, NULL, a->g_r, a->g_c, NULL);
    printf("\"bwd_%s\": [%d, \"%s\"],\n", name, rb, rb ? nconv_last_error() : "");
}

#define BAD(name, defect) do { A a = good(); defect; call(name, &a); } while (0)

int main(void) {
    printf("{\n\"ws\": [%zu, %zu, %zu, %zu],\n", nconv_conf_loss_workspace_bytes(2, 4, 8),
           nconv_conf_loss_workspace_bytes(8, 352, 1216), nconv_conf_loss_workspace_bytes(0, 4, 8),
           nconv_conf_loss_workspace_bytes(1, 4, -1));
    BAD("null_r", a.r = NULL);
    BAD("null_c", a.c = NULL);
    BAD("null_t", a.t = NULL);
    BAD("null_lam", a.lam = NULL);
    BAD("B_zero", a.B = 0);
    BAD("H_negative", a.H = -1);
    BAD("beta_zero", a.beta = 0.0f);
    BAD("beta_negative", a.beta = -1.0f);
    BAD("beta_nan", a.beta = NAN);
    BAD("kind_2", a.kind = 2);
    BAD("kind_negative", a.kind = -1);
    BAD("r_row_stride_short", a.rrs = 7);
    BAD("c_image_stride_short", a.cbs = 31);
    /* an extent of 2^31 bytes: (H - 1) * row stride + W = 2^29 elements of 4 bytes */
    BAD("r_plane_too_large", (a.B = 1, a.rrs = ((1LL << 29) - 8) / 3 + 1));
    BAD("c_plane_too_large", (a.B = 1, a.crs = ((1LL << 29) - 8) / 3 + 1));
    BAD("t_plane_too_large", (a.B = 1, a.trs = ((1LL << 29) - 8) / 3 + 1));
    /* forward only: the loss and its workspace; backward only: both outputs absent */
    BAD("null_loss_or_outputs", (a.loss = NULL, a.g_r = NULL, a.g_c = NULL));
    { A a = good(); a.ws_bytes -= 1; call_fwd("workspace_small_fwd_only", &a); }
    { A a = good(); a.ws = NULL; call_fwd("workspace_null_fwd_only", &a); }

    /* nconv_bwd_tail_conf: the NULL plane is nconv_bwd_ex (the same checks, the same message); the plane
     * without a tail is refused. nconv6's geometry at 16 x 16, a workspace one byte short. */
    nconv_layer L = {0};
    L.B = 1; L.Cin = 16; L.H = 16; L.W = 16; L.Cout = 8; L.Ho = 14; L.Wo = 14;
    L.KH = L.KW = 3; L.SH = L.SW = L.DH = L.DW = L.groups = 1; L.PH = L.PW = 0; L.eps = 1e-20f;
    L.load_mode = NCONV_LOAD_UPCAT_UP_FIRST; L.thresh = 0.01f; L.math = NCONV_MATH_FP32; L.bwd_math = NCONV_MATH_FP32;
    L.a.x = R_; L.a.c = C_; L.a.C = 8; L.a.H = 16; L.a.W = 16;
    L.b.x = R_; L.b.c = C_; L.b.C = 8; L.b.H = 8; L.b.W = 8;
    L.weight = R_; L.bias = R_; L.wsum = R_;
    size_t need = nconv_bwd_workspace_bytes(&L);
    nconv_bwd_io io = {0};
    io.y = R_; io.cout = C_; io.gy = T_; io.gxa = GR;
    int r0 = nconv_bwd_ex(&L, &io, WS, need - 1, 0, NULL);
    printf("\"tail_ex\": [%d, \"%s\"],\n", r0, nconv_last_error());
    int r1 = nconv_bwd_tail_conf(&L, &io, NULL, WS, need - 1, 0, NULL);
    printf("\"tail_conf_null\": [%d, \"%s\"],\n", r1, nconv_last_error());
    int r2 = nconv_bwd_tail_conf(&L, &io, GC, WS, need, 0, NULL);
    printf("\"tail_conf_no_tail\": [%d, \"%s\"],\n", r2, nconv_last_error());
    int r3 = nconv_bwd_tail_conf(&L, NULL, NULL, WS, need, 0, NULL);
    printf("\"tail_conf_null_io\": [%d, \"%s\"],\n", r3, nconv_last_error());
    printf("\"need\": [%zu, 0],\n", need);
    printf("\"abi\": [%d, %d]\n}\n", nconv_abi_version(), NCONV_ABI_VERSION);
    return 0;
}
