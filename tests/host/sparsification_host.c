/* A non-Python host of nconv_depth_sparsification, compiled against include/nconv.h by
 * tests/test_sparsification_cpu.py: prints the layout of struct nconv_depth_sparsification for the
 * comparison with the ctypes binding and the ABI pair, then makes invalid calls that must fail with
 * -EINVAL on the host (no GPU needed). Plain C99. */
#include <stddef.h>
#include <stdio.h>
#include "nconv.h"

#define T nconv_depth_sparsification_desc
#define F(f) printf("\"nconv_depth_sparsification.%s\": [%zu, %zu],\n", #f, offsetof(T, f), sizeof(((T*)0)->f))

static struct nconv_depth_sparsification good(void) {
    /* one KITTI-sized frame; the pointers are never dereferenced */
    struct nconv_depth_sparsification d = {0};
    d.B = 1; d.H = 352; d.W = 1216; d.steps = 100;
    d.pred = (const float*)0x1000000; d.pred_row_stride = 1216;
    d.gt = (const float*)0x2000000; d.gt_row_stride = 1216;
    d.conf = (const float*)0x3000000; d.conf_row_stride = 1216;
    d.gt_max = 80.0f;
    d.curves = (double*)0x4000000;
    return d;
}

static void call(const char* name, const struct nconv_depth_sparsification* d, void* ws, size_t bytes) {
    const int rc = nconv_depth_sparsification(d, ws, bytes, NULL);
    printf("\"%s\": [%d, \"%s\"],\n", name, rc, nconv_last_error());
}

int main(void) {
    printf("{\n");
    printf("\"nconv_depth_sparsification\": [0, %zu],\n", sizeof(T));
    F(B); F(H); F(W); F(steps); F(pred); F(pred_image_stride); F(pred_row_stride); F(gt); F(gt_image_stride);
    F(gt_row_stride); F(conf); F(conf_image_stride); F(conf_row_stride); F(gt_min); F(gt_max); F(clamp_lo);
    F(clamp_hi); F(uncertainty); F(curves); F(order);

    void* ws = (void*)0x8000000;
    const size_t need = nconv_depth_sparsification_workspace_bytes(1, 352, 1216, 100);
    printf("\"workspace_bytes\": [%zu, %zu, %zu, %zu, %zu],\n", need,
           nconv_depth_sparsification_workspace_bytes(0, 352, 1216, 100),
           nconv_depth_sparsification_workspace_bytes(1, 352, 1216, 0),
           nconv_depth_sparsification_workspace_bytes(1, 352, 1216, 1025),
           nconv_depth_sparsification_workspace_bytes(1, 65536, 32768, 100));
    struct nconv_depth_sparsification d;

    call("rc_null_descriptor", NULL, ws, need);
    d = good(); d.pred = NULL; call("rc_null_pred", &d, ws, need);
    d = good(); d.gt = NULL; call("rc_null_gt", &d, ws, need);
    d = good(); d.conf = NULL; call("rc_null_conf", &d, ws, need);
    d = good(); d.curves = NULL; call("rc_null_curves", &d, ws, need);
    d = good(); d.B = 0; call("rc_B", &d, ws, need);
    d = good(); d.H = -1; call("rc_H", &d, ws, need);
    d = good(); d.W = 0; call("rc_W", &d, ws, need);
    d = good(); d.steps = 0; call("rc_steps_low", &d, ws, need);
    d = good(); d.steps = 1025; call("rc_steps_high", &d, ws, need);
    d = good(); d.pred_row_stride = 1215; call("rc_pred_row_stride", &d, ws, need);
    d = good(); d.gt_row_stride = 1215; call("rc_gt_row_stride", &d, ws, need);
    d = good(); d.conf_row_stride = 1215; call("rc_conf_row_stride", &d, ws, need);
    d = good(); call("rc_workspace_small", &d, ws, need - 1);
    d = good(); call("rc_workspace_null", &d, NULL, need);
    d = good(); call("rc_workspace_misaligned", &d, (void*)0x8000004, need);
    /* 352 rows of stride 2^21 elements: ((H - 1) * stride + W) * 4 bytes is past 2^31 */
    d = good(); d.conf_row_stride = 1LL << 21; call("rc_plane_too_large", &d, ws, need);
    /* H * W = 2^31: pixel numbers no longer fit int32 */
    d = good(); d.H = 65536; d.W = 32768; d.pred_row_stride = d.gt_row_stride = d.conf_row_stride = 32768;
    call("rc_pixel_numbers", &d, ws, need);
    d = good(); d.B = 2; d.pred_image_stride = d.gt_image_stride = 352LL * 1216; d.conf_image_stride = 352LL * 1216 - 1;
    call("rc_image_stride", &d, ws, nconv_depth_sparsification_workspace_bytes(2, 352, 1216, 100));
    d = good(); d.gt_min = -1.0f; call("rc_bound", &d, ws, need);
    d = good(); d.curves = (double*)0x4000004; call("rc_curves_misaligned", &d, ws, need);
    d = good(); d.order = (int*)0x5000002; call("rc_order_misaligned", &d, ws, need);
    printf("\"abi\": [%d, %d]\n}\n", nconv_abi_version(), NCONV_ABI_VERSION);
    return 0;
}
