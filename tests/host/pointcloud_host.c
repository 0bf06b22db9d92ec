/* A non-Python host of the back-projection entry points, compiled against include/nconv.h by
 * tests/test_pointcloud_cpu.py: prints the layout of nconv_backproject for the comparison with the
 * ctypes binding, then makes invalid calls that must fail with -EINVAL on the host (no GPU needed)
 * and asks for a workspace size. Plain C99. */
#include <stddef.h>
#include <stdio.h>
#include "nconv.h"

#define F(T, f) printf("\"%s.%s\": [%zu, %zu],\n", #T, #f, offsetof(T, f), sizeof(((T*)0)->f))
#define S(T) printf("\"%s\": [0, %zu],\n", #T, sizeof(T))

int main(void) {
    printf("{\n");
    S(nconv_backproject);
    F(nconv_backproject, B); F(nconv_backproject, H); F(nconv_backproject, W); F(nconv_backproject, color_kind);
    F(nconv_backproject, depth); F(nconv_backproject, depth_image_stride); F(nconv_backproject, depth_row_stride);
    F(nconv_backproject, conf); F(nconv_backproject, conf_image_stride); F(nconv_backproject, conf_row_stride);
    F(nconv_backproject, color); F(nconv_backproject, color_image_stride); F(nconv_backproject, color_channel_stride);
    F(nconv_backproject, color_row_stride); F(nconv_backproject, reverse); F(nconv_backproject, z_min);
    F(nconv_backproject, z_max); F(nconv_backproject, conf_min); F(nconv_backproject, k);
    F(nconv_backproject, k_image_stride);
    printf("\"kinds\": [%d, %d, %d],\n", NCONV_COLOR_NONE, NCONV_COLOR_F32_PLANAR, NCONV_COLOR_U8_INTERLEAVED);

    /* one KITTI-sized frame whose row stride is one element short; the pointers are never dereferenced */
    nconv_backproject d = {0};
    d.B = 1; d.H = 352; d.W = 1216;
    d.depth = (const float*)0x1000; d.depth_row_stride = 1215; d.k = (const float*)0x3000;
    int rc = nconv_backproject_map(&d, (float*)0x2000, NULL);
    printf("\"rc_row_stride\": [%d, \"%s\"],\n", rc, nconv_last_error());
    d.depth_row_stride = 1216;
    rc = nconv_backproject_points(&d, (float*)0x2000, NULL, NULL, 16, (int*)0x4000, (void*)0x5000, 4, NULL);
    printf("\"rc_workspace\": [%d, \"%s\"],\n", rc, nconv_last_error());
    /* 8 x 352 x 1216: 5 segments of 256 pixels per row, one int each */
    printf("\"workspace\": [%zu, %zu],\n", nconv_backproject_workspace_bytes(8, 352, 1216),
           nconv_backproject_workspace_bytes(0, 352, 1216));
    printf("\"abi\": [%d, %d]\n}\n", nconv_abi_version(), NCONV_ABI_VERSION);
    return 0;
}
