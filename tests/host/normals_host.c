/* A non-Python host of the surface-normal entry points, compiled against include/nconv.h by
 * tests/test_normals_cpu.py: prints the layout of nconv_normals_opts for the comparison with the
 * ctypes binding, then makes invalid calls that must fail with -EINVAL on the host (no GPU needed)
 * and one legal call that launches nothing. Plain C99. */
#include <stddef.h>
#include <stdio.h>
#include "nconv.h"

#define F(T, f) printf("\"%s.%s\": [%zu, %zu],\n", #T, #f, offsetof(T, f), sizeof(((T*)0)->f))
#define S(T) printf("\"%s\": [0, %zu],\n", #T, sizeof(T))

int main(void) {
    printf("{\n");
    S(nconv_normals_opts);
    F(nconv_normals_opts, jump_rel); F(nconv_normals_opts, jump_abs); F(nconv_normals_opts, empty_rgb);

    /* one KITTI-sized frame; the pointers are never dereferenced */
    nconv_backproject d = {0};
    d.B = 1; d.H = 352; d.W = 1216;
    d.depth = (const float*)0x1000; d.depth_row_stride = 1216; d.k = (const float*)0x3000;
    nconv_normals_opts o = {0};
    int rc = nconv_depth_normals(&d, &o, NULL, NULL, NULL);
    printf("\"rc_no_output\": [%d, \"%s\"],\n", rc, nconv_last_error());
    o.jump_rel = -0.5f;
    rc = nconv_depth_normals(&d, &o, (float*)0x2000, NULL, NULL);
    printf("\"rc_jump\": [%d, \"%s\"],\n", rc, nconv_last_error());
    o.jump_rel = 0.1f;
    d.depth_row_stride = 1215;
    rc = nconv_depth_normals_points(&d, &o, (const int*)0x4000, (const int*)0x5000, 16, (float*)0x2000, NULL);
    printf("\"rc_row_stride\": [%d, \"%s\"],\n", rc, nconv_last_error());
    d.depth_row_stride = 1216;
    rc = nconv_depth_normals_points(&d, NULL, (const int*)0x4000, (const int*)0x5000, -1, (float*)0x2000, NULL);
    printf("\"rc_capacity\": [%d, \"%s\"],\n", rc, nconv_last_error());
    /* capacity 0: legal, nothing is launched and no pointer is needed */
    rc = nconv_depth_normals_points(&d, NULL, NULL, NULL, 0, NULL, NULL);
    printf("\"rc_empty\": [%d],\n", rc);
    printf("\"abi\": [%d, %d]\n}\n", nconv_abi_version(), NCONV_ABI_VERSION);
    return 0;
}
