/* A non-Python host of the frame entry points, compiled against include/nconv.h by
 * tests/test_frames_cpu.py: prints the layout of nconv_frame_plane / nconv_frame_ingest for the
 * comparison with the ctypes binding, then makes two invalid calls that must fail with -EINVAL
 * on the host (no GPU needed). Plain C99. */
#include <stddef.h>
#include <stdio.h>
#include "nconv.h"

#define F(T, f) printf("\"%s.%s\": [%zu, %zu],\n", #T, #f, offsetof(T, f), sizeof(((T*)0)->f))
#define S(T) printf("\"%s\": [0, %zu],\n", #T, sizeof(T))

int main(void) {
    printf("{\n");
    S(nconv_frame_plane);
    F(nconv_frame_plane, src); F(nconv_frame_plane, image_stride); F(nconv_frame_plane, row_stride);
    F(nconv_frame_plane, dtype); F(nconv_frame_plane, shift); F(nconv_frame_plane, scale); F(nconv_frame_plane, out);
    S(nconv_frame_ingest_desc);
    F(nconv_frame_ingest_desc, B); F(nconv_frame_ingest_desc, h); F(nconv_frame_ingest_desc, w);
    F(nconv_frame_ingest_desc, reverse); F(nconv_frame_ingest_desc, rgb); F(nconv_frame_ingest_desc, rgb_image_stride);
    F(nconv_frame_ingest_desc, rgb_row_stride); F(nconv_frame_ingest_desc, rgb_out); F(nconv_frame_ingest_desc, plane);
    printf("\"dtypes\": [%d, %d, %d],\n", NCONV_FRAME_U8, NCONV_FRAME_U16, NCONV_FRAME_F32);

    /* a KITTI-style u16 plane whose row stride is one byte short; never dereferenced */
    struct nconv_frame_ingest d = {0};
    d.B = 1; d.h = 4; d.w = 8;
    d.plane[0].src = (const void*)0x1000; d.plane[0].row_stride = 15; d.plane[0].dtype = NCONV_FRAME_U16;
    d.plane[0].shift = 8; d.plane[0].scale = 1.0f / 256.0f; d.plane[0].out = (float*)0x2000;
    int rc = nconv_frame_ingest(&d, NULL);
    printf("\"rc_row_stride\": [%d, \"%s\"],\n", rc, nconv_last_error());
    rc = nconv_depth_export_u16((const float*)0x1000, 32, 8, 1, 4, 8, 0.0f, (unsigned short*)0x2000, NULL);
    printf("\"rc_scale\": [%d, \"%s\"],\n", rc, nconv_last_error());
    printf("\"abi\": [%d, %d]\n}\n", nconv_abi_version(), NCONV_ABI_VERSION);
    return 0;
}
