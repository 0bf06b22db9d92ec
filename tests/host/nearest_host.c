/* A non-Python host of the nearest-sample entry point, compiled against include/nconv.h by
 * tests/test_nearest_cpu.py: prints the layout of struct nconv_depth_nearest for the comparison with the
 * ctypes binding, then makes every invalid call the header lists, each of which must fail with -EINVAL on
 * the host (no GPU needed; the pointers are never dereferenced). Plain C99. */
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include "nconv.h"

typedef struct nconv_depth_nearest T;
#define F(f) printf("\"nconv_depth_nearest.%s\": [%zu, %zu],\n", #f, offsetof(T, f), sizeof(((T*)0)->f))

static float* const DST = (float*)0x200000;
static int* const WORK = (int*)0x300000;
static int* const INDEX = (int*)0x400000;
static int* const DIST2 = (int*)0x500000;
static float* const DIST = (float*)0x600000;

static T good(void) {
    T d = {0};
    d.B = 2; d.H = 4; d.W = 8;
    d.src = (const float*)0x100000; d.src_image_stride = 40; d.src_row_stride = 10;
    d.floor = 0.0f; d.max_dist2 = -1;
    return d;
}

static void call(const char* name, const T* d, float* dst, long long dbs, long long drs, int* index, int* dist2,
                 float* dist, int* work) {
    int rc = nconv_depth_nearest(d, dst, dbs, drs, index, dist2, dist, work, NULL);
    printf("\"rc_%s\": [%d, \"%s\"],\n", name, rc, nconv_last_error());
}

#define BAD(name, defect) do { T d = good(); defect; call(name, &d, DST, 32, 8, INDEX, DIST2, DIST, WORK); } while (0)

int main(void) {
    printf("{\n\"nconv_depth_nearest\": [0, %zu],\n", sizeof(T));
    F(B); F(H); F(W); F(src); F(src_image_stride); F(src_row_stride); F(floor); F(max_dist2);
    printf("\"desc_typedef\": %zu,\n", sizeof(nconv_depth_nearest_desc));

    T g = good();
    call("null_descriptor", NULL, DST, 32, 8, INDEX, DIST2, DIST, WORK);
    BAD("null_src", d.src = NULL);
    call("null_work", &g, DST, 32, 8, INDEX, DIST2, DIST, NULL);
    call("no_output", &g, NULL, 32, 8, NULL, NULL, NULL, WORK);
    BAD("B_zero", d.B = 0);
    BAD("H_zero", d.H = 0);
    BAD("W_negative", d.W = -1);
    BAD("too_many_pixels", (d.B = 1 << 15, d.H = 1 << 8, d.W = 1 << 8));
    BAD("diagonal_too_long_W", (d.B = 1, d.H = 1, d.W = 46341));  /* 46341^2 >= 2^31 */
    BAD("diagonal_too_long_HW", (d.B = 1, d.H = 32768, d.W = 32768));  /* B * H * W = 2^30 */
    BAD("floor_nan", d.floor = NAN);
    BAD("src_misaligned", d.src = (const float*)0x100002);
    call("dst_misaligned", &g, (float*)0x200002, 32, 8, INDEX, DIST2, DIST, WORK);
    call("index_misaligned", &g, DST, 32, 8, (int*)0x400001, DIST2, DIST, WORK);
    call("dist2_misaligned", &g, DST, 32, 8, INDEX, (int*)0x500002, DIST, WORK);
    call("dist_misaligned", &g, DST, 32, 8, INDEX, DIST2, (float*)0x600003, WORK);
    call("work_misaligned", &g, DST, 32, 8, INDEX, DIST2, DIST, (int*)0x300002);
    BAD("src_row_stride_short", d.src_row_stride = 7);
    BAD("src_image_stride_short", d.src_image_stride = 39);
    call("dst_row_stride_short", &g, DST, 32, 7, INDEX, DIST2, DIST, WORK);
    call("dst_image_stride_short", &g, DST, 31, 8, INDEX, DIST2, DIST, WORK);
    BAD("src_image_2_31_bytes", (d.B = 1, d.src_row_stride = 1LL << 28));
    {
        T d = good();
        d.B = 1;
        call("dst_image_2_31_bytes", &d, DST, 0, 1LL << 28, INDEX, DIST2, DIST, WORK);
    }
    /* dst begins inside src's extent; dst's last byte is src's first pixel; dst is src */
    call("dst_overlap_inside", &g, (float*)g.src + 12, 32, 8, INDEX, DIST2, DIST, WORK);
    call("dst_overlap_tail", &g, (float*)g.src - (32 + 3 * 8 + 7), 32, 8, INDEX, DIST2, DIST, WORK);
    call("dst_overlap_same", &g, (float*)g.src, 40, 10, INDEX, DIST2, DIST, WORK);
    /* work and every output apart from src and from each other: a (2, 4, 8) plane is 64 elements */
    call("work_is_src", &g, DST, 32, 8, INDEX, DIST2, DIST, (int*)g.src);
    call("work_in_dst", &g, DST, 32, 8, INDEX, DIST2, DIST, (int*)(DST + 63));
    call("index_in_src", &g, DST, 32, 8, (int*)g.src + 77, DIST2, DIST, WORK);
    call("index_in_work", &g, NULL, 0, 0, WORK + 8, NULL, NULL, WORK);
    call("dist2_in_work", &g, DST, 32, 8, INDEX, WORK - 63, DIST, WORK);
    call("dist2_is_index", &g, NULL, 0, 0, INDEX, INDEX, NULL, WORK);
    call("dist_in_dst", &g, DST, 32, 8, INDEX, DIST2, DST + 4, WORK);
    call("dist_in_dist2", &g, NULL, 0, 0, NULL, DIST2, (float*)(DIST2 + 63), WORK);
    call("dist_in_src", &g, NULL, 0, 0, NULL, NULL, (float*)g.src - 63, WORK);
    printf("\"abi\": [%d, %d]\n}\n", nconv_abi_version(), NCONV_ABI_VERSION);
    return 0;
}
