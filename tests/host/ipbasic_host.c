/* A non-Python host of the IP-Basic entry point, compiled against include/nconv.h by
 * tests/test_ipbasic_cpu.py: prints the layout of struct nconv_depth_ipbasic for the comparison with the
 * ctypes binding, then makes every invalid call the header lists, each of which must fail with -EINVAL on
 * the host (no GPU needed; the pointers are never dereferenced). Plain C99. */
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include "nconv.h"

typedef struct nconv_depth_ipbasic T;
#define F(f) printf("\"nconv_depth_ipbasic.%s\": [%zu, %zu],\n", #f, offsetof(T, f), sizeof(((T*)0)->f))

static float* const DST = (float*)0x200000;
static float* const WORK = (float*)0x300000;
static int* const TOP = (int*)0x400000;

static T good(void) {
    T d = {0};
    d.B = 2; d.H = 4; d.W = 8;
    d.src = (const float*)0x100000; d.src_image_stride = 40; d.src_row_stride = 10;
    d.max_depth = 100.0f; d.kernel_shape = NCONV_IPBASIC_DIAMOND; d.kernel_size = 5;
    d.extrapolate = 1; d.median = 1; d.blur = NCONV_IPBASIC_BLUR_GAUSSIAN; d.keep_samples = 0;
    return d;
}

static void call(const char* name, const T* d, float* dst, long long dbs, long long drs, float* work, int* top) {
    int rc = nconv_depth_ipbasic(d, dst, dbs, drs, work, top, NULL);
    printf("\"rc_%s\": [%d, \"%s\"],\n", name, rc, nconv_last_error());
}

#define BAD(name, defect) do { T d = good(); defect; call(name, &d, DST, 32, 8, WORK, TOP); } while (0)

int main(void) {
    printf("{\n\"nconv_depth_ipbasic\": [0, %zu],\n", sizeof(T));
    F(B); F(H); F(W); F(src); F(src_image_stride); F(src_row_stride); F(max_depth); F(kernel_shape); F(kernel_size);
    F(extrapolate); F(median); F(blur); F(keep_samples);
    printf("\"desc_typedef\": %zu,\n", sizeof(nconv_depth_ipbasic_desc));
    printf("\"enums\": [%d, %d, %d, %d, %d],\n", NCONV_IPBASIC_FULL, NCONV_IPBASIC_CROSS, NCONV_IPBASIC_DIAMOND,
           NCONV_IPBASIC_BLUR_NONE, NCONV_IPBASIC_BLUR_GAUSSIAN);

    T g = good();
    call("null_descriptor", NULL, DST, 32, 8, WORK, TOP);
    BAD("null_src", d.src = NULL);
    call("null_dst", &g, NULL, 32, 8, WORK, TOP);
    BAD("B_zero", d.B = 0);
    BAD("H_zero", d.H = 0);
    BAD("W_negative", d.W = -1);
    BAD("too_many_pixels", (d.B = 1 << 15, d.H = 1 << 8, d.W = 1 << 8));
    BAD("shape_negative", d.kernel_shape = -1);
    BAD("shape_3", d.kernel_shape = 3);
    BAD("size_4", d.kernel_size = 4);
    BAD("size_9", d.kernel_size = 9);
    BAD("size_1", d.kernel_size = 1);
    BAD("blur_2", d.blur = 2);
    BAD("blur_negative", d.blur = -1);
    BAD("max_depth_nan", d.max_depth = NAN);
    BAD("max_depth_inf", d.max_depth = INFINITY);
    BAD("max_depth_2T", d.max_depth = 2.0f * 0.1f);
    BAD("max_depth_negative", d.max_depth = -100.0f);
    BAD("src_misaligned", d.src = (const float*)0x100002);
    call("dst_misaligned", &g, (float*)0x200002, 32, 8, WORK, TOP);
    call("work_misaligned", &g, DST, 32, 8, (float*)0x300001, TOP);
    call("top_misaligned", &g, DST, 32, 8, WORK, (int*)0x400002);
    BAD("src_row_stride_short", d.src_row_stride = 7);
    BAD("src_image_stride_short", d.src_image_stride = 39);
    call("dst_row_stride_short", &g, DST, 32, 7, WORK, TOP);
    call("dst_image_stride_short", &g, DST, 31, 8, WORK, TOP);
    BAD("src_image_2_31_bytes", (d.B = 1, d.src_row_stride = 1LL << 28));
    {
        T d = good();
        d.B = 1;
        call("dst_image_2_31_bytes", &d, DST, 0, 1LL << 28, WORK, TOP);
    }
    /* dst begins inside src's extent; dst's last byte is src's first pixel; dst is src */
    call("overlap_inside", &g, (float*)g.src + 12, 32, 8, WORK, TOP);
    call("overlap_tail", &g, (float*)g.src - (32 + 3 * 8 + 7), 32, 8, WORK, TOP);
    call("overlap_same", &g, (float*)g.src, 40, 10, WORK, TOP);
    /* extrapolate needs both workspaces, apart from src, dst and each other */
    call("work_missing", &g, DST, 32, 8, NULL, TOP);
    call("top_missing", &g, DST, 32, 8, WORK, NULL);
    call("work_is_src", &g, DST, 32, 8, (float*)g.src, TOP);
    call("top_in_dst", &g, DST, 32, 8, WORK, (int*)(DST + 4));
    call("top_in_work", &g, DST, 32, 8, WORK, (int*)(WORK + 8));
    printf("\"abi\": [%d, %d]\n}\n", nconv_abi_version(), NCONV_ABI_VERSION);
    return 0;
}
