/* A non-Python host of the occlusion filter's entry point, compiled against include/nconv.h by
 * tests/test_occlusion_cpu.py: prints the layout of struct nconv_depth_occlusion for the comparison
 * with the ctypes binding, then makes every invalid call the header lists, each of which must fail with
 * -EINVAL on the host (no GPU needed; the pointers are never dereferenced). Plain C99. */
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include "nconv.h"

typedef struct nconv_depth_occlusion T;
#define F(f) printf("\"nconv_depth_occlusion.%s\": [%zu, %zu],\n", #f, offsetof(T, f), sizeof(((T*)0)->f))

static float* const DST = (float*)0x200000;
static unsigned char* const REMOVED = (unsigned char*)0x300001;
static int* const INDEX = (int*)0x400000;
static int* const COUNTS = (int*)0x500000;

static T good(void) {
    T d = {0};
    d.B = 2; d.H = 4; d.W = 8; d.rh = 3; d.rw = 3; d.min_support = 1;
    d.src = (const float*)0x100000; d.src_image_stride = 40; d.src_row_stride = 10;
    d.jump_abs = 1.0f; d.jump_rel = 0.0f; d.floor = 0.0f;
    return d;
}

static void call(const char* name, const T* d, float* dst, long long dbs, long long drs, int* index, int* counts) {
    int rc = nconv_depth_occlusion(d, dst, dbs, drs, REMOVED, index, counts, NULL);
    printf("\"rc_%s\": [%d, \"%s\"],\n", name, rc, nconv_last_error());
}

#define BAD(name, defect) do { T d = good(); defect; call(name, &d, DST, 32, 8, INDEX, COUNTS); } while (0)

int main(void) {
    printf("{\n\"nconv_depth_occlusion\": [0, %zu],\n", sizeof(T));
    F(B); F(H); F(W); F(rh); F(rw); F(min_support); F(src); F(src_image_stride); F(src_row_stride); F(jump_abs);
    F(jump_rel); F(floor);
    printf("\"desc_typedef\": %zu,\n", sizeof(nconv_depth_occlusion_desc));

    T g = good();
    call("null_descriptor", NULL, DST, 32, 8, INDEX, COUNTS);
    BAD("null_src", d.src = NULL);
    call("null_dst", &g, NULL, 32, 8, INDEX, COUNTS);
    BAD("B_zero", d.B = 0);
    BAD("H_zero", d.H = 0);
    BAD("W_negative", d.W = -1);
    BAD("too_many_pixels", (d.B = 1 << 15, d.H = 1 << 8, d.W = 1 << 8));
    BAD("rh_negative", d.rh = -1);
    BAD("rh_17", d.rh = 17);
    BAD("rw_negative", d.rw = -1);
    BAD("rw_17", d.rw = 17);
    BAD("jump_abs_negative", d.jump_abs = -0.5f);
    BAD("jump_abs_nan", d.jump_abs = NAN);
    BAD("jump_rel_negative", d.jump_rel = -0.5f);
    BAD("jump_rel_nan", d.jump_rel = NAN);
    BAD("floor_nan", d.floor = NAN);
    BAD("min_support_zero", d.min_support = 0);
    BAD("src_misaligned", d.src = (const float*)0x100002);
    call("dst_misaligned", &g, (float*)0x200002, 32, 8, INDEX, COUNTS);
    call("index_misaligned", &g, DST, 32, 8, (int*)0x400001, COUNTS);
    call("counts_misaligned", &g, DST, 32, 8, INDEX, (int*)0x500002);
    BAD("src_row_stride_short", d.src_row_stride = 7);
    BAD("src_image_stride_short", d.src_image_stride = 39);
    call("dst_row_stride_short", &g, DST, 32, 7, INDEX, COUNTS);
    call("dst_image_stride_short", &g, DST, 31, 8, INDEX, COUNTS);
    BAD("src_image_2_31_bytes", (d.B = 1, d.src_row_stride = 1LL << 28));
    {
        T d = good();
        d.B = 1;
        call("dst_image_2_31_bytes", &d, DST, 0, 1LL << 28, INDEX, COUNTS);
    }
    /* dst begins inside src's extent; dst's last byte is src's first pixel; dst is src */
    call("overlap_inside", &g, (float*)g.src + 12, 32, 8, INDEX, COUNTS);
    call("overlap_tail", &g, (float*)g.src - (32 + 3 * 8 + 7), 32, 8, INDEX, COUNTS);
    call("overlap_same", &g, (float*)g.src, 40, 10, INDEX, COUNTS);
    printf("\"abi\": [%d, %d]\n}\n", nconv_abi_version(), NCONV_ABI_VERSION);
    return 0;
}
