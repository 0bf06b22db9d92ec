/* A non-Python host of the depth colouring entry points, compiled against include/nconv.h by
 * tests/test_colorize_cpu.py: prints the layout of struct nconv_depth_colorize for the comparison with
 * the ctypes binding, then makes every invalid call the header lists, each of which must fail with
 * -EINVAL on the host (no GPU needed; the pointers are never dereferenced), and asks for workspace
 * sizes. Plain C99. */
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include "nconv.h"

typedef struct nconv_depth_colorize T;
#define F(f) printf("\"nconv_depth_colorize.%s\": [%zu, %zu],\n", #f, offsetof(T, f), sizeof(((T*)0)->f))

static unsigned char* const OUT = (unsigned char*)0x20001;
static void* const WS = (void*)0x40000;

static T good(void) {
    T d = {0};
    d.B = 2; d.H = 4; d.W = 8; d.radius = 1;
    d.depth = (const float*)0x10000; d.image_stride = 40; d.row_stride = 10;
    d.cmap_id = 0; d.auto_range = 1; d.floor = -INFINITY;
    return d;
}

static void call(const char* name, const T* d, unsigned char* out, void* ws, size_t ws_bytes) {
    int rc = nconv_depth_colorize(d, out, ws, ws_bytes, NULL);
    printf("\"rc_%s\": [%d, \"%s\"],\n", name, rc, nconv_last_error());
}

#define BAD(name, defect) do { T d = good(); defect; call(name, &d, OUT, WS, 16); } while (0)

int main(void) {
    printf("{\n\"nconv_depth_colorize\": [0, %zu],\n", sizeof(T));
    F(B); F(H); F(W); F(radius); F(depth); F(image_stride); F(row_stride); F(lut); F(cmap_id); F(auto_range);
    F(vmin); F(vmax); F(floor); F(bgr); F(background); F(background_image_stride); F(background_row_stride);
    F(empty_rgb);
    printf("\"desc_typedef\": %zu,\n", sizeof(nconv_depth_colorize_desc));

    T g = good();
    call("null_descriptor", NULL, OUT, WS, 16);
    BAD("null_depth", d.depth = NULL);
    call("null_out", &g, NULL, WS, 16);
    BAD("B_zero", d.B = 0);
    BAD("H_zero", d.H = 0);
    BAD("W_negative", d.W = -1);
    BAD("too_many_pixels", (d.B = 1 << 15, d.H = 1 << 8, d.W = 1 << 8));
    BAD("radius_negative", d.radius = -1);
    BAD("radius_5", d.radius = 5);
    BAD("cmap_id_5", d.cmap_id = 5);
    BAD("cmap_id_negative", d.cmap_id = -1);
    BAD("vmin_nan", (d.auto_range = 0, d.vmin = NAN, d.vmax = 1.0f));
    BAD("vmax_nan", (d.auto_range = 0, d.vmin = 0.0f, d.vmax = NAN));
    BAD("floor_nan", d.floor = NAN);
    call("workspace_null", &g, OUT, NULL, 16);
    call("workspace_short", &g, OUT, WS, 15);
    call("workspace_misaligned", &g, OUT, (char*)WS + 4, 16);
    BAD("depth_misaligned", d.depth = (const float*)0x10002);
    BAD("row_stride_short", d.row_stride = 7);
    BAD("image_stride_short", d.image_stride = 39);
    BAD("background_row_stride_short", (d.background = (const unsigned char*)0x50000, d.background_row_stride = 23,
                                        d.background_image_stride = 1000));

    printf("\"workspace\": [%zu, %zu, %zu, %zu],\n", nconv_depth_colorize_workspace_bytes(1),
           nconv_depth_colorize_workspace_bytes(8), nconv_depth_colorize_workspace_bytes(0),
           nconv_depth_colorize_workspace_bytes(-3));
    printf("\"abi\": [%d, %d]\n}\n", nconv_abi_version(), NCONV_ABI_VERSION);
    return 0;
}
