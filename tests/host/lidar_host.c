/* A non-Python host of the LiDAR projection entry points, compiled against include/nconv.h by
 * tests/test_lidar_cpu.py: prints the layout of struct nconv_lidar_project for the comparison with the
 * ctypes binding, then makes every invalid call the header lists, each of which must fail with -EINVAL
 * on the host (no GPU needed; the pointers are never dereferenced), and asks for workspace sizes.
 * Plain C99. */
#include <stddef.h>
#include <stdio.h>
#include "nconv.h"

typedef struct nconv_lidar_project T;
#define F(f) printf("\"nconv_lidar_project.%s\": [%zu, %zu],\n", #f, offsetof(T, f), sizeof(((T*)0)->f))

static float* const DEPTH = (float*)0x20000;
static int* const INDEX = (int*)0x30000;
static void* const WS = (void*)0x40000;

static T good(void) {
    T d = {0};
    d.B = 2; d.H = 4; d.W = 8; d.point_stride = 4;
    d.points = (const float*)0x10000; d.n_rows = 100;
    d.offsets = (const int*)0x50000; d.m = (const float*)0x60000; d.m_image_stride = 12;
    return d;
}

static void call(const char* name, const T* d, float* depth, int* index, void* ws, size_t ws_bytes) {
    int rc = nconv_lidar_project(d, depth, index, ws, ws_bytes, NULL);
    printf("\"rc_%s\": [%d, \"%s\"],\n", name, rc, nconv_last_error());
}

#define BAD(name, defect) do { T d = good(); defect; call(name, &d, DEPTH, NULL, NULL, 0); } while (0)

int main(void) {
    printf("{\n\"nconv_lidar_project\": [0, %zu],\n", sizeof(T));
    F(B); F(H); F(W); F(point_stride); F(points); F(n_rows); F(offsets); F(m); F(m_image_stride); F(z_min);
    F(z_max);
    printf("\"desc_typedef\": %zu,\n", sizeof(nconv_lidar_project_desc));

    const size_t need = 8u * 2 * 4 * 8;
    T g = good();
    call("null_descriptor", NULL, DEPTH, NULL, NULL, 0);
    BAD("null_points", d.points = NULL);
    BAD("null_offsets", d.offsets = NULL);
    BAD("null_m", d.m = NULL);
    call("null_depth", &g, NULL, NULL, NULL, 0);
    BAD("B_zero", d.B = 0);
    BAD("H_zero", d.H = 0);
    BAD("W_negative", d.W = -1);
    BAD("too_many_pixels", (d.B = 1 << 15, d.H = 1 << 8, d.W = 1 << 8));
    BAD("n_rows_negative", d.n_rows = -1);
    BAD("n_rows_2_31", d.n_rows = 1LL << 31);
    BAD("point_stride_2", d.point_stride = 2);
    BAD("z_min_negative", d.z_min = -1.0f);
    BAD("z_min_nan", d.z_min = __builtin_nanf(""));
    BAD("z_max_below_z_min", (d.z_min = 2.0f, d.z_max = 1.0f));
    call("workspace_null", &g, DEPTH, INDEX, NULL, need);
    call("workspace_short", &g, DEPTH, INDEX, WS, need - 1);
    call("workspace_misaligned", &g, DEPTH, INDEX, (char*)WS + 4, need);
    BAD("points_misaligned", d.points = (const float*)0x10002);
    call("depth_misaligned", &g, (float*)0x20002, NULL, NULL, 0);
    call("index_misaligned", &g, DEPTH, (int*)0x30001, WS, need);

    printf("\"workspace\": [%zu, %zu, %zu, %zu, %zu],\n", nconv_lidar_project_workspace_bytes(8, 352, 1216, 0),
           nconv_lidar_project_workspace_bytes(8, 352, 1216, 1), nconv_lidar_project_workspace_bytes(0, 352, 1216, 1),
           nconv_lidar_project_workspace_bytes(2, -1, 8, 1), nconv_lidar_project_workspace_bytes(1 << 15, 1 << 8, 1 << 8, 1));
    printf("\"abi\": [%d, %d]\n}\n", nconv_abi_version(), NCONV_ABI_VERSION);
    return 0;
}
