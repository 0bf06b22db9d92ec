/* A non-Python host of nconv_voxel_merge, compiled against include/nconv.h by tests/test_voxel_cpu.py: prints
 * the layout of struct nconv_voxel_merge_args for the comparison with the ctypes binding and the ABI pair, the
 * workspace query at several sizes, then makes invalid calls that must fail with -EINVAL on the host (no GPU
 * needed: the pointers are never dereferenced). Plain C99. */
#include <math.h>
#include <stddef.h>
#include <stdio.h>
#include "nconv.h"

#define T nconv_voxel_merge_desc
#define F(f) printf("\"nconv_voxel_merge_args.%s\": [%zu, %zu],\n", #f, offsetof(T, f), sizeof(((T*)0)->f))

static struct nconv_voxel_merge_args good(void) {
    struct nconv_voxel_merge_args d = {0};
    d.n_points = 1000;
    d.xyz = (const float*)0x1000000; d.xyz_row_stride = 3;
    d.rgb = (const unsigned char*)0x2000000; d.rgb_row_stride = 3;
    d.normals = (const float*)0x3000000; d.normals_row_stride = 3;
    d.weights = (const int*)0x4000000;
    d.offsets = (const int*)0x5000000;
    d.poses = (const float*)0x6000000;
    d.n_segments = 2;
    d.nx = 100; d.ny = 80; d.nz = 20;
    d.voxel = 0.1f;
    d.max_voxels = 500;
    d.out_xyz = (float*)0x7000000; d.out_rgb = (unsigned char*)0x7100000; d.out_normals = (float*)0x7200000;
    d.out_count = (int*)0x7300000; d.out_key = (int*)0x7400000; d.stats = (int*)0x7500000;
    return d;
}

static void call(const char* name, const struct nconv_voxel_merge_args* d, void* ws, size_t bytes) {
    const int rc = nconv_voxel_merge(d, ws, bytes, NULL);
    printf("\"%s\": [%d, \"%s\"],\n", name, rc, nconv_last_error());
}

int main(void) {
    printf("{\n");
    printf("\"nconv_voxel_merge_args\": [0, %zu],\n", sizeof(T));
    F(n_points); F(xyz); F(xyz_row_stride); F(rgb); F(rgb_row_stride); F(normals); F(normals_row_stride);
    F(weights); F(offsets); F(poses); F(n_segments); F(nx); F(ny); F(nz); F(voxel); F(origin); F(max_voxels);
    F(out_xyz); F(out_rgb); F(out_normals); F(out_count); F(out_key); F(stats);

    void* ws = (void*)0x8000000;
    const size_t need = nconv_voxel_merge_workspace_bytes(1000, 100, 80, 20);
    printf("\"workspace_bytes\": [%zu, %zu, %zu, %zu, %zu, %zu, %zu],\n",
           nconv_voxel_merge_workspace_bytes(0, 100, 80, 20), nconv_voxel_merge_workspace_bytes(1, 100, 80, 20),
           nconv_voxel_merge_workspace_bytes(255, 1, 1, 1), nconv_voxel_merge_workspace_bytes(256, 1, 1, 1),
           nconv_voxel_merge_workspace_bytes(257, 1, 1, 1), need,
           nconv_voxel_merge_workspace_bytes((1LL << 31) - 1, 1290, 1290, 1290));
    printf("\"workspace_refused\": [%zu, %zu, %zu, %zu, %zu],\n", nconv_voxel_merge_workspace_bytes(-1, 100, 80, 20),
           nconv_voxel_merge_workspace_bytes(1LL << 31, 100, 80, 20), nconv_voxel_merge_workspace_bytes(1000, 0, 80, 20),
           nconv_voxel_merge_workspace_bytes(1000, 100, -1, 20), nconv_voxel_merge_workspace_bytes(1000, 2048, 1024, 1024));
    struct nconv_voxel_merge_args d;

    call("rc_null_descriptor", NULL, ws, need);
    d = good(); d.n_points = -1; call("rc_n_points_negative", &d, ws, need);
    d = good(); d.n_points = 1LL << 31; call("rc_n_points_large", &d, ws, (size_t)1 << 40);
    d = good(); d.max_voxels = -1; call("rc_max_voxels_negative", &d, ws, need);
    d = good(); d.max_voxels = 1LL << 31; call("rc_max_voxels_large", &d, ws, need);
    d = good(); d.stats = NULL; call("rc_null_stats", &d, ws, need);
    d = good(); d.xyz = NULL; call("rc_null_xyz", &d, ws, need);
    d = good(); d.xyz_row_stride = 2; call("rc_xyz_row_stride", &d, ws, need);
    d = good(); d.xyz_row_stride = -3; call("rc_xyz_row_stride_negative", &d, ws, need);
    d = good(); d.rgb_row_stride = 2; call("rc_rgb_row_stride", &d, ws, need);
    d = good(); d.normals_row_stride = 0; call("rc_normals_row_stride", &d, ws, need);
    d = good(); d.n_segments = 0; call("rc_n_segments", &d, ws, need);
    d = good(); d.offsets = NULL; call("rc_segments_without_offsets", &d, ws, need);
    d = good(); d.nx = 0; call("rc_nx", &d, ws, need);
    d = good(); d.ny = -4; call("rc_ny", &d, ws, need);
    d = good(); d.nz = 0; call("rc_nz", &d, ws, need);
    d = good(); d.nx = 2048; d.ny = 1024; d.nz = 1024; call("rc_cells", &d, ws, need);
    d = good(); d.nx = 65536; d.ny = 65536; d.nz = 65536; call("rc_cells_wrap", &d, ws, need);
    d = good(); d.voxel = 0.0f; call("rc_voxel_zero", &d, ws, need);
    d = good(); d.voxel = -0.1f; call("rc_voxel_negative", &d, ws, need);
    d = good(); d.voxel = NAN; call("rc_voxel_nan", &d, ws, need);
    d = good(); d.voxel = INFINITY; call("rc_voxel_inf", &d, ws, need);
    d = good(); d.origin[1] = NAN; call("rc_origin_nan", &d, ws, need);
    d = good(); d.origin[2] = -INFINITY; call("rc_origin_inf", &d, ws, need);
    d = good(); d.xyz = (const float*)0x1000002; call("rc_xyz_misaligned", &d, ws, need);
    d = good(); d.normals = (const float*)0x3000001; call("rc_normals_misaligned", &d, ws, need);
    d = good(); d.weights = (const int*)0x4000002; call("rc_weights_misaligned", &d, ws, need);
    d = good(); d.offsets = (const int*)0x5000002; call("rc_offsets_misaligned", &d, ws, need);
    d = good(); d.poses = (const float*)0x6000002; call("rc_poses_misaligned", &d, ws, need);
    d = good(); d.stats = (int*)0x7500002; call("rc_stats_misaligned", &d, ws, need);
    d = good(); d.out_xyz = NULL; call("rc_null_out_xyz", &d, ws, need);
    d = good(); d.out_count = NULL; call("rc_null_out_count", &d, ws, need);
    d = good(); d.out_key = NULL; call("rc_null_out_key", &d, ws, need);
    d = good(); d.out_rgb = NULL; call("rc_null_out_rgb", &d, ws, need);
    d = good(); d.out_normals = NULL; call("rc_null_out_normals", &d, ws, need);
    d = good(); d.out_xyz = (float*)0x7000002; call("rc_out_xyz_misaligned", &d, ws, need);
    d = good(); d.out_key = (int*)0x7400001; call("rc_out_key_misaligned", &d, ws, need);
    d = good(); call("rc_workspace_small", &d, ws, need - 1);
    d = good(); call("rc_workspace_null", &d, NULL, need);
    d = good(); call("rc_workspace_misaligned", &d, (void*)0x8000004, need);
    printf("\"abi\": [%d, %d]\n}\n", nconv_abi_version(), NCONV_ABI_VERSION);
    return 0;
}
