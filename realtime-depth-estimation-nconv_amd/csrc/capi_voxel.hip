// capi_voxel.hip — the extern "C" entry points of the voxel-grid merge (nconv_voxel_merge and its workspace
// query). Host code only: it validates the descriptor, fills VoxelArgs (nconv_internal.h) and calls the launcher
// of voxel_merge.hip.
#include <cmath>
#include "capi_common.h"

using namespace nconv::capi;

// 1 <= nx ny nz < 2^31, every dimension positive
static bool dims_ok(int nx, int ny, int nz) {
    if (nx <= 0 || ny <= 0 || nz <= 0) return false;
    const long long xy = (long long)nx * ny;  // < 2^62
    return xy < (1LL << 31) && xy * nz < (1LL << 31);
}

extern "C" {

size_t nconv_voxel_merge_workspace_bytes(long long n_points, int nx, int ny, int nz) {
    if (n_points < 0 || n_points >= (1LL << 31) || !dims_ok(nx, ny, nz)) return 0;
    return nconv::voxel_merge_workspace_bytes(n_points);
}

int nconv_voxel_merge(const struct nconv_voxel_merge_args* d, void* workspace, size_t workspace_bytes,
                      void* stream) {
    const char* fn = "nconv_voxel_merge";
    if (!d) return fail(-22, fn, "null descriptor");
    if (d->n_points < 0 || d->n_points >= (1LL << 31)) return fail(-22, fn, "n_points must be in [0, 2^31)");
    if (d->max_voxels < 0 || d->max_voxels >= (1LL << 31)) return fail(-22, fn, "max_voxels must be in [0, 2^31)");
    if (!d->stats) return fail(-22, fn, "null stats");
    if (d->n_points > 0 && !d->xyz) return fail(-22, fn, "null xyz");
    if (d->xyz_row_stride < 3) return fail(-22, fn, "xyz: row stride smaller than 3");
    if (d->rgb && d->rgb_row_stride < 3) return fail(-22, fn, "rgb: row stride smaller than 3");
    if (d->normals && d->normals_row_stride < 3) return fail(-22, fn, "normals: row stride smaller than 3");
    if (d->n_segments < 1) return fail(-22, fn, "n_segments must be >= 1");
    if (!d->offsets && d->n_segments != 1) return fail(-22, fn, "n_segments must be 1 without offsets");
    if (!dims_ok(d->nx, d->ny, d->nz)) return fail(-22, fn, "dims: every dimension >= 1 and nx * ny * nz < 2^31");
    if (!(d->voxel > 0.f) || !std::isfinite(d->voxel)) return fail(-22, fn, "voxel must be > 0 and finite");
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(d->origin[k])) return fail(-22, fn, "origin must be finite");
    if ((size_t)d->xyz % 4 || (size_t)d->normals % 4 || (size_t)d->weights % 4 || (size_t)d->offsets % 4 ||
        (size_t)d->poses % 4 || (size_t)d->stats % 4)
        return fail(-22, fn, "xyz / normals / weights / offsets / poses / stats not 4-byte aligned");
    if (d->max_voxels > 0) {
        if (!d->out_xyz || !d->out_count || !d->out_key) return fail(-22, fn, "null out_xyz, out_count or out_key");
        if (d->rgb && !d->out_rgb) return fail(-22, fn, "null out_rgb with rgb");
        if (d->normals && !d->out_normals) return fail(-22, fn, "null out_normals with normals");
        if ((size_t)d->out_xyz % 4 || (size_t)d->out_normals % 4 || (size_t)d->out_count % 4 || (size_t)d->out_key % 4)
            return fail(-22, fn, "out_xyz / out_normals / out_count / out_key not 4-byte aligned");
    }
    if (!workspace || workspace_bytes < nconv::voxel_merge_workspace_bytes(d->n_points))
        return fail(-22, fn, "workspace too small");
    if ((size_t)workspace % 8) return fail(-22, fn, "workspace not 8-byte aligned");
    nconv::VoxelArgs a{};
    a.N = d->n_points;
    a.xyz = d->xyz, a.xs = d->xyz_row_stride;
    a.rgb = d->rgb, a.cs = d->rgb_row_stride;
    a.nrm = d->normals, a.ns = d->normals_row_stride;
    a.w = d->weights, a.offsets = d->offsets, a.poses = d->poses;
    a.S = d->n_segments, a.nx = d->nx, a.ny = d->ny, a.nz = d->nz;
    a.voxel = d->voxel, a.ox = d->origin[0], a.oy = d->origin[1], a.oz = d->origin[2];
    a.cap = d->max_voxels;
    a.oxyz = d->out_xyz, a.orgb = d->out_rgb, a.onrm = d->out_normals;
    a.ocount = d->out_count, a.okey = d->out_key, a.stats = d->stats;
    return launched(fn, nconv::launch_voxel_merge, a, workspace, (hipStream_t)stream);
}

}  // extern "C"
