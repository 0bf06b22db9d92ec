"""Per-frame point clouds merged into one voxel-grid map, on the device.

backproject gives one cloud per frame and estimate_pose the camera's motion; this is the step that
puts the frames of a drive into one map without keeping every duplicate of the same road:

  voxel_merge   points (one cloud, or several with `offsets` and one pose each) -> a VoxelMap: one
                point per occupied cell of a stated box of cubic cells, the weighted mean of the
                points that fell into it, with the mean colour and normal, in ascending cell number
                (nconv_voxel_merge, csrc/voxel_merge.hip)
  VoxelMerger   the same with its outputs and workspace kept, for torch.cuda.graph
  VoxelMap.add  a further cloud merged into an existing map

The rule is stated operation by operation in include/nconv.h (nconv_voxel_merge): the point goes to
the world by its segment's [R | t], its cell is floorf((p - origin) / voxel) per axis, the inside
points are sorted stably by cell number, and the sums of each cell are taken in double in a fixed
tree over sorted positions. The same input gives the same bits on every run; 5 + 2 P launches with
P = ceil(bits(nx ny nz - 1) / 8), no host synchronisation, no atomics on floats. Device tensors only:
there is no PyTorch path.
"""
import ctypes
import math

import torch

from . import _views
from .pointcloud import PointCloud

_PREFIX = "voxelmap"


def _rows3(x, what, dtype, n=None):
    """x as an (N, 3) tensor of dtype with a unit innermost stride; its row stride in elements."""
    _views.require_tensor(x, what, (dtype,), _PREFIX)
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"{_PREFIX}: {what} must be (N, 3), got {tuple(x.shape)}")
    if n is not None and x.shape[0] != n:
        raise ValueError(f"{_PREFIX}: {what} has {x.shape[0]} rows, xyz {n}")
    if x.shape[0] > 1 and (x.stride(1) != 1 or x.stride(0) < 3):
        raise ValueError(f"{_PREFIX}: {what} of strides {x.stride()} has no unit innermost stride with rows at "
                         "least 3 apart")
    if x.shape[0] == 1 and x.stride(1) != 1:
        raise ValueError(f"{_PREFIX}: {what} of strides {x.stride()} has no unit innermost stride")
    return x.stride(0) if x.shape[0] > 1 else 3


def _grid(voxel, origin, dims):
    voxel = float(voxel)
    if not (voxel > 0.0 and math.isfinite(voxel)):
        raise ValueError(f"{_PREFIX}: voxel = {voxel} must be > 0 and finite")
    origin = tuple(float(v) for v in origin)
    if len(origin) != 3 or not all(math.isfinite(v) for v in origin):
        raise ValueError(f"{_PREFIX}: origin must be three finite values, got {origin}")
    dims = tuple(int(v) for v in dims)
    if len(dims) != 3 or min(dims) < 1:
        raise ValueError(f"{_PREFIX}: dims must be three values >= 1, got {dims}")
    if dims[0] * dims[1] * dims[2] >= 2 ** 31:
        raise ValueError(f"{_PREFIX}: dims = {dims} has nx * ny * nz >= 2^31 cells")
    return voxel, origin, dims


def launches(dims):
    """The kernel launches of one merge on a grid of dims cells: 5 + 2 ceil(bits(nx ny nz - 1) / 8)."""
    cells = int(dims[0]) * int(dims[1]) * int(dims[2])
    return 5 + 2 * -(-(cells - 1).bit_length() // 8)


def workspace_bytes(n_points, dims):
    """Bytes of the workspace of a merge of n_points rows (nconv_voxel_merge_workspace_bytes)."""
    from . import _lib
    n = _lib.lib().nconv_voxel_merge_workspace_bytes(int(n_points), int(dims[0]), int(dims[1]), int(dims[2]))
    if n == 0:
        raise ValueError(f"{_PREFIX}: n_points = {n_points} with dims = {tuple(dims)} is too large "
                         "(n_points < 2^31, 1 <= nx * ny * nz < 2^31)")
    return n


class VoxelMap:
    """The result of voxel_merge: device tensors at full capacity. xyz (capacity, 3) fp32 the mean
    point of every occupied cell; rgb (capacity, 3) uint8 or None; normals (capacity, 3) fp32 unit
    mean normals, (0, 0, 0) where a cell has none, or None; count (capacity) int32 the cell's summed
    weight (saturating); key (capacity) int32 the cell number (iz * ny + iy) * nx + ix, ascending;
    stats (4) int32 {n_voxels, n_inside, n_dropped, 0}. Rows from min(n_voxels, capacity) on are not
    written. voxel, origin, dims: the grid. Building one does not synchronise; n_voxels(), truncated()
    and points() read stats on the host (once)."""

    def __init__(self, xyz, rgb, normals, count, key, stats, voxel, origin, dims):
        self.xyz, self.rgb, self.normals, self.count, self.key, self.stats = xyz, rgb, normals, count, key, stats
        self.voxel, self.origin, self.dims = voxel, origin, dims
        self._host = None

    @property
    def capacity(self):
        return self.xyz.shape[0]

    def host_stats(self):
        """stats as a list of ints: the one host read (a synchronisation), then cached."""
        if self._host is None:
            self._host = self.stats.cpu().tolist()
        return self._host

    def n_voxels(self):
        """The true number of occupied cells (may exceed the capacity)."""
        return self.host_stats()[0]

    def truncated(self):
        return self.n_voxels() > self.capacity

    def points(self):
        """(xyz, rgb, normals) rows of the occupied cells (what the capacity kept of them), e.g. for write_ply."""
        n = min(self.n_voxels(), self.capacity)
        return (self.xyz[:n], None if self.rgb is None else self.rgb[:n],
                None if self.normals is None else self.normals[:n])

    def add(self, pc, poses=None, *, weights=None, max_voxels=None, out=None):
        """This map and a further cloud merged on the same grid: a new VoxelMap. The map's rows form a
        first segment with the identity pose and weights = count (rows past n_voxels get weight 0 and
        are counted in n_dropped); the cloud's segments follow with `poses` ((S, 3, 4), None:
        identity) and `weights` ((N) int32, None: 1). pc: a PointCloud, or an (N, 3) tensor as one
        segment; it must carry rgb / normals iff the map does. This is two applications of the rule,
        not one merge of everything: the stored means were rounded to fp32 in between, so the result
        is close to, not bit-equal to, voxel_merge of all the clouds at once. No host synchronisation, but the joined rows, weights
        and offsets are new tensors (torch.cat, arange, where): unlike VoxelMerger, add allocates and
        is not meant for capture."""
        if isinstance(pc, PointCloud):
            xyz, rgb, nrm, off = pc.xyz, pc.rgb, pc.normals, pc.offsets
        else:
            xyz, rgb, nrm, off = pc, None, None, None
        _rows3(xyz, "xyz", torch.float32)
        n = xyz.shape[0]
        if (rgb is None) != (self.rgb is None) or (nrm is None) != (self.normals is None):
            raise ValueError(f"{_PREFIX}: add needs a cloud with rgb and normals exactly where the map has them")
        dev, cap = self.xyz.device, self.capacity
        if off is None:
            off = torch.tensor([0, n], dtype=torch.int32, device=dev)
        S = off.numel() - 1
        rows = torch.arange(cap, dtype=torch.int32, device=dev)
        w_map = torch.where(rows < self.stats[0], self.count, torch.zeros_like(self.count))
        if weights is None:
            weights = torch.ones(n, dtype=torch.int32, device=dev)
        _views.require_tensor(weights, "weights", (torch.int32,), _PREFIX)
        if tuple(weights.shape) != (n,):
            raise ValueError(f"{_PREFIX}: weights must be ({n},), got {tuple(weights.shape)}")
        weights = torch.cat([w_map, weights])
        offsets = torch.cat([torch.zeros(1, dtype=torch.int32, device=dev), off.to(torch.int32) + cap])
        if poses is not None:
            _check_poses(poses, S)
            eye = torch.eye(3, 4, dtype=torch.float32, device=dev)[None]
            poses = torch.cat([eye, poses.reshape(S, 3, 4)])
        return voxel_merge(torch.cat([self.xyz, xyz]), offsets, poses, voxel=self.voxel, origin=self.origin,
                           dims=self.dims, rgb=None if rgb is None else torch.cat([self.rgb, rgb]),
                           normals=None if nrm is None else torch.cat([self.normals, nrm]), weights=weights,
                           max_voxels=max_voxels, out=out)


def _check_poses(poses, S):
    _views.require_tensor(poses, "poses", (torch.float32,), _PREFIX)
    if tuple(poses.shape) not in ((S, 3, 4),) + (((3, 4),) if S == 1 else ()):
        raise ValueError(f"{_PREFIX}: poses must be ({S}, 3, 4), one [R | t] per segment, got {tuple(poses.shape)}")
    if not poses.is_contiguous():
        raise ValueError(f"{_PREFIX}: poses of strides {poses.stride()} is not contiguous")


def voxel_merge(xyz, offsets=None, poses=None, *, voxel, origin, dims, rgb=None, normals=None, weights=None,
                max_voxels=None, out=None):
    """The points merged into a VoxelMap: one row per occupied cell of the box that starts at
    `origin` and has dims = (nx, ny, nz) cubic cells of edge `voxel` (1 <= nx ny nz < 2^31).
    xyz: (N, 3) fp32 device rows with a unit innermost stride, or a PointCloud, which then supplies
    offsets, rgb and normals. offsets: (S + 1) int32, non-decreasing, PointCloud.offsets' convention:
    rows [offsets[s], min(offsets[s + 1], N)) are segment s, rows at or beyond offsets[S] belong to no
    segment and are dropped; None: one segment. poses: (S, 3, 4) fp32 [R | t] from the segment's camera
    frame to the world (the inverse of what estimate_pose chains: inverse_pose); None: identity.
    rgb (N, 3) uint8, normals (N, 3) fp32 with (0, 0, 0) = none, weights (N) int32 (default 1): per
    point. A point outside the box, with a NaN or infinite coordinate, or with a weight <= 0 (negative
    weights included: they cannot be refused without reading the device) is dropped and counted in
    stats[2]. max_voxels: the capacity of the outputs (default min(N, nx ny nz)); cells beyond it are
    dropped and VoxelMap.truncated() tells. out: an optional dict of preallocated contiguous buffers
    'xyz', 'rgb', 'normals', 'count', 'key', 'stats', 'workspace' (uint8, workspace_bytes(N, dims)) --
    static buffers under hipGraph capture. launches(dims) launches, no allocation when out is complete,
    no host synchronisation."""
    from . import _lib
    if isinstance(xyz, PointCloud):
        if offsets is not None or rgb is not None or normals is not None:
            raise ValueError(f"{_PREFIX}: a PointCloud supplies offsets, rgb and normals itself")
        xyz, offsets, rgb, normals = xyz.xyz, xyz.offsets, xyz.rgb, xyz.normals
    voxel, origin, dims = _grid(voxel, origin, dims)
    xs = _rows3(xyz, "xyz", torch.float32)
    N = xyz.shape[0]
    cs = _rows3(rgb, "rgb", torch.uint8, N) if rgb is not None else 0
    ns = _rows3(normals, "normals", torch.float32, N) if normals is not None else 0
    if weights is not None:
        _views.require_tensor(weights, "weights", (torch.int32,), _PREFIX)
        if tuple(weights.shape) != (N,) or not weights.is_contiguous():
            raise ValueError(f"{_PREFIX}: weights must be a contiguous ({N},) tensor, got {tuple(weights.shape)} "
                             f"of strides {weights.stride()}")
    S = 1
    if offsets is not None:
        _views.require_tensor(offsets, "offsets", (torch.int32,), _PREFIX)
        if offsets.dim() != 1 or offsets.numel() < 2 or not offsets.is_contiguous():
            raise ValueError(f"{_PREFIX}: offsets must be a contiguous (S + 1,) tensor with S >= 1, got "
                             f"{tuple(offsets.shape)}")
        S = offsets.numel() - 1
    if poses is not None:
        _check_poses(poses, S)
    cap = min(N, dims[0] * dims[1] * dims[2]) if max_voxels is None else int(max_voxels)
    if cap < 0 or cap >= 2 ** 31:
        raise ValueError(f"{_PREFIX}: max_voxels = {max_voxels} must be in [0, 2^31)")
    dev = xyz.device
    for t, what in ((xyz, "xyz"), (rgb, "rgb"), (normals, "normals"), (weights, "weights"), (offsets, "offsets"),
                    (poses, "poses")):
        if t is None:
            continue
        _views.on_device(t, what, _PREFIX, "the merge is computed by libnconv")
        if t.device != dev:
            raise RuntimeError(f"{_PREFIX}: {what} on {t.device}, xyz on {dev}")
    o_xyz = _views.output(out, "xyz", (cap, 3), torch.float32, dev, _PREFIX, "points")
    o_rgb = _views.output(out, "rgb", (cap, 3), torch.uint8, dev, _PREFIX, "points") if rgb is not None else None
    o_nrm = _views.output(out, "normals", (cap, 3), torch.float32, dev, _PREFIX, "points") if normals is not None else None
    o_cnt = _views.output(out, "count", (cap,), torch.int32, dev, _PREFIX, "points")
    o_key = _views.output(out, "key", (cap,), torch.int32, dev, _PREFIX, "points")
    stats = _views.output(out, "stats", (4,), torch.int32, dev, _PREFIX, "points")
    nws = workspace_bytes(N, dims)
    ws = None if out is None else out.get("workspace")
    if ws is None:
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    elif not (torch.is_tensor(ws) and ws.dtype == torch.uint8 and ws.dim() == 1 and ws.is_contiguous()
              and ws.numel() >= nws and ws.device == dev):
        raise TypeError(f"{_PREFIX}: out['workspace'] must be a contiguous uint8 tensor of at least {nws} bytes on {dev}")
    d = _lib.NconvVoxelMerge()
    d.n_points, d.xyz, d.xyz_row_stride = N, xyz.data_ptr() if N else None, xs
    if rgb is not None:
        d.rgb, d.rgb_row_stride = rgb.data_ptr() if N else None, cs
    if normals is not None:
        d.normals, d.normals_row_stride = normals.data_ptr() if N else None, ns
    d.weights = weights.data_ptr() if weights is not None and N else None
    d.offsets = None if offsets is None else offsets.data_ptr()
    d.poses = None if poses is None else poses.data_ptr()
    d.n_segments = S
    d.nx, d.ny, d.nz = dims
    d.voxel = voxel
    d.origin[0], d.origin[1], d.origin[2] = origin
    d.max_voxels = cap
    if cap:  # at capacity 0 nothing but stats is written (an empty tensor has no storage to point at)
        d.out_xyz, d.out_count, d.out_key = o_xyz.data_ptr(), o_cnt.data_ptr(), o_key.data_ptr()
        d.out_rgb = None if o_rgb is None else o_rgb.data_ptr()
        d.out_normals = None if o_nrm is None else o_nrm.data_ptr()
    d.stats = stats.data_ptr()
    rc = _lib.lib().nconv_voxel_merge(ctypes.byref(d), _lib.ptr(ws), ws.numel(), _lib.stream_handle(dev))
    _lib.check(rc, "nconv_voxel_merge")
    return VoxelMap(o_xyz, o_rgb, o_nrm, o_cnt, o_key, stats, voxel, origin, dims)


class VoxelMerger:
    """voxel_merge with its outputs and workspace allocated once, for clouds of at most max_points
    rows on one grid: a call allocates nothing and can be captured with torch.cuda.graph (keep the
    input tensors static and refill them). rgb / normals: whether the clouds carry them. The returned
    VoxelMap shares the merger's buffers: the next call overwrites it."""

    def __init__(self, max_points, dims, *, voxel, origin, max_voxels=None, rgb=False, normals=False, device="cuda"):
        self.voxel, self.origin, self.dims = _grid(voxel, origin, dims)
        self.max_points = int(max_points)
        if self.max_points < 0:
            raise ValueError(f"{_PREFIX}: max_points = {max_points} is negative")
        cap = min(self.max_points, dims[0] * dims[1] * dims[2]) if max_voxels is None else int(max_voxels)
        dev = torch.device(device)
        self.max_voxels = cap
        self.out = {"xyz": torch.empty((cap, 3), dtype=torch.float32, device=dev),
                    "count": torch.empty((cap,), dtype=torch.int32, device=dev),
                    "key": torch.empty((cap,), dtype=torch.int32, device=dev),
                    "stats": torch.empty((4,), dtype=torch.int32, device=dev),
                    "workspace": torch.empty(workspace_bytes(self.max_points, self.dims), dtype=torch.uint8, device=dev)}
        if rgb:
            self.out["rgb"] = torch.empty((cap, 3), dtype=torch.uint8, device=dev)
        if normals:
            self.out["normals"] = torch.empty((cap, 3), dtype=torch.float32, device=dev)

    def __call__(self, xyz, offsets=None, poses=None, *, rgb=None, normals=None, weights=None):
        n = xyz.capacity if isinstance(xyz, PointCloud) else (xyz.shape[0] if torch.is_tensor(xyz) else 0)
        if n > self.max_points:
            raise ValueError(f"{_PREFIX}: {n} rows, the merger was built for at most {self.max_points}")
        return voxel_merge(xyz, offsets, poses, voxel=self.voxel, origin=self.origin, dims=self.dims, rgb=rgb,
                           normals=normals, weights=weights, max_voxels=self.max_voxels, out=self.out)
