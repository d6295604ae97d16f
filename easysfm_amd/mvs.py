"""Dense reconstruction over the C ABI (include/esfm.h, "Dense reconstruction"; the reference README's TODO "add multi-view
stereo dense reconstruction"): plane-sweep depth maps with windowed NCC and their geometric-consistency fusion into a
coloured point cloud.  ``esfm_mvs_plan`` (view selection, depth range) is host code in the library; the sweep and the fusion
run on the GPU.  ``dense_reconstruct`` takes what the pipeline holds after its final bundle adjustment: the frames (pose,
K, undistorted image, track ids), which of them are registered, and the sparse cloud with its track ids."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np

from ._lib import Context, MVSNormalOptions, MVSOptions, check, default_context, lib
from .cloud import voxel_merge
from .types import Frame, SparsePointCloud


def default_mvs_options() -> MVSOptions:
    """esfm_mvs_options_default: 128 planes, 7 x 7 window, 4 neighbours, best 2 costs, ..."""
    opt = MVSOptions()
    lib().esfm_mvs_options_default(C.byref(opt))
    return opt


def default_mvs_normal_options() -> MVSNormalOptions:
    """esfm_mvs_normal_options_default: 7 x 7 window, at least 25 taps within 5 % of the centre's inverse depth."""
    opt = MVSNormalOptions()
    lib().esfm_mvs_normal_options_default(C.byref(opt))
    return opt


def _ptr(a: np.ndarray) -> C.c_void_p:
    return C.c_void_p(a.ctypes.data)


def plan_arrays(registered, poses, xyz, obs_offsets, obs_points, opt: Optional[MVSOptions] = None) -> Tuple[np.ndarray, np.ndarray]:
    """esfm_mvs_plan on plain arrays.  registered [n] bool, poses [n, 12] (or [n, 3, 4] / [n, 4, 4]) float32 world-to-camera,
    xyz [m, 3] float32, obs_offsets [n + 1] / obs_points: CSR of the cloud points each view observes.
    Returns (neighbours [n, max_neighbours] int32, -1 padded; depth_range [n, 2] float32, (0, 0) = no depth map)."""
    opt = opt or default_mvs_options()
    reg = np.ascontiguousarray(np.asarray(registered, bool).astype(np.uint8))
    n = len(reg)
    P = np.ascontiguousarray(np.asarray(poses, np.float32).reshape(n, -1, 4)[:, :3, :].reshape(n, 12))
    X = np.ascontiguousarray(np.asarray(xyz, np.float32).reshape(-1, 3))
    off = np.ascontiguousarray(obs_offsets, np.int32)
    pts = np.ascontiguousarray(obs_points, np.int32)
    if len(off) != n + 1:
        raise ValueError("obs_offsets must have n_views + 1 entries")
    nb = np.zeros((n, opt.max_neighbours), np.int32)
    rng = np.zeros((n, 2), np.float32)
    check(lib().esfm_mvs_plan(n, _ptr(reg), _ptr(P), len(X), _ptr(X) if len(X) else None, _ptr(off), _ptr(pts) if len(pts) else None,
                              C.byref(opt), _ptr(nb), _ptr(rng)))
    return nb, rng


def observations(frames: Sequence[Frame], cloud: SparsePointCloud) -> Tuple[np.ndarray, np.ndarray]:
    """CSR of the cloud points each frame observes: the points whose track id is among the frame's unique_pixel_ids."""
    ids = np.asarray(cloud.unique_point_ids, np.int64)
    rows = [np.nonzero(np.isin(ids, np.asarray(f.unique_pixel_ids, np.int64)))[0].astype(np.int32) for f in frames]
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    pts = np.concatenate(rows).astype(np.int32) if rows else np.zeros(0, np.int32)
    return off, pts


def mvs_plan(frames: Sequence[Frame], process_frame_id: Sequence[bool], cloud: SparsePointCloud,
             opt: Optional[MVSOptions] = None) -> Tuple[np.ndarray, np.ndarray]:
    """Neighbours and depth range of every frame.  process_frame_id as in BundleAdjustment.doSFMBA: False = registered."""
    if len(process_frame_id) != len(frames):
        raise ValueError("process_frame_id must have one entry per frame")
    off, pts = observations(frames, cloud)
    poses = np.stack([np.asarray(f.pose_cam, np.float32)[:3, :4] for f in frames])
    registered = ~np.asarray(process_frame_id, bool)
    return plan_arrays(registered, poses, cloud.xyz, off, pts, opt)


def _views(images, K4, poses):
    imgs = np.ascontiguousarray(images, np.uint8)
    if imgs.ndim == 3:
        imgs = imgs[..., None]
    if imgs.ndim != 4 or imgs.shape[3] not in (1, 3):
        raise ValueError("images must be [n_views, rows, cols] or [n_views, rows, cols, 1 | 3] uint8")
    n = imgs.shape[0]
    K = np.ascontiguousarray(np.asarray(K4, np.float32).reshape(n, 4))
    P = np.ascontiguousarray(np.asarray(poses, np.float32).reshape(n, -1, 4)[:, :3, :].reshape(n, 12))
    return imgs, K, P


def mvs_depth_maps(images, K4, poses, neighbours, depth_range, opt: Optional[MVSOptions] = None,
                   ctx: Optional[Context] = None) -> Tuple[np.ndarray, np.ndarray]:
    """esfm_mvs_depth_maps.  images [n, rows, cols(, 1 | 3)] uint8 (BGR or grey), K4 [n, 4] = (fx, cx, fy, cy), poses [n, 12]
    (or [n, 3 | 4, 4]) world-to-camera, neighbours [n, max_neighbours] int32 (-1 = none), depth_range [n, 2].
    Returns (depth [n, rows, cols] float32, 0 = no estimate; cost [n, rows, cols] float32, +inf = no valid plane)."""
    opt = opt or default_mvs_options()
    ctx = ctx or default_context()
    imgs, K, P = _views(images, K4, poses)
    n, rows, cols, ch = imgs.shape
    nb = np.ascontiguousarray(np.asarray(neighbours, np.int32).reshape(n, opt.max_neighbours))
    rng = np.ascontiguousarray(np.asarray(depth_range, np.float32).reshape(n, 2))
    depth = np.zeros((n, rows, cols), np.float32)
    cost = np.zeros((n, rows, cols), np.float32)
    check(lib().esfm_mvs_depth_maps(ctx.handle, n, rows, cols, ch, _ptr(imgs), _ptr(K), _ptr(P), _ptr(nb), _ptr(rng), C.byref(opt),
                                    _ptr(depth), _ptr(cost)))
    return depth, cost


def mvs_fuse(images, K4, poses, neighbours, depth, opt: Optional[MVSOptions] = None,
             ctx: Optional[Context] = None, return_index: bool = False):
    """esfm_mvs_fuse.  Returns (xyz [N, 3] float32, rgb [N, 3] uint8), ordered by (view, row, col); with return_index
    (esfm_mvs_fuse_ex) also pixel_index [N] int32 = (view rows + y) cols + x of each point."""
    opt = opt or default_mvs_options()
    ctx = ctx or default_context()
    imgs, K, P = _views(images, K4, poses)
    n, rows, cols, ch = imgs.shape
    nb = np.ascontiguousarray(np.asarray(neighbours, np.int32).reshape(n, opt.max_neighbours))
    d = np.ascontiguousarray(np.asarray(depth, np.float32).reshape(n, rows, cols))
    cap = n * rows * cols
    xyz = np.zeros((cap, 3), np.float32)
    rgb = np.zeros((cap, 3), np.uint8)
    cnt = C.c_int32(0)
    if not return_index:
        check(lib().esfm_mvs_fuse(ctx.handle, n, rows, cols, ch, _ptr(imgs), _ptr(K), _ptr(P), _ptr(nb), _ptr(d), C.byref(opt),
                                  _ptr(xyz), _ptr(rgb), C.byref(cnt)))
        return xyz[:cnt.value].copy(), rgb[:cnt.value].copy()
    index = np.zeros(cap, np.int32)
    check(lib().esfm_mvs_fuse_ex(ctx.handle, n, rows, cols, ch, _ptr(imgs), _ptr(K), _ptr(P), _ptr(nb), _ptr(d), C.byref(opt),
                                 _ptr(xyz), _ptr(rgb), _ptr(index), C.byref(cnt)))
    return xyz[:cnt.value].copy(), rgb[:cnt.value].copy(), index[:cnt.value].copy()


def mvs_normals(K4, poses, depth, opt: Optional[MVSNormalOptions] = None, ctx: Optional[Context] = None) -> np.ndarray:
    """esfm_mvs_normals.  depth [n, rows, cols] float32 (0 = no estimate), K4 [n, 4], poses [n, 12] (or [n, 3 | 4, 4]).
    Returns world normals [n, rows, cols, 3] float32 facing their camera; (0, 0, 0) = no normal."""
    opt = opt or default_mvs_normal_options()
    ctx = ctx or default_context()
    d = np.ascontiguousarray(depth, np.float32)
    if d.ndim != 3:
        raise ValueError("depth must be [n_views, rows, cols]")
    n, rows, cols = d.shape
    K = np.ascontiguousarray(np.asarray(K4, np.float32).reshape(n, 4))
    P = np.ascontiguousarray(np.asarray(poses, np.float32).reshape(n, -1, 4)[:, :3, :].reshape(n, 12))
    out = np.zeros((n, rows, cols, 3), np.float32)
    check(lib().esfm_mvs_normals(ctx.handle, n, rows, cols, _ptr(K), _ptr(P), _ptr(d), C.byref(opt), _ptr(out)))
    return out


def frame_arrays(frames: Sequence[Frame], process_frame_id: Sequence[bool]):
    """(images [n, rows, cols, ch], K4 [n, 4], poses [n, 12]) of the frames; a registered frame without an image is a
    ValueError, an unregistered one contributes zeros (it is never a reference or a source)."""
    reg = ~np.asarray(process_frame_id, bool)
    shapes = {np.asarray(f.rgb_image).shape for f, r in zip(frames, reg) if r and f.rgb_image is not None}
    for i, (f, r) in enumerate(zip(frames, reg)):
        if r and f.rgb_image is None:
            raise ValueError(f"registered frame {i} has no image")
    if len(shapes) != 1:
        raise ValueError(f"registered frames need one image size, got {sorted(shapes)}")
    shape = shapes.pop()
    ch = 1 if len(shape) == 2 else shape[2]
    rows, cols = shape[:2]
    imgs = np.zeros((len(frames), rows, cols, ch), np.uint8)
    for i, (f, r) in enumerate(zip(frames, reg)):
        if r:
            imgs[i] = np.asarray(f.rgb_image, np.uint8).reshape(rows, cols, ch)
    K4 = np.array([[f.K_cam[0, 0], f.K_cam[0, 2], f.K_cam[1, 1], f.K_cam[1, 2]] for f in frames], np.float32)
    poses = np.stack([np.asarray(f.pose_cam, np.float32)[:3, :4].reshape(12) for f in frames])
    return imgs, K4, poses


def dense_reconstruction(frames: Sequence[Frame], process_frame_id: Sequence[bool], cloud: SparsePointCloud,
                         opt: Optional[MVSOptions] = None, ctx: Optional[Context] = None):
    """dense_reconstruct with its intermediate results: (dense cloud, neighbours, depth_range, depth, cost)."""
    opt = opt or default_mvs_options()
    imgs, K4, poses = frame_arrays(frames, process_frame_id)
    ctx = ctx or default_context()
    nb, rng = mvs_plan(frames, process_frame_id, cloud, opt)
    depth, cost = mvs_depth_maps(imgs, K4, poses, nb, rng, opt, ctx)
    xyz, rgb = mvs_fuse(imgs, K4, poses, nb, depth, opt, ctx)
    return SparsePointCloud(xyz=xyz, rgb=rgb), nb, rng, depth, cost


def dense_reconstruct(frames: Sequence[Frame], process_frame_id: Sequence[bool], cloud: SparsePointCloud,
                      opt: Optional[MVSOptions] = None, ctx: Optional[Context] = None) -> SparsePointCloud:
    """Plan, depth maps and fusion for the registered frames (process_frame_id False) of a reconstruction; cloud is the
    sparse cloud with its track ids (before the SOR filter).  Returns the fused, coloured dense cloud."""
    return dense_reconstruction(frames, process_frame_id, cloud, opt, ctx)[0]


class MergeOptions:
    """Settings of dense_merge's voxel grid.  voxel_size > 0 is used as given; 0 derives it from the cloud: voxel_scale times the
    lower median of the points' pixel footprints depth / fx.  A voxel is kept with at least min_points members from at least
    min_tags views.  normals: esfm_mvs_normal_options, None = its defaults."""

    def __init__(self, voxel_size: float = 0.0, voxel_scale: float = 2.0, min_points: int = 1, min_tags: int = 2,
                 normals: Optional[MVSNormalOptions] = None):
        self.voxel_size, self.voxel_scale, self.min_points, self.min_tags, self.normals = voxel_size, voxel_scale, min_points, min_tags, normals


def merge_voxel_size(depth, K4, pixel_index, merge_opt: MergeOptions) -> np.float32:
    """The voxel size dense_merge uses: merge_opt.voxel_size if > 0, else (f32) voxel_scale * the lower median,
    sorted[(n - 1) // 2], of the f32 footprints depth[pixel_index] / fx_view."""
    if merge_opt.voxel_size > 0:
        return np.float32(merge_opt.voxel_size)
    d = np.asarray(depth, np.float32)
    idx = np.asarray(pixel_index, np.int64)
    if len(idx) == 0:
        raise ValueError("no points to derive a voxel size from")
    fx = np.asarray(K4, np.float32).reshape(len(d), 4)[idx // (d.shape[1] * d.shape[2]), 0]
    foot = np.sort(d.reshape(-1)[idx] / fx)
    return np.float32(np.float32(merge_opt.voxel_scale) * foot[(len(foot) - 1) // 2])


def dense_merge(frames: Sequence[Frame], process_frame_id: Sequence[bool], cloud: SparsePointCloud,
                opt: Optional[MVSOptions] = None, merge_opt: Optional[MergeOptions] = None, ctx: Optional[Context] = None):
    """Plan, depth maps, fusion with pixel indices, depth-map normals and the voxel merge: one point per occupied voxel with a
    normal, tagged by the views that saw it.  Returns (merged cloud, normals [M, 3] float32, count [M] int32 members,
    tagmask [M] uint64 with bit v set for view v, the unmerged dense cloud)."""
    if len(frames) > 64:
        raise ValueError("dense_merge tags points by view: at most 64 views")
    opt = opt or default_mvs_options()
    merge_opt = merge_opt or MergeOptions()
    ctx = ctx or default_context()
    imgs, K4, poses = frame_arrays(frames, process_frame_id)
    nb, rng = mvs_plan(frames, process_frame_id, cloud, opt)
    depth, _ = mvs_depth_maps(imgs, K4, poses, nb, rng, opt, ctx)
    return merge_arrays(imgs, K4, poses, nb, depth, opt, merge_opt, ctx)


def merge_arrays(imgs, K4, poses, nb, depth, opt: MVSOptions, merge_opt: MergeOptions, ctx: Context):
    """dense_merge behind the depth maps (plain arrays)."""
    if len(depth) > 64:
        raise ValueError("dense_merge tags points by view: at most 64 views")
    xyz, rgb, index = mvs_fuse(imgs, K4, poses, nb, depth, opt, ctx, return_index=True)
    dense = SparsePointCloud(xyz=xyz, rgb=rgb)
    if len(xyz) == 0:
        return SparsePointCloud(), np.zeros((0, 3), np.float32), np.zeros(0, np.int32), np.zeros(0, np.uint64), dense
    normals = mvs_normals(K4, poses, depth, merge_opt.normals, ctx).reshape(-1, 3)[index]
    tags = (index // (depth.shape[1] * depth.shape[2])).astype(np.int32)
    h = merge_voxel_size(depth, K4, index, merge_opt)
    m_xyz, m_rgb, m_nrm, count, mask = voxel_merge(xyz, rgb, normals, tags, float(h), merge_opt.min_points, merge_opt.min_tags, ctx)
    return SparsePointCloud(xyz=m_xyz, rgb=m_rgb), m_nrm, count, mask, dense
