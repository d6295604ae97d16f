"""Robust multi-view track triangulation and the reprojection filter (include/esfm.h "Track triangulation").

``track_triangulate`` re-estimates every point from all the observations of its track (two-ray midpoint hypotheses scored by
inlier count and truncated cost, a Gauss-Newton refit on the winner's inliers) and judges it by reprojection error, depth sign
and triangulation angle; ``track_evaluate`` judges given points the same way without re-estimating them.  Both run on the GPU;
``host=True`` runs the same arithmetic compiled for the CPU (no GPU needed).  ``refine_tracks`` applies them to a reconstruction
in progress.  The defaults -- 4 px, 1.5 degrees -- are the common conventions of incremental SfM and have not been measured on
this project's data."""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional, Sequence

import numpy as np

from ._lib import Context, TrackOptionsStruct, check, default_context, lib
from .types import Frame, SparsePointCloud

STATUS_KEPT, STATUS_TOO_FEW, STATUS_NO_HYPOTHESIS, STATUS_FEW_INLIERS, STATUS_SMALL_ANGLE, STATUS_NON_FINITE = range(6)


class TrackOptions:
    """esfm_track_options.  cos_min_angle, what the verdict compares against, follows min_angle_deg."""

    def __init__(self, max_reproj_error_px: float = 4.0, min_angle_deg: float = 1.5, min_views: int = 2, max_hypotheses: int = 64,
                 refine_iterations: int = 5):
        self.max_reproj_error_px = float(max_reproj_error_px)
        self.min_angle_deg = float(min_angle_deg)
        self.min_views = int(min_views)
        self.max_hypotheses = int(max_hypotheses)
        self.refine_iterations = int(refine_iterations)

    @property
    def cos_min_angle(self) -> float:
        return math.cos(self.min_angle_deg * (3.14159265358979323846 / 180.0))

    def struct(self) -> TrackOptionsStruct:
        return TrackOptionsStruct(self.max_reproj_error_px, self.min_angle_deg, self.cos_min_angle, self.min_views, self.max_hypotheses,
                                  self.refine_iterations, 0)


class TrackResult(NamedTuple):
    xyz: Optional[np.ndarray]       # [n_pt, 3] float64 (None from track_evaluate)
    obs_inlier: np.ndarray          # [n_obs] bool
    obs_err2: np.ndarray            # [n_obs] float32, squared pixels
    status: np.ndarray              # [n_pt] int32, STATUS_*
    n_inliers: np.ndarray           # [n_pt] int32
    min_cos: np.ndarray             # [n_pt] float64
    mse: np.ndarray                 # [n_pt] float64


def _call(evaluate: bool, cam_idx, pt_idx, uv, K4, Rt, n_pt: int, xyz_in, options: Optional[TrackOptions], ctx: Optional[Context],
          host: bool) -> TrackResult:
    cam_idx = np.ascontiguousarray(cam_idx, np.int32).reshape(-1)
    pt_idx = np.ascontiguousarray(pt_idx, np.int32).reshape(-1)
    uv = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
    K4 = np.ascontiguousarray(K4, np.float32).reshape(-1, 4)
    Rt = np.ascontiguousarray(Rt, np.float64).reshape(-1, 12)
    n_obs, n_cam, n_pt = len(cam_idx), len(K4), int(n_pt)
    if len(pt_idx) != n_obs or len(uv) != n_obs or len(Rt) != n_cam:
        raise ValueError("cam_idx, pt_idx and uv need one row per observation, K4 and Rt one per camera")
    if xyz_in is not None:
        xyz_in = np.ascontiguousarray(xyz_in, np.float64).reshape(-1, 3)
        if len(xyz_in) != n_pt:
            raise ValueError("xyz_in needs one row per point")
    elif evaluate:
        raise ValueError("track_evaluate needs the points")
    opt = (options or TrackOptions()).struct()
    xyz = None if evaluate else np.zeros((n_pt, 3), np.float64)
    inl = np.zeros(n_obs, np.uint8); err2 = np.zeros(n_obs, np.float32)
    status = np.zeros(n_pt, np.int32); n_inl = np.zeros(n_pt, np.int32)
    min_cos = np.zeros(n_pt, np.float64); mse = np.zeros(n_pt, np.float64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None   # noqa: E731
    args = [n_cam, n_pt, n_obs, ptr(cam_idx), ptr(pt_idx), ptr(uv), ptr(K4), ptr(Rt), ptr(xyz_in), C.byref(opt)]
    if not evaluate:
        args.append(ptr(xyz))
    args += [ptr(inl), ptr(err2), ptr(status), ptr(n_inl), ptr(min_cos), ptr(mse)]
    L = lib()
    if host:
        check((L.esfm_track_evaluate_host if evaluate else L.esfm_track_triangulate_host)(*args))
    else:
        ctx = ctx or default_context()
        check((L.esfm_track_evaluate if evaluate else L.esfm_track_triangulate)(ctx.handle, *args))
    return TrackResult(xyz, inl.astype(bool), err2, status, n_inl, min_cos, mse)


def track_triangulate(cam_idx, pt_idx, uv, K4, Rt, n_pt: int, xyz_in=None, options: Optional[TrackOptions] = None,
                      ctx: Optional[Context] = None, host: bool = False) -> TrackResult:
    """esfm_track_triangulate (host=True: esfm_track_triangulate_host).  cam_idx, pt_idx, uv: bundle adjustment's observation
    arrays; K4 [n_cam, 4] = fx, cx, fy, cy; Rt [n_cam, 3, 4] world -> camera, float64.  A point that is not kept comes back as
    xyz_in's (zeros without xyz_in)."""
    return _call(False, cam_idx, pt_idx, uv, K4, Rt, n_pt, xyz_in, options, ctx, host)


def track_evaluate(cam_idx, pt_idx, uv, K4, Rt, xyz, options: Optional[TrackOptions] = None, ctx: Optional[Context] = None,
                   host: bool = False) -> TrackResult:
    """esfm_track_evaluate (host=True: esfm_track_evaluate_host): inliers, statistics and verdict of the given points; no
    hypotheses, no refit."""
    xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
    return _call(True, cam_idx, pt_idx, uv, K4, Rt, len(xyz), xyz, options, ctx, host)


def track_observations(frames: Sequence[Frame], todo: Sequence[bool], cloud: SparsePointCloud):
    """Every keypoint of a registered frame whose unique_pixel_ids is a cloud id -- a track's first observer included, which
    setBAProblem's unique_pixel_has_match gate drops -- camera-major, keypoint index ascending.  Returns (cam_idx, pt_idx, uv, K4,
    Rt, frame index per camera, keypoint index per observation)."""
    pid = np.asarray(cloud.unique_point_ids, np.int64)
    order = np.argsort(pid, kind="stable")
    pid_s = pid[order]
    cams, pts, uvs, kps, K4, Rt, frame_of = [], [], [], [], [], [], []
    for i, fr in enumerate(frames):
        if todo[i]:
            continue
        c = len(frame_of)
        frame_of.append(i)
        K = np.asarray(fr.K_cam, np.float32)
        K4.append([K[0, 0], K[0, 2], K[1, 1], K[1, 2]])
        Rt.append(np.asarray(fr.pose_cam, np.float32)[:3, :4].astype(np.float64))
        ids = np.asarray(fr.unique_pixel_ids, np.int64)
        if len(ids) == 0 or len(pid) == 0:
            continue
        pos = np.minimum(np.searchsorted(pid_s, ids), len(pid_s) - 1)
        hit = np.nonzero(pid_s[pos] == ids)[0]
        cams.append(np.full(len(hit), c, np.int32)); pts.append(order[pos[hit]].astype(np.int32)); kps.append(hit.astype(np.int64))
        uvs.append(np.asarray(fr.keypoints, np.float32).reshape(-1, 2)[hit])
    cat = lambda parts, shape, dt: np.concatenate(parts) if parts else np.zeros(shape, dt)   # noqa: E731
    return (cat(cams, 0, np.int32), cat(pts, 0, np.int32), cat(uvs, (0, 2), np.float32), np.array(K4, np.float32).reshape(-1, 4),
            np.array(Rt, np.float64).reshape(-1, 3, 4), frame_of, cat(kps, 0, np.int64))


def refine_tracks(frames: Sequence[Frame], todo: Sequence[bool], cloud: SparsePointCloud, options: Optional[TrackOptions] = None,
                  ctx: Optional[Context] = None, evaluate_only: bool = False):
    """Re-triangulate (or, with evaluate_only, only judge) every cloud point from all its observations in the registered frames.
    Kept points are written back as float32; points that are not kept leave all four cloud arrays together, as outlierFilter
    removes points; unique_pixel_has_match is cleared on the outlier observations of kept points (setBAProblem alone reads that
    flag, so bundle adjustment stops using them).  A point dropped here may be added again by a later doTriangulation and is then
    judged again by the next call.  Prints one "Track refine:" line and returns (tracks, re-triangulated, points dropped,
    observations dropped)."""
    cam_idx, pt_idx, uv, K4, Rt, frame_of, kp = track_observations(frames, todo, cloud)
    xyz0 = np.asarray(cloud.xyz, np.float32).reshape(-1, 3)
    n_pt = len(xyz0)
    if evaluate_only:
        res = track_evaluate(cam_idx, pt_idx, uv, K4, Rt, xyz0.astype(np.float64), options, ctx)
    else:
        res = track_triangulate(cam_idx, pt_idx, uv, K4, Rt, n_pt, xyz0.astype(np.float64), options, ctx)
    keep = res.status == STATUS_KEPT
    n_tracks = int(np.count_nonzero(np.bincount(pt_idx, minlength=n_pt) >= 2)) if n_pt else 0
    n_retri = 0 if evaluate_only else int(keep.sum())
    drop_obs = ~res.obs_inlier & keep[pt_idx] if len(pt_idx) else np.zeros(0, bool)
    n_obs_dropped = 0
    for c, i in enumerate(frame_of):
        sel = drop_obs & (cam_idx == c)
        flags = np.asarray(frames[i].unique_pixel_has_match, bool)
        n_obs_dropped += int(np.count_nonzero(flags[kp[sel]]))
        flags[kp[sel]] = False
        frames[i].unique_pixel_has_match = flags
    if not evaluate_only:
        xyz0 = np.where(keep[:, None], res.xyz.astype(np.float32), xyz0)
    cloud.xyz = xyz0[keep].copy()
    if len(cloud.rgb) == n_pt:
        cloud.rgb = np.asarray(cloud.rgb)[keep].copy()
    cloud.unique_point_ids = np.asarray(cloud.unique_point_ids)[keep].copy()
    cloud.is_inlier = np.asarray(cloud.is_inlier)[keep].copy()
    counts = (n_tracks, n_retri, int(n_pt - keep.sum()), n_obs_dropped)
    print(f"Track refine: [{counts[0]}] tracks, [{counts[1]}] re-triangulated, [{counts[2]}] points dropped, [{counts[3]}] observations dropped")
    return counts
