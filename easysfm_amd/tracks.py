"""Robust multi-view track triangulation and the reprojection filter (include/esfm.h "Track triangulation").

``track_triangulate`` re-estimates every point from all the observations of its track (two-ray midpoint hypotheses scored by
inlier count and truncated cost, a Gauss-Newton refit on the winner's inliers) and judges it by reprojection error, depth sign
and triangulation angle; ``track_evaluate`` judges given points the same way without re-estimating them.  Both run on the GPU;
``host=True`` runs the same arithmetic compiled for the CPU (no GPU needed).  ``refine_tracks`` applies them to a reconstruction
in progress.  The defaults -- 4 px, 1.5 degrees -- are the common conventions of incremental SfM and have not been measured on
this project's data.

``track_complete`` (include/esfm.h "Track completion") adds observations: every point is projected into every camera that does not
observe it, and the free keypoint near the projection whose descriptor is nearest to the track's takes the point;
``complete_tracks`` applies it to a reconstruction in progress."""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional, Sequence

import numpy as np

from ._lib import ESFM_HAMMING, ESFM_L2_F32, Context, TrackCompleteOptionsStruct, TrackOptionsStruct, check, default_context, lib
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


# ---- track completion --------------------------------------------------------------------------------------------------------
class TrackCompleteOptions:
    """esfm_track_complete_options: conventions of incremental SfM, not measured on this project's data."""

    def __init__(self, search_radius_px: float = 4.0, max_distance: float = math.inf, ratio: float = 0.8, max_refs: int = 8):
        self.search_radius_px = float(search_radius_px)
        self.max_distance = float(max_distance)
        self.ratio = float(ratio)
        self.max_refs = int(max_refs)

    def struct(self) -> TrackCompleteOptionsStruct:
        return TrackCompleteOptionsStruct(self.search_radius_px, self.max_distance, self.ratio, self.max_refs, 0)


class TrackCompleteResult(NamedTuple):
    kp_point: np.ndarray            # [rows] int32: the point a keypoint row is given to, or -1
    kp_dist: np.ndarray             # [rows] float32: its descriptor distance d0, or FLT_MAX
    stats: np.ndarray               # int64[4]: jobs with an admissible row, proposals, proposals lost to a conflict, keypoints assigned


def track_complete(desc, kp, kp_free, set_row_offset, K4, Rt, xyz, cam_idx, pt_idx, obs_kp, options: Optional[TrackCompleteOptions] = None,
                   ctx: Optional[Context] = None, host: bool = False) -> TrackCompleteResult:
    """esfm_track_complete (host=True: esfm_track_complete_host).  desc: the cameras' descriptor rows back to back, float32 (L2) or
    uint8 (Hamming, 16 / 32 / 64 bytes); kp [rows, 2] float32; kp_free [rows]; set_row_offset [n_cam + 1]; K4 [n_cam, 4]; Rt
    [n_cam, 3, 4] float64; xyz [n_pt, 3] float64; cam_idx, pt_idx, obs_kp: the existing observations, obs_kp local to its camera."""
    desc = np.asarray(desc)
    metric = ESFM_HAMMING if desc.dtype == np.uint8 else ESFM_L2_F32
    desc = np.ascontiguousarray(desc, np.uint8 if metric == ESFM_HAMMING else np.float32)
    if desc.ndim != 2:
        raise ValueError("desc needs one row per keypoint")
    rows, width = desc.shape
    kp = np.ascontiguousarray(kp, np.float32).reshape(-1, 2)
    kp_free = np.ascontiguousarray(kp_free).astype(np.uint8).reshape(-1)
    off = np.ascontiguousarray(set_row_offset, np.int32).reshape(-1)
    K4 = np.ascontiguousarray(K4, np.float32).reshape(-1, 4)
    Rt = np.ascontiguousarray(Rt, np.float64).reshape(-1, 12)
    xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
    cam_idx = np.ascontiguousarray(cam_idx, np.int32).reshape(-1)
    pt_idx = np.ascontiguousarray(pt_idx, np.int32).reshape(-1)
    obs_kp = np.ascontiguousarray(obs_kp, np.int32).reshape(-1)
    n_cam = len(K4)
    if len(kp) != rows or len(kp_free) != rows or len(off) != n_cam + 1 or len(Rt) != n_cam or int(off[-1]) != rows:
        raise ValueError("kp and kp_free need one row per descriptor row, set_row_offset one entry per camera and one more, ending at the row count")
    if len(pt_idx) != len(cam_idx) or len(obs_kp) != len(cam_idx):
        raise ValueError("cam_idx, pt_idx and obs_kp need one entry per observation")
    opt = (options or TrackCompleteOptions()).struct()
    kp_point = np.full(rows, -1, np.int32); kp_dist = np.full(rows, np.finfo(np.float32).max, np.float32); stats = np.zeros(4, np.int64)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    args = [metric, ptr(desc), ptr(kp), ptr(kp_free), ptr(off), n_cam, int(width), ptr(K4), ptr(Rt), len(xyz), ptr(xyz), len(cam_idx),
            ptr(cam_idx), ptr(pt_idx), ptr(obs_kp), C.byref(opt), ptr(kp_point), ptr(kp_dist), ptr(stats)]
    L = lib()
    if host:
        check(L.esfm_track_complete_host(*args))
    else:
        ctx = ctx or default_context()
        check(L.esfm_track_complete(ctx.handle, *args))
    return TrackCompleteResult(kp_point, kp_dist, stats)


def free_keypoints(frames: Sequence[Frame], cloud: SparsePointCloud):
    """Per frame, which keypoints are free: the unique_pixel_ids value is not a cloud id and no keypoint of any other frame carries
    it -- a keypoint no verified match ever touched, so re-labelling it breaks no track."""
    ids = [np.asarray(f.unique_pixel_ids, np.int64) for f in frames]
    every = np.concatenate(ids) if ids else np.zeros(0, np.int64)
    values, counts = np.unique(every, return_counts=True)
    shared = values[counts > 1]
    pid = np.asarray(cloud.unique_point_ids, np.int64)
    return [~np.isin(i, shared) & ~np.isin(i, pid) for i in ids]


def match_distance_quantile(frames: Sequence[Frame], todo: Sequence[bool], graph, q: float = 0.9) -> float:
    """The q quantile by nearest rank -- the ceil(q n)-th smallest of n -- of the `distance` of all verified matches between
    registered frames; +inf when there is none."""
    d = [m.distance for i in range(len(frames)) for j in range(i) if not todo[i] and not todo[j] for m in graph[i][j].matches]
    if not d:
        return math.inf
    d = np.sort(np.asarray(d, np.float64))
    return float(d[max(int(math.ceil(q * len(d))), 1) - 1])


def complete_inputs(frames: Sequence[Frame], todo: Sequence[bool], cloud: SparsePointCloud):
    """What track_complete takes, from the registered frames: (desc, kp, kp_free, set_row_offset, K4, Rt, xyz, cam_idx, pt_idx,
    obs_kp, frame index per camera)."""
    cam_idx, pt_idx, _, K4, Rt, frame_of, obs_kp = track_observations(frames, todo, cloud)
    free = free_keypoints(frames, cloud)
    desc = [np.asarray(frames[i].descriptors) for i in frame_of]
    off = np.concatenate([[0], np.cumsum([len(frames[i].keypoints) for i in frame_of])]).astype(np.int32)
    kp = [np.asarray(frames[i].keypoints, np.float32).reshape(-1, 2) for i in frame_of]
    cat = lambda parts, empty: np.concatenate(parts) if parts else empty   # noqa: E731
    return (cat(desc, np.zeros((0, 1), np.float32)), cat(kp, np.zeros((0, 2), np.float32)), cat([free[i] for i in frame_of], np.zeros(0, bool)), off,
            K4, Rt, np.asarray(cloud.xyz, np.float32).reshape(-1, 3).astype(np.float64), cam_idx, pt_idx, obs_kp.astype(np.int32), frame_of)


def complete_tracks(frames: Sequence[Frame], todo: Sequence[bool], cloud: SparsePointCloud, options: Optional[TrackCompleteOptions] = None,
                    ctx: Optional[Context] = None, graph=None, track_matrix=None, host: bool = False):
    """Projection search over the registered frames: a free keypoint that track_complete gives to a cloud point takes the point's
    id and unique_pixel_has_match = True (in a frame that has no observation in bundle adjustment yet: the id alone; track_matrix,
    propagate_track_ids' feature_track_matrix, follows when given).  With
    options.max_distance left at +inf and a graph, the gate is match_distance_quantile (the 0.9 quantile by nearest rank of the
    verified matches' distances between registered frames; a convention, not tuned).  Prints one "Track complete:" line and returns
    (jobs with a candidate, observations added, points that gained one, conflicts)."""
    o = options or TrackCompleteOptions()
    if math.isinf(o.max_distance) and o.max_distance > 0 and graph is not None:
        o = TrackCompleteOptions(o.search_radius_px, match_distance_quantile(frames, todo, graph), o.ratio, o.max_refs)
    desc, kp, kp_free, off, K4, Rt, xyz, cam_idx, pt_idx, obs_kp, frame_of = complete_inputs(frames, todo, cloud)
    if len(desc) == 0:
        counts = (0, 0, 0, 0)
    else:
        res = track_complete(desc, kp, kp_free, off, K4, Rt, xyz, cam_idx, pt_idx, obs_kp, o, ctx, host)
        pid = np.asarray(cloud.unique_point_ids, np.int64)
        for c, i in enumerate(frame_of):
            won = res.kp_point[off[c]:off[c + 1]]
            k = np.nonzero(won >= 0)[0]
            if len(k) == 0:
                continue
            ids = np.asarray(frames[i].unique_pixel_ids).copy(); flags = np.asarray(frames[i].unique_pixel_has_match, bool).copy()
            # A frame none of whose keypoints enters bundle adjustment (setBAProblem takes has_match keypoints only, and every keypoint
            # of the first frame is its track's first observer) keeps it that way: the new observations take the id, so that
            # re-triangulation sees them, but not the flag -- a handful of observations would free that camera in the adjustment on
            # little data (measured on synth.sfm_scene(): largest camera-centre error 0.0037 -> 0.0167 with 12 of them).
            in_ba = bool(np.any(flags & np.isin(ids, pid)))
            if track_matrix is not None:
                track_matrix[i, ids[k]] = False
                track_matrix[i, pid[won[k]]] = True
            ids[k] = pid[won[k]]; flags[k] = in_ba
            frames[i].unique_pixel_ids = ids; frames[i].unique_pixel_has_match = flags
        counts = (int(res.stats[0]), int(res.stats[3]), int(len(np.unique(res.kp_point[res.kp_point >= 0]))), int(res.stats[2]))
    print(f"Track complete: [{counts[0]}] candidates, [{counts[1]}] observations added to [{counts[2]}] points, [{counts[3]}] conflicts")
    return counts
