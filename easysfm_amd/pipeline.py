"""The body of the reference's ``main`` after feature extraction (cpp_code/test/sfm.cpp:128-339), mirrored over the GPU
stages of this package: all-pairs matching -> 5-point RANSAC + relative depth per pair -> track ids -> initial pair ->
triangulation -> BA -> (next frame by PnP -> triangulation -> periodic BA)* -> final BA -> SOR filter -> .ply.

Feature extraction (detectFeaturesSURF / detectFeaturesORB from pixels, sfm.cpp:84-126) lives in
``features.py``; ``run_sfm`` starts from frames that already carry keypoints and descriptors.  The stages that the reference runs pair by
pair but whose results do not depend on the loop state (matching, RANSAC, pose recovery, depth) are batched over all pairs;
the track bookkeeping that does depend on it runs in the reference's order."""
from __future__ import annotations

from dataclasses import dataclass, field
import os
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from ._lib import Context, ESFM_HAMMING, ESFM_L2_F32, default_context
from .ba import BundleAdjustment
from .cloud import CProceesing, write_ply, write_ply_mesh, write_ply_normals, write_ply_textured_mesh, write_png_rgb
from .matching import DescriptorBank, FeatureMatching, PairMatcher
from .motion import (FOCAL_MIN_DEPTH, MotionEstimator, _dehomogenise, find_essential_pairs, find_fundamental_pairs, find_homography_pairs,
                     focal_from_fundamentals, pixel2cam, recover_pose_pairs, triangulate_pairs)
from .mesh import (MeshCleanOptions, MeshOptions, auto_texels, default_atlas_width, mesh_arrays, mesh_clean, mesh_components, mesh_simplify,
                   mesh_texture_bake, mesh_texture_level, mesh_texture_views)
from .render import mesh_render, mesh_render_error
from .mvs import MergeOptions, default_mvs_options, dense_reconstruction, frame_arrays, merge_arrays
from .retrieval import RetrievalOptions, select_pairs, working_dim
from .tracks import TrackCompleteOptions, TrackOptions, complete_tracks, refine_tracks
from .types import DMatch, Frame, SparsePointCloud
from .cameras import check_one_image_size, distortion_line, pair_stage_view, refresh_pinhole_keypoints
from .features import undistort


@dataclass
class FramePair:
    """frame_pair_t (utility.h:57-78)."""
    frame_id_1: int
    frame_id_2: int
    matches: List[DMatch] = field(default_factory=list)
    T_21: np.ndarray = field(default_factory=lambda: np.eye(4, dtype=np.float32))
    appro_depth: float = 1.0
    h_inliers: int = 0            # correspondences within the threshold of the returned, re-fitted homography (esfm_find_homography_pairs'
                                  # n_inliers: not the RANSAC mask's count); homography_check only
    h_inlier_ratio: float = 0.0   # ... divided by the essential matrix's RANSAC mask count: near 1 for a planar or rotation-only pair


@dataclass
class AutoFocalOptions:
    """run_sfm(auto_focal=...): the uncalibrated start (esfm.h "Fundamental-matrix RANSAC").  Every camera_id's K_cam is set from the
    fundamental matrices of its own pairs; what the frames carried in K_cam before is not read."""
    image_size: Optional[Tuple[int, int]] = None   # (width, height) of frames that carry no rgb_image
    min_depth: float = FOCAL_MIN_DEPTH             # the estimate counts from this depth of the coarse cost curve's minimum on
    max_h_inlier_ratio: float = 0.8                # homography inliers / F inliers above which a pair is planar or panoramic: its F means nothing
    fallback_factor: float = 1.2                   # f = this x max(width, height) without a usable estimate: the common convention


def _frame_size(f: Frame, options: AutoFocalOptions) -> Tuple[float, float]:
    if f.rgb_image is not None:
        h, w = np.asarray(f.rgb_image).shape[:2]
        return float(w), float(h)
    if options.image_size is None:
        raise ValueError("auto_focal needs the image size: a frame carries no rgb_image and AutoFocalOptions.image_size is not set")
    return float(options.image_size[0]), float(options.image_size[1])


def _centred_K(f: float, w: float, h: float) -> np.ndarray:
    return np.array([[f, 0.0, w / 2.0], [0.0, f, h / 2.0], [0.0, 0.0, 1.0]], np.float32)


def auto_focal_calibration(frames: Sequence[Frame], options: AutoFocalOptions, ransac_reproj_distance: float, num_min_pair: int,
                           ctx: Optional[Context] = None) -> Callable:
    """The `calibrate` callable run_sfm hands to match_and_verify_all_pairs.  Over the matched correspondences of all pairs: one
    esfm_find_fundamental_pairs call (threshold ransac_reproj_distance, confidence 0.99) and one esfm_find_homography_pairs call; a pair
    is kept when its F has more than num_min_pair inliers and its homography inliers / F inliers do not exceed
    options.max_h_inlier_ratio, and weighs as much as its F inliers.  Every camera_id then gets K_cam = [f 0 w/2; 0 f h/2; 0 0 1] on all
    its frames, f from motion.focal_from_fundamentals over the kept pairs BOTH of whose frames it took; without such a pair, or with an
    estimate that is not confident, f = options.fallback_factor x max(w, h).  Prints one "Auto focal:" line per camera."""
    sizes = {}
    for f in frames:
        sizes.setdefault(int(f.camera_id), _frame_size(f, options))

    def calibrate(pairs, sel, off, p1, p2):
        F, _, status, _, f_inl = find_fundamental_pairs(off, p1, p2, ransac_reproj_distance, 0.99, ctx)
        _, _, _, _, h_inl = find_homography_pairs(off, p1, p2, ransac_reproj_distance, 0.995, ctx)
        for cam, (w, h) in sorted(sizes.items()):
            own = [s for s, k in enumerate(sel) if int(frames[pairs[k][0]].camera_id) == cam and int(frames[pairs[k][1]].camera_id) == cam]
            used = [s for s in own if status[s] and f_inl[s] > num_min_pair and float(h_inl[s]) / float(f_inl[s]) <= options.max_h_inlier_ratio]
            focal, depth, verdict = options.fallback_factor * max(w, h), 0.0, "fallback"
            if used:
                est = focal_from_fundamentals(F[used], f_inl[used].astype(np.float64), w, h, options, ctx)
                depth = est["depth"]
                if est["confident"]:
                    focal, verdict = est["f"], "estimated"
            for f in frames:
                if int(f.camera_id) == cam:
                    f.K_cam = _centred_K(focal, w, h)
            print(f"Auto focal: camera [{cam}] f = [{focal:.2f}] from [{len(used)}] of [{len(own)}] pairs, depth [{depth:.4f}], {verdict}")
    return calibrate


MATCH_FILTERS = ("ratio", "cross", "ratio+cross", "ratio+guided", "cross+guided", "ratio+cross+guided")


def merge_guided(plain, guided):
    """The union of a pair's plain RANSAC inliers and its guided list, (queryIdx, trainIdx, distance) arrays each, in ascending
    query order: a query both lists hold carries the same train row in both (esfm.h "Epipolar-guided matching", property (b)), so
    the guided entries of the queries the plain list lacks are added."""
    pq, pt, pd = plain
    gq, gt, gd = guided
    new = ~np.isin(gq, pq)
    q = np.concatenate([pq, gq[new]]); t = np.concatenate([pt, gt[new]]); d = np.concatenate([pd, gd[new]])
    order = np.argsort(q, kind="stable")
    return q[order], t[order], d[order]


def _checked_pairs(pairs, n_frames: int) -> np.ndarray:
    """A pair list as match_and_verify_all_pairs takes it: int32 [P, 2], every pair (i, j) with 0 <= j < i < n_frames, none twice."""
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    if len(pairs) and not (np.all(pairs[:, 1] >= 0) and np.all(pairs[:, 0] > pairs[:, 1]) and np.all(pairs[:, 0] < n_frames)):
        raise ValueError("pairs must be (i, j) with 0 <= j < i < the number of frames")
    if len(np.unique(pairs, axis=0)) != len(pairs):
        raise ValueError("pairs lists a pair twice")
    return pairs


def match_and_verify_all_pairs(frames: Sequence[Frame], use_feature: str = "S", ransac_reproj_distance: float = 1.0,
                               num_min_pair: int = 20, ctx: Optional[Context] = None, match_filter: str = "ratio",
                               homography_check: bool = False, pairs=None, calibrate: Optional[Callable] = None) -> List[List[FramePair]]:
    """sfm.cpp:140-167 for every (i, j < i): matchFeatures{SURF,ORB,SIFT}(frames[i], frames[j]) (use_feature S, O or I); if more than num_min_pair
    matches survive, estimate2D2D_E5P_RANSAC (threshold = ransac_reproj_distance, prob 0.99) and getDepthFast on the inliers;
    otherwise no inliers, identity transform, depth 1 (:147-148).  Returns img_match_graph[i][j].
    match_filter: "ratio" (the reference's one-way Lowe test), "cross" (mutual nearest neighbours) or "ratio+cross" (both, the
    ratio test in both directions: esfm.h "Cross-check matching").  With "+guided" appended, every pair that got an essential
    matrix is matched a second time with the search restricted to the rows that matrix admits within ransac_reproj_distance (one
    esfm_match_guided_pairs_dev call, the same filter), and its matches become the union of the RANSAC inliers and that list;
    T_21 and appro_depth stay those of the first pass.
    homography_check: one esfm_find_homography_pairs call (esfm.h "Homography RANSAC", confidence 0.995) over the same
    correspondences and the same ransac_reproj_distance fills h_inliers and h_inlier_ratio = homography inliers / essential-matrix
    RANSAC inliers (the mask of find_essential_pairs, before recoverPose) of every pair that got an essential matrix; matches, T_21
    and appro_depth are untouched.
    pairs: None for every (i, j < i); else an int32 [P, 2] list of (i, j < i) pairs (retrieval.select_pairs' output), or a callable
    that is given the DescriptorBank built here and returns such a list (so that a selection runs on the rows already uploaded).
    Only the listed pairs are matched and verified; every other graph[i][j] stays the default FramePair.
    calibrate: when given, it is called once as calibrate(pairs, sel, off, p1, p2) after matching and before any frame's K_cam is read --
    pairs the int32 [P, 2] pair list, sel the indices into it of the pairs with more than num_min_pair matches, off / p1 / p2 their
    concatenated matched pixels -- and may set the frames' K_cam (auto_focal_calibration).  None: nothing changes."""
    if match_filter not in MATCH_FILTERS:
        raise ValueError(f"match_filter must be one of {MATCH_FILTERS}, not {match_filter!r}")
    ctx = ctx or default_context()
    n = len(frames)
    metric = ESFM_HAMMING if use_feature == "O" else ESFM_L2_F32
    ratio = {"O": 0.8, "I": 0.7}.get(use_feature, 0.5)                   # I (SIFT): the prototype's nn_ratio
    selection = pairs
    pairs = np.array([(i, j) for i in range(n) for j in range(i)], np.int32).reshape(-1, 2)
    graph: List[List[FramePair]] = [[FramePair(i, j) for j in range(i)] for i in range(n)]
    if len(pairs) == 0:
        return graph
    if selection is not None and not callable(selection):
        pairs = _checked_pairs(selection, n)
        if len(pairs) == 0:
            return graph
    guided = match_filter.endswith("+guided")
    first_filter = match_filter[:-len("+guided")] if guided else match_filter
    kps = [np.asarray(f.keypoints, np.float32).reshape(-1, 2) for f in frames] if guided else None
    bank = DescriptorBank([f.descriptors for f in frames], metric, device=f"cuda:{ctx.device}", keypoints=kps)
    if callable(selection):
        pairs = _checked_pairs(selection(bank), n)
        if len(pairs) == 0:
            return graph
    pm = PairMatcher(bank, pairs, ctx)                                  # drains torch's upload stream before its first launch
    if first_filter == "ratio":
        res = pm.match(ratio).to_host()
    else:
        res = pm.match_cross(ratio if first_filter == "ratio+cross" else None).to_host()
    # RANSAC + pose for every pair with enough matches, in shared launches
    sel = [k for k in range(len(pairs)) if len(res[k][0]) > num_min_pair]
    if sel:
        off = np.concatenate([[0], np.cumsum([len(res[k][0]) for k in sel])]).astype(np.int32)
        p1 = np.concatenate([np.asarray(frames[pairs[k][0]].keypoints, np.float32).reshape(-1, 2)[res[k][0]] for k in sel])
        p2 = np.concatenate([np.asarray(frames[pairs[k][1]].keypoints, np.float32).reshape(-1, 2)[res[k][1]] for k in sel])
        if calibrate is not None:
            calibrate(pairs, sel, off, p1, p2)
        K4 = np.array([[frames[pairs[k][0]].K_cam[0, 0], frames[pairs[k][0]].K_cam[0, 2], frames[pairs[k][0]].K_cam[1, 1],
                        frames[pairs[k][0]].K_cam[1, 2]] for k in sel], np.float32)
        Es, mask, status, _ = find_essential_pairs(off, p1, p2, K4, 0.99, ransac_reproj_distance, ctx)
        good, Rs, ts, _ = recover_pose_pairs(off, p1, p2, K4, Es, mask, ctx)
        verified = [s for s in range(len(sel)) if status[s]]
        if homography_check:
            _, _, _, _, h_inl = find_homography_pairs(off, p1, p2, ransac_reproj_distance, 0.995, ctx)
            for s in verified:
                i, j = pairs[sel[s]]
                e_inl = int(np.count_nonzero(mask[off[s]:off[s + 1]]))
                graph[i][j].h_inliers = int(h_inl[s])
                graph[i][j].h_inlier_ratio = float(h_inl[s]) / float(e_inl) if e_inl else 0.0
        extra = {}
        if guided and verified:
            lists = pm.match_guided([sel[s] for s in verified], Es[verified], K4[verified], ransac_reproj_distance,
                                    None if first_filter == "cross" else ratio, first_filter != "ratio").to_host()
            extra = dict(zip(verified, lists))
        # getDepthFast: every 20th inlier match, identity vs T_21, frame i's K for both images
        jobs_P2, jobs_a, jobs_b, jobs_off, jobs_k = [], [], [], [0], []
        for s, k in enumerate(sel):
            i, j = pairs[k]
            g = graph[i][j]
            if not status[s]:
                continue
            m = mask[off[s]:off[s + 1]]
            q, t, d = res[k]
            kept = (q[m], t[m], d[m]) if s not in extra else merge_guided((q[m], t[m], d[m]), extra[s])
            g.matches = [DMatch(int(a), int(b), float(c)) for a, b, c in zip(*kept)]
            T = np.eye(4, dtype=np.float32)
            T[:3, :3] = Rs[s].astype(np.float32); T[:3, 3] = ts[s].astype(np.float32)
            g.T_21 = T
            pick = np.arange(0, int(m.sum()), 20)
            if len(pick):
                Ki = frames[i].K_cam
                jobs_P2.append(T[:3]); jobs_k.append((i, j))
                jobs_a.append(pixel2cam(p1[off[s]:off[s + 1]][m][pick], Ki)); jobs_b.append(pixel2cam(p2[off[s]:off[s + 1]][m][pick], Ki))
                jobs_off.append(jobs_off[-1] + len(pick))
        if jobs_k:
            P1 = np.tile(np.eye(4, dtype=np.float32)[:3], (len(jobs_k), 1, 1))
            h = triangulate_pairs(P1, np.stack(jobs_P2), np.array(jobs_off, np.int32), np.concatenate(jobs_a), np.concatenate(jobs_b), ctx)
            for s, (i, j) in enumerate(jobs_k):
                p = _dehomogenise(h[jobs_off[s]:jobs_off[s + 1]])
                depth_sum = 0.0
                for v in p:
                    depth_sum += float(np.sqrt(np.float32(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])))
                graph[i][j].appro_depth = depth_sum / len(p)
    return graph


def propagate_track_ids(frames: Sequence[Frame], graph: List[List[FramePair]]):
    """sfm.cpp:173-216: a frame's keypoint takes the track id of its verified match in an earlier frame unless that id is
    already used in the frame; unmatched keypoints get fresh ids.  Returns (feature_track_matrix [n_frames, n_total_keypoints]
    bool, number of unique points)."""
    n = len(frames)
    total = sum(len(f.keypoints) for f in frames)
    track = np.zeros((n, max(total, 1)), bool)
    cur = 0
    for i in range(n):
        fi = frames[i]
        used = set(int(v) for v in fi.unique_pixel_ids if v >= 0)
        for j in range(i):
            fj = frames[j]
            for m in graph[i][j].matches:
                tid = int(fj.unique_pixel_ids[m.trainIdx])
                if fi.unique_pixel_ids[m.queryIdx] < 0 or fi.unique_pixel_ids[m.queryIdx] != tid:
                    if tid not in used:                                  # is_duplicated scan (:181-188)
                        old = int(fi.unique_pixel_ids[m.queryIdx])
                        fi.unique_pixel_ids[m.queryIdx] = tid
                        fi.unique_pixel_has_match[m.queryIdx] = True
                        used.add(tid)
                        if old >= 0 and not np.any(fi.unique_pixel_ids == old):
                            used.discard(old)
        fresh = 0
        for k in range(len(fi.unique_pixel_ids)):
            if fi.unique_pixel_ids[k] < 0:
                fi.unique_pixel_ids[k] = cur + fresh
                fresh += 1
            track[i, fi.unique_pixel_ids[k]] = True
        cur += fresh
    return track, cur


def run_sfm(frames: List[Frame], output_file: Optional[str] = None, use_feature: str = "S", ransac_reproj_distance: float = 1.0,
            use_track_frames_as_init: bool = True, fix_calib_tolerance_BA: float = 0.0, frequency_BA: int = 4,
            ctx: Optional[Context] = None, verbose: bool = False, match_filter: str = "ratio", dense_output_file: Optional[str] = None,
            dense_merged_output_file: Optional[str] = None, dense_mesh_output_file: Optional[str] = None,
            dense_mesh_clean: Optional[MeshCleanOptions] = None, dense_mesh_simplify: Optional[float] = None,
            dense_mesh_texture: Optional[int] = None, dense_mesh_texture_level: bool = False, dense_mesh_render_dir: Optional[str] = None,
            init_max_h_inlier_ratio: Optional[float] = None, track_refine: Optional[TrackOptions] = None,
            pair_selection: Optional[RetrievalOptions] = None, ba_radial_tolerance: Optional[float] = None,
            auto_focal: Optional[AutoFocalOptions] = None, track_complete: Optional[TrackCompleteOptions] = None):
    """sfm.cpp:128-339.  Returns (sparse cloud before the final filter, filtered cloud, img_match_graph).
    dense_output_file: after the final BA and the sparse .ply, run dense_reconstruct on the registered frames and the cloud
    before the filter (it carries the track ids) and write the dense cloud there (esfm.h "Dense reconstruction").
    dense_merged_output_file: merge that dense cloud into one oriented point per voxel that two or more views support (esfm.h
    "Dense-cloud merge", mvs.dense_merge's defaults) and write it there with write_ply_normals.
    dense_mesh_output_file: integrate the depth maps, masked to the pixels the fusion kept, into a signed distance volume and
    write the triangle mesh extracted from it there with write_ply_mesh (esfm.h "Surface reconstruction", mesh.dense_mesh's
    defaults); prints one "Dense mesh:" line.
    dense_mesh_clean: with dense_mesh_output_file, clean that mesh with these options before it is written (esfm.h "Mesh
    clean-up": small components dropped, Taubin smoothing, normals from the faces); prints one "Mesh clean:" line.  None: the
    mesh is written as extracted.
    dense_mesh_simplify: with dense_mesh_output_file, the side of a simplification cell in voxels of the signed distance volume:
    after the optional clean-up all vertices of one cell, counted from the volume's origin, are merged into one (esfm.h "Mesh
    simplification", default options); prints one "Mesh simplify:" line.  None: no simplification.
    dense_mesh_texture: with dense_mesh_output_file, the chart size in texels (4..64), or 0 to derive it from the triangles' screen
    areas: after the optional clean-up and simplification every triangle chooses one of the registered frames (at most 64, in
    frame order) and a texture atlas is baked from them (esfm.h "Mesh texturing", default options, a square atlas); the mesh is
    written with texture coordinates and the atlas beside it as a .png; prints one "Mesh texture:" line.  None: vertex colours only.
    dense_mesh_texture_level: with dense_mesh_texture, level the seams between triangles that chose different frames before the bake
    (esfm.h "Mesh texturing", esfm_mesh_texture_level, default options); prints one "Mesh texture level:" line.
    dense_mesh_render_dir: with dense_mesh_output_file, an existing directory (it is not created here, nor by the drivers): after the mesh is written it is drawn into every registered frame,
    in frame order (esfm.h "Mesh rendering", default options; with the atlas if the mesh was textured, else with its vertex colours);
    the pictures go there as render_%04d.png, numbered by frame index, and one "Mesh render:" line states the number of views, the
    pixels the mesh covers in them and the mean absolute difference to the photographs over those pixels and three channels.
    init_max_h_inlier_ratio: when given, every verified pair also gets a homography RANSAC (match_and_verify_all_pairs'
    homography_check) and findInitializeFramePair skips the pairs whose h_inlier_ratio exceeds this limit (0.8 separates planar and
    rotation-only pairs from general ones by an order of magnitude: DESIGN 6.4); prints one "Init pair:" line.  None: no check, every
    output as before.
    track_refine: when given, tracks.refine_tracks runs immediately before every doSFMBA call (every cloud point is re-triangulated
    from all its observations in the registered frames; points that fail the reprojection / depth / angle verdict and the outlier
    observations of the others leave bundle adjustment) and once more after the final doSFMBA, before SORFilter, as a filter alone
    (evaluate_only); each call prints one "Track refine:" line (esfm.h "Track triangulation").  A point dropped by one call may be
    added again by a later doTriangulation and is then judged again.  None: every output as before, to the bit.
    track_complete: when given, tracks.complete_tracks runs immediately before every refine_tracks call but the final evaluate-only
    one (without track_refine: immediately before every doSFMBA call), so that re-triangulation and bundle adjustment see the new
    observations: every cloud point is projected into the registered frames that do not observe it, and a keypoint no verified match
    has touched, near the projection and with a descriptor that agrees with the track's, takes the point's id (esfm.h "Track
    completion"); max_distance left at +inf becomes the 0.9 quantile of the verified matches' distances between registered frames;
    each call prints one "Track complete:" line.  It reads keypoints (the pinhole-equivalent pixels) and every frame's own K_cam.
    A new observation also gets unique_pixel_has_match = True and so enters bundle adjustment -- except in a frame none of whose
    keypoints is in bundle adjustment yet (the first frame, always): there it takes the id alone, for re-triangulation, and the
    frame stays out of the adjustment as it was (DESIGN 6.5a "One deviation").  None: every output as before, to the bit.
    pair_selection: when given, retrieval.select_pairs chooses the pairs to match (esfm.h "Image retrieval": the top_k most similar
    images of every image by int8 VLAD, plus the `window` preceding ones) on the descriptor rows the matcher has uploaded, and only
    those pairs are matched and verified; prints one "Pair selection:" line.  None: every output as before, to the bit.
    ba_radial_tolerance: when given (> 0), every bundle adjustment also frees k1, k2 of every camera_id, boxed to their start +- this
    value (esfm.h "Free radial distortion"; with fix_calib_tolerance_BA == 0 a narrow box holds fx, cx, fy, cy).  Frames keep the
    pixels as detected in keypoints_raw, which is what bundle adjustment observes; keypoints is the pinhole-equivalent pixel of the
    frame's current (K_cam, radial_cam) (cameras.pinhole_keypoints), refreshed for every frame after every bundle adjustment, and
    it is what the pair stage, PnP, triangulation, guided matching and track refinement read.  With a dense output every registered
    frame's image is undistorted with its camera's final k1, k2 first.  Prints one "Distortion:" line.  None: every output as
    before, to the bit.
    auto_focal: when given, no K_cam is read: after matching, every camera_id's K_cam is set from the fundamental matrices of its own
    pairs (auto_focal_calibration; esfm.h "Fundamental-matrix RANSAC"), the principal point at the image centre, and everything behind
    runs as with that K given; one "Auto focal:" line per camera.  It is a start value: give fix_calib_tolerance_BA > 0 so that
    bundle adjustment polishes it.  A pair across two cameras is verified with its first frame's K, as in a one-camera run (two focal
    lengths per pair are left out); not combined with ba_radial_tolerance.  None: every output as before, to the bit."""
    if ba_radial_tolerance is not None and not ba_radial_tolerance > 0.0:
        raise ValueError("ba_radial_tolerance must be positive")
    calibrate = None
    if auto_focal is not None:
        if ba_radial_tolerance is not None:
            raise ValueError("auto_focal cannot be combined with ba_radial_tolerance")
        ctx = ctx or default_context()
        calibrate = auto_focal_calibration(frames, auto_focal, ransac_reproj_distance, 20, ctx)     # (reads every frame's size: fails before any work)
        w, h = _frame_size(frames[0], auto_focal)
        for f in frames:                                # one placeholder K until `calibrate` runs: the pair stage then sees the pixels as detected
            f.K_cam = _centred_K(auto_focal.fallback_factor * max(w, h), w, h)
    ctx = ctx or default_context()
    fm, ee = FeatureMatching(ctx), MotionEstimator(ctx)
    for f in frames:
        f.init_pixel_ids()
    if dense_output_file or dense_merged_output_file or dense_mesh_output_file:
        check_one_image_size(frames)                    # before any work: the dense stages take one image size
    # Multiple-camera mode (cameras.py): frames that do not all share one K_cam go through the pair stage with their keypoints remapped
    # into the canonical camera's pixels and its K -- ransac_reproj_distance is then in canonical pixels; everything behind the pair
    # stage sees the original pixels and each frame's own K_cam.  One K_cam: nothing is touched.
    if ba_radial_tolerance is not None:
        refresh_pinhole_keypoints(frames)               # keypoints_raw <- the detected pixels; keypoints: those of the start (K_cam, radial_cam)
    with pair_stage_view(frames):
        graph = _pair_stage(frames, use_feature, ransac_reproj_distance, ctx, match_filter, init_max_h_inlier_ratio, pair_selection, calibrate)
    return _run_sfm_after_pairs(frames, graph, fm, ee, output_file, ransac_reproj_distance, use_track_frames_as_init, fix_calib_tolerance_BA,
                                frequency_BA, ctx, verbose, dense_output_file, dense_merged_output_file, dense_mesh_output_file, dense_mesh_clean,
                                dense_mesh_simplify, dense_mesh_texture, dense_mesh_texture_level, dense_mesh_render_dir, init_max_h_inlier_ratio,
                                track_refine, ba_radial_tolerance, track_complete)


def undistort_registered_images(frames, todo, ctx: Optional[Context] = None) -> None:
    """The dense chain models a pinhole: every registered frame's image goes once more through the existing undistortion (esfm_undistort:
    k1, k2, p1, p2) with its own K_cam and its camera's final k1, k2 (p1 = p2 = 0).  Frames without an image, or with k1 = k2 = 0, and
    frames still to be registered are left alone."""
    for f, t in zip(frames, todo):
        if not t and f.rgb_image is not None and any(f.radial_cam):
            f.rgb_image = undistort(f.rgb_image, f.K_cam, np.array([f.radial_cam[0], f.radial_cam[1], 0.0, 0.0], np.float64), ctx)


def _pair_stage(frames, use_feature, ransac_reproj_distance, ctx, match_filter, init_max_h_inlier_ratio, pair_selection, calibrate=None):
    if pair_selection is None:
        graph = match_and_verify_all_pairs(frames, use_feature, ransac_reproj_distance, 20, ctx, match_filter,
                                           homography_check=init_max_h_inlier_ratio is not None, calibrate=calibrate)
    else:
        def choose(bank):
            chosen = select_pairs(bank, bank.metric, pair_selection, ctx)
            n = len(frames)
            print(f"Pair selection: [{len(chosen)}] of [{n * (n - 1) // 2}] pairs, [{pair_selection.top_k}] nearest of [{n}] images, "
                  f"window [{pair_selection.window}], codebook [{pair_selection.n_centres}] x [{working_dim(bank.metric, bank.width)}]")
            return chosen
        graph = match_and_verify_all_pairs(frames, use_feature, ransac_reproj_distance, 20, ctx, match_filter,
                                           homography_check=init_max_h_inlier_ratio is not None, pairs=choose, calibrate=calibrate)
    return graph


def _run_sfm_after_pairs(frames, graph, fm, ee, output_file, ransac_reproj_distance, use_track_frames_as_init, fix_calib_tolerance_BA, frequency_BA,
                         ctx, verbose, dense_output_file, dense_merged_output_file, dense_mesh_output_file, dense_mesh_clean, dense_mesh_simplify,
                         dense_mesh_texture, dense_mesh_texture_level, dense_mesh_render_dir, init_max_h_inlier_ratio, track_refine,
                         ba_radial_tolerance=None, track_complete=None):
    radial_tol = float(ba_radial_tolerance) if ba_radial_tolerance is not None else 0.0

    def before_adjust():
        """what runs in front of a bundle adjustment: track completion, then track refinement, each when asked for"""
        if track_complete is not None:
            complete_tracks(frames, todo, cloud, track_complete, ctx, graph=graph, track_matrix=track)
        if track_refine is not None:
            refine_tracks(frames, todo, cloud, track_refine, ctx)

    def adjust(tolerance):
        """doSFMBA; in a radial run every frame of a camera then takes that camera's k1, k2 and its keypoints are refreshed"""
        ba.doSFMBA(frames, todo, cloud, tolerance, -1, radial_tol)
        if radial_tol > 0:
            # doSFMBA wrote each group's K_cam and radial_cam to its registered frames; the camera's frames still to be registered take
            # BOTH too, so that their refreshed keypoints are the inverse of one model (and PnP sees the K those pixels belong to)
            by_id = {int(f.camera_id): (f.K_cam, f.radial_cam) for f, t in zip(frames, todo) if not t}
            for f, t in zip(frames, todo):
                if t and int(f.camera_id) in by_id:
                    K, k = by_id[int(f.camera_id)]
                    f.K_cam, f.radial_cam = np.array(K, np.float32, copy=True), k
            refresh_pinhole_keypoints(frames)

    track, n_unique = propagate_track_ids(frames, graph)
    if verbose:
        for i in range(len(frames)):
            for j in range(i):
                if graph[i][j].matches:
                    print(f"Pair ( {i} , {j} ): [{len(graph[i][j].matches)}] verified matches.")
        print(f"The total unique feature point number is {n_unique}")
    init_1, init_2, depth_init = 1, 0, 10.0
    if use_track_frames_as_init:
        if init_max_h_inlier_ratio is None:
            found, a, b, d = fm.findInitializeFramePair(track, frames, [[p.appro_depth for p in row] + [0.0] * (len(frames) - len(row)) for row in graph])
        else:
            h_stats = {}
            found, a, b, d = fm.findInitializeFramePair(track, frames, graph, max_h_inlier_ratio=init_max_h_inlier_ratio, h_stats=h_stats)
            print(f"Init pair: skipped {h_stats['skipped']} of {h_stats['candidates']} candidate pairs as planar or panoramic")
        init_1, init_2 = a, b
        if found:
            depth_init = d
    if verbose:
        print(f"Initialization frames: [ {init_1} ] and [ {init_2} ]")
    cloud = SparsePointCloud()
    frames[init_1].pose_cam = np.eye(4, dtype=np.float32)
    frames[init_2].pose_cam = (graph[init_1][init_2].T_21 @ frames[init_1].pose_cam).astype(np.float32)
    ee.doTriangulation(frames[init_1], frames[init_2], graph[init_1][init_2].matches, cloud, rgb_image=frames[init_1].rgb_image)
    todo = [True] * len(frames)
    todo[init_1] = todo[init_2] = False
    ba = BundleAdjustment(ctx)
    before_adjust()
    adjust(fix_calib_tolerance_BA)
    remaining = len(frames) - 2
    reproj = ransac_reproj_distance
    while remaining > 0:
        nxt = fm.findNextFrame(track, todo, cloud.unique_point_ids, -1)
        if nxt < 0:
            break                                                        # the reference would index with an uninitialised value
        ok = ee.estimate2D3D_P3P_RANSAC(frames[nxt], cloud, reproj)
        reproj += 1.0
        for i in range(len(frames)):
            if not todo[i]:
                if nxt > i:
                    ee.doTriangulation(frames[nxt], frames[i], graph[nxt][i].matches, cloud, rgb_image=frames[nxt].rgb_image)
                else:
                    ee.doTriangulation(frames[i], frames[nxt], graph[i][nxt].matches, cloud, rgb_image=frames[i].rgb_image)
        if not ok:
            ee.outlierFilter(cloud)
        todo[nxt] = False
        remaining -= 1
        if remaining % frequency_BA == 0:
            ba.initBA()
            before_adjust()
            adjust(fix_calib_tolerance_BA)
            reproj = ransac_reproj_distance
        if verbose:
            print(f"Progress: [ {len(frames) - remaining} / {len(frames)} ]")
    before_adjust()
    adjust(0.0)
    if radial_tol > 0:
        print(distortion_line([f for f, t in zip(frames, todo) if not t]))
    if track_refine is not None:
        refine_tracks(frames, todo, cloud, track_refine, ctx, evaluate_only=True)
    out = CProceesing(ctx).SORFilter(cloud)
    if output_file:
        write_ply(output_file, out)
    if (dense_output_file or dense_merged_output_file or dense_mesh_output_file) and radial_tol > 0:
        undistort_registered_images(frames, todo, ctx)
    if dense_output_file or dense_merged_output_file or dense_mesh_output_file:
        dense, nb, rng, depth, _ = dense_reconstruction(frames, todo, cloud, ctx=ctx)
        if dense_output_file:
            if verbose:
                print(f"Dense reconstruction: [{int(np.count_nonzero(rng[:, 0] > 0))}] depth maps, [{len(dense.xyz)}] points.")
            write_ply(dense_output_file, dense)
        if dense_merged_output_file:
            imgs, K4, poses = frame_arrays(frames, todo)
            merged, normals, _, _, _ = merge_arrays(imgs, K4, poses, nb, depth, default_mvs_options(), MergeOptions(), ctx)
            if verbose:
                print(f"Dense merge: [{len(dense.xyz)}] points into [{len(merged.xyz)}] voxels, "
                      f"[{int(np.count_nonzero(np.any(normals != 0, axis=1)))}] with a normal.")
            write_ply_normals(dense_merged_output_file, merged, normals)
        if dense_mesh_output_file:
            imgs, K4, poses = frame_arrays(frames, todo)
            vertices, normals, rgb, triangles, grid = mesh_arrays(imgs, K4, poses, nb, depth, default_mvs_options(), MeshOptions(), ctx)
            print(f"Dense mesh: [{len(vertices)}] vertices, [{len(triangles)}] triangles from [{grid.dims[0]}] x [{grid.dims[1]}] x "
                  f"[{grid.dims[2]}] voxels of [{grid.voxel_size:g}].")
            if dense_mesh_clean is not None:
                n_before = mesh_components(triangles, len(vertices), ctx)[2]
                vertices, normals, rgb, triangles = mesh_clean(vertices, rgb, triangles, dense_mesh_clean, ctx)
                n_after = mesh_components(triangles, len(vertices), ctx)[2]
                print(f"Mesh clean: [{n_after}] of [{n_before}] components kept, [{len(vertices)}] vertices, [{len(triangles)}] triangles.")
            if dense_mesh_simplify is not None:
                n_v, n_t = len(vertices), len(triangles)
                cell = float(np.float32(dense_mesh_simplify) * np.float32(grid.voxel_size))
                vertices, normals, rgb, triangles = mesh_simplify(vertices, rgb, triangles, cell, np.array(grid.origin, np.float32), None, ctx)
                print(f"Mesh simplify: [{n_v}] vertices, [{n_t}] triangles into [{len(vertices)}] vertices, [{len(triangles)}] triangles, "
                      f"cells of [{cell:g}].")
            if dense_mesh_texture is not None:
                reg = ~np.asarray(todo, bool)
                label, score = mesh_texture_views(vertices, triangles, imgs.shape[1], imgs.shape[2], K4[reg], poses[reg], None, ctx)
                texels = int(dense_mesh_texture) if dense_mesh_texture else auto_texels(label, score)
                offsets = None
                if dense_mesh_texture_level:
                    offsets, _, level = mesh_texture_level(vertices, triangles, label, imgs[reg], K4[reg], poses[reg], None, ctx)
                    print(f"Mesh texture level: [{level.nodes}] nodes, [{level.seam_vertices}] seam vertices, [{level.iterations}] iterations")
                atlas, uv = mesh_texture_bake(vertices, rgb, triangles, label, imgs[reg], K4[reg], poses[reg], texels, default_atlas_width(len(triangles)), ctx,
                                              offsets)
                print(f"Mesh texture: [{len(triangles)}] triangles, [{int(np.count_nonzero(label >= 0))}] labelled from [{int(reg.sum())}] views, charts of "
                      f"[{texels}] texels, atlas [{atlas.shape[1]}] x [{atlas.shape[0]}].")
                write_ply_textured_mesh(dense_mesh_output_file, vertices, normals, triangles, uv, atlas)
            else:
                uv = atlas = None
                write_ply_mesh(dense_mesh_output_file, vertices, normals, rgb, triangles)
            if dense_mesh_render_dir:
                registered = np.nonzero(~np.asarray(todo, bool))[0]
                total = covered = 0
                for first in range(0, len(registered), 64):              # esfm_mesh_render takes 64 views per call
                    sel = registered[first:first + 64]
                    pictures, _, ids = mesh_render(vertices, triangles, K4[sel], poses[sel], imgs.shape[1], imgs.shape[2], None if uv is not None else rgb,
                                                   uv, atlas, None, ctx, outputs=("rgb", "triangle_id"))
                    err, cov = mesh_render_error(pictures, ids, imgs[sel])
                    total += int(err.sum()); covered += int(cov.sum())
                    for frame, picture in zip(sel, pictures):
                        write_png_rgb(os.path.join(dense_mesh_render_dir, "render_%04d.png" % int(frame)), picture)
                mean = float(total) / (3.0 * float(covered)) if covered else 0.0
                print(f"Mesh render: [{len(registered)}] views, [{covered}] covered pixels, mean absolute error [{mean:.3f}]")
    return cloud, out, graph
