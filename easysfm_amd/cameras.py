"""Multiple-camera mode in front of the solver: a data set taken with several cameras (intrinsics models).

The pair stage's kernels -- 5-point RANSAC, recoverPose, the homography check, guided matching, getDepthFast -- take ONE K per pair
(the reference uses frame 1's for both images, estimate_motion.cpp:245) and stay as they are.  In a run whose frames do not all share
one ``K_cam`` every image's keypoints are remapped once, on the host, into the pixels of a canonical camera ``K_ref`` -- the ``K_cam``
of camera_id 0 -- and the pair stage sees those keypoints and ``K_ref`` (``pair_stage_view``); ransac_reproj_distance and the guided
matcher's epipolar distance are then in CANONICAL pixels.  Registration, triangulation, tracks, bundle adjustment and everything after
keep the original pixels and each frame's own ``K_cam``.  Frames whose ``K_cam`` equals ``K_ref`` bit for bit are not touched, so a
one-camera run is exactly what it was.

Also the drivers' side of it: the ``+cameras`` token at the very end of the match filter, and the calibration / distortion files it
switches to (``9 G`` numbers, G row-major matrices, then one camera index per image; none, 4 or ``4 G`` distortion coefficients)."""
from __future__ import annotations

import contextlib
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .types import Frame

CAMERAS_TOKEN = "+cameras"


def _same_K(a, b) -> bool:
    return np.asarray(a, np.float32).tobytes() == np.asarray(b, np.float32).tobytes()


def canonical_camera(frames: Sequence[Frame]) -> np.ndarray:
    """K_ref: the K_cam of the first frame with camera_id 0 (of the first frame, if no frame has id 0)."""
    for f in frames:
        if int(f.camera_id) == 0:
            return np.asarray(f.K_cam, np.float32)
    return np.asarray(frames[0].K_cam, np.float32)


def remap_keypoints(keypoints, K, K_ref) -> np.ndarray:
    """u' = (u - cx) fx_ref / fx + cx_ref, likewise v: computed in float64, rounded to float32 once.  The SAME array object comes
    back when K equals K_ref bit for bit."""
    if _same_K(K, K_ref):
        return keypoints
    kp = np.asarray(keypoints, np.float32).reshape(-1, 2).astype(np.float64)
    K = np.asarray(K, np.float32).astype(np.float64); R = np.asarray(K_ref, np.float32).astype(np.float64)
    out = np.empty_like(kp)
    out[:, 0] = (kp[:, 0] - K[0, 2]) * R[0, 0] / K[0, 0] + R[0, 2]
    out[:, 1] = (kp[:, 1] - K[1, 2]) * R[1, 1] / K[1, 1] + R[1, 2]
    return out.astype(np.float32)


@contextlib.contextmanager
def pair_stage_view(frames: Sequence[Frame]):
    """Inside the block every frame carries its canonical keypoints and K_ref; outside, its own.  Nothing is touched when all frames
    share one K_cam."""
    K_ref = canonical_camera(frames) if len(frames) else None
    if K_ref is None or all(_same_K(f.K_cam, K_ref) for f in frames):
        yield False
        return
    saved = [(f.keypoints, f.K_cam) for f in frames]
    try:
        for f in frames:
            f.keypoints = remap_keypoints(f.keypoints, f.K_cam, K_ref)
            f.K_cam = K_ref.copy()
        yield True
    finally:
        for f, (kp, K) in zip(frames, saved):
            f.keypoints, f.K_cam = kp, K


def check_one_image_size(frames: Sequence[Frame]) -> None:
    """The dense stages take one image size for all views (different intrinsics at one size are fine: they take K per view)."""
    sizes = {tuple(np.asarray(f.rgb_image).shape[:2]) for f in frames if f.rgb_image is not None}
    if len(sizes) > 1:
        raise ValueError(f"dense outputs need images of one size; this run has {sorted(sizes)}")


# ---- free radial distortion: the pinhole-equivalent pixels of detected keypoints ------------------------------------------------------
RADIAL_TOKEN = "+radial"
RADIAL_TOKEN_TOLERANCE = 1.0        # the box half width of k1, k2 the +radial token stands for: a convention, not tuned


def undistort_normalised(xd, yd, k1: float, k2: float):
    """The inverse of (x, y) -> (x, y) L(x, y), L = 1 + k1 r2 + k2 r2^2, by 20 fixed-point iterations (x, y) <- (xd, yd) / L(x, y) in
    float64 (a few thousand points per frame, on the host)."""
    xd = np.asarray(xd, np.float64); yd = np.asarray(yd, np.float64)
    x, y = xd.copy(), yd.copy()
    for _ in range(20):
        r2 = x * x + y * y
        L = 1.0 + k1 * r2 + k2 * r2 * r2
        x, y = xd / L, yd / L
    return x, y


def pinhole_keypoints(keypoints_raw, K, radial) -> np.ndarray:
    """The pixels a pinhole camera K would have seen: raw pixel -> normalised distorted point -> undistort_normalised -> pixel.
    float64 inside, float32 out.  k1 = k2 = 0: a copy of the input, bit for bit."""
    kp = np.asarray(keypoints_raw, np.float32).reshape(-1, 2)
    k1, k2 = float(radial[0]), float(radial[1])
    if k1 == 0.0 and k2 == 0.0:
        return kp.copy()
    K = np.asarray(K, np.float32).astype(np.float64)
    x, y = undistort_normalised((kp[:, 0].astype(np.float64) - K[0, 2]) / K[0, 0], (kp[:, 1].astype(np.float64) - K[1, 2]) / K[1, 1], k1, k2)
    return np.stack([x * K[0, 0] + K[0, 2], y * K[1, 1] + K[1, 2]], 1).astype(np.float32)


def refresh_pinhole_keypoints(frames: Sequence[Frame]) -> None:
    """keypoints <- pinhole_keypoints(keypoints_raw, K_cam, radial_cam) for every frame (keypoints_raw is taken from keypoints the
    first time)."""
    for f in frames:
        if f.keypoints_raw is None:
            f.keypoints_raw = np.array(f.keypoints, np.float32, copy=True).reshape(-1, 2)
        f.keypoints = pinhole_keypoints(f.keypoints_raw, f.K_cam, f.radial_cam)


def distortion_line(frames: Sequence[Frame]) -> str:
    by_id = {}
    for f in frames:
        by_id.setdefault(int(f.camera_id), f.radial_cam)
    return "Distortion: " + ", ".join(f"camera {c}: k1 [{k[0]:.6g}] k2 [{k[1]:.6g}]" for c, k in sorted(by_id.items()))


def split_radial_token(match_filter: str) -> Tuple[str, bool]:
    """(the filter without a final "+radial", whether it was there).  Called after split_cameras_token: "+radial" stands at the end of
    the filter, in front of "+cameras" if both are given."""
    if match_filter.endswith(RADIAL_TOKEN) and len(match_filter) > len(RADIAL_TOKEN):
        return match_filter[:-len(RADIAL_TOKEN)], True
    return match_filter, False


# ---- the drivers' arguments ---------------------------------------------------------------------------------------------------------
def split_cameras_token(match_filter: str) -> Tuple[str, bool]:
    """(the filter without a final "+cameras", whether it was there).  Stripped first: the rest of the token grammar is unchanged."""
    if match_filter.endswith(CAMERAS_TOKEN) and len(match_filter) > len(CAMERAS_TOKEN):
        return match_filter[:-len(CAMERAS_TOKEN)], True
    return match_filter, False


def parse_camera_file(text: str, n_images: int) -> Tuple[np.ndarray, np.ndarray]:
    """The calibration file of a +cameras run: 9 G numbers (G row-major 3 x 3 matrices) followed by one camera index per image of the
    image list, exactly 9 G + N numbers with every index in [0, G).  Returns (K [G, 3, 3] float32, camera_of_image [N] int32)."""
    tokens = text.split()
    try:
        vals = [float(t) for t in tokens]
    except ValueError as e:
        raise ValueError(f"camera file: not a number: {e}") from None
    n_k = len(vals) - n_images
    if n_k < 9 or n_k % 9 != 0:
        raise ValueError(f"camera file: {len(vals)} numbers for {n_images} images; expected 9 G + {n_images} (G matrices, then one camera index per image)")
    G = n_k // 9
    idx = vals[n_k:]
    for v in idx:
        if v != int(v) or not 0 <= int(v) < G:
            raise ValueError(f"camera file: camera index {v:g} is not an integer in [0, {G})")
    return np.array(vals[:n_k], np.float32).reshape(G, 3, 3), np.array([int(v) for v in idx], np.int32)


def parse_camera_distort(text: Optional[str], n_cameras: int) -> np.ndarray:
    """The distortion file of a +cameras run: None (no file: zeros), 4 numbers (all cameras) or 4 G (per camera).  Returns [G, 4]
    float64 in the reference's storage (features.import_distort: the floats' bits in the first 16 bytes of the double matrix)."""
    out = np.zeros((n_cameras, 4), np.float64)
    if text is None:
        return out
    try:
        vals = [float(t) for t in text.split()]
    except ValueError as e:
        raise ValueError(f"distortion file: not a number: {e}") from None
    if len(vals) not in (4, 4 * n_cameras):
        raise ValueError(f"distortion file: {len(vals)} numbers; expected 4 (all cameras) or {4 * n_cameras} (4 per camera)")
    for g in range(n_cameras):
        v = vals[4 * g:4 * g + 4] if len(vals) == 4 * n_cameras else vals[:4]
        out[g].view(np.float32)[:4] = np.asarray(v, np.float32)
    return out


def cameras_line(camera_of_image, n_cameras: int) -> str:
    counts = np.bincount(np.asarray(camera_of_image, np.int64), minlength=n_cameras)
    return f"Cameras: {n_cameras} models, " + " / ".join(str(int(c)) for c in counts) + " images"
