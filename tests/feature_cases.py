"""Input images shared by the ORB / SURF / SIFT reference tests (tests/test_orb_ref_cpu.py, tests/test_surf_ref_cpu.py,
tests/test_sift_ref_cpu.py, tests/test_feature_ref_gpu.py): one crop of a committed fixture and seeded synthetic images, the
smallest that reach every rule of the detectors.  Every case is (name, BGR image, parameter); the gray form of a case is the 14-bit BGR2GRAY of its BGR
form, taken by the reference under test, so both forms of a case describe the same picture."""
import functools
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _bgr_of(gray, rng):
    """A colour image whose channels differ (so the gray weights matter) around the given picture."""
    g = gray.astype(np.int64)
    return np.clip(np.stack([g + rng.integers(-12, 13, g.shape), g + rng.integers(-3, 4, g.shape), g + rng.integers(-9, 10, g.shape)], axis=2),
                   0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def fountain_crop():
    """256 x 320 BGR crop of the half-resolution fountain view: all eight ORB levels stay larger than their border."""
    return np.ascontiguousarray(np.load(os.path.join(GOLD, "fountain_pair_half.npz"))["img0"][:, 32:352])


@functools.lru_cache(maxsize=None)
def blocks(rows, cols, seed, cell=4, noise=8):
    """Random cell x cell blocks plus noise: corners everywhere (the texture tests/test_orb_gpu.py uses for its small images)."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, ((rows + cell - 1) // cell, (cols + cell - 1) // cell))
    img = np.kron(base, np.ones((cell, cell), np.int64))[:rows, :cols] + rng.integers(-noise, noise + 1, (rows, cols))
    return _bgr_of(np.clip(img, 0, 255), rng)


@functools.lru_cache(maxsize=None)
def blobs(rows, cols, seed, n_blobs, sigma_lo=1.5, sigma_hi=14.0, noise=1.0, border=False):
    """Gaussian blobs of both signs on a flat ground; sigma up to 14 px puts maxima into all four SURF octaves.  With border=True
    the centres lie within 14 px of an image edge, so the keypoints found sit as close to the border as the detector allows."""
    rng = np.random.default_rng(seed)
    img = np.full((rows, cols), 120.0)
    yy, xx = np.mgrid[0:rows, 0:cols]
    for k in range(n_blobs):
        if border:
            side = k % 4
            t = rng.uniform(10.0, 14.0)
            cy, cx = ((t, rng.uniform(0, cols)), (rows - 1 - t, rng.uniform(0, cols)), (rng.uniform(0, rows), t), (rng.uniform(0, rows), cols - 1 - t))[side]
            sg = rng.uniform(1.8, 3.0)
        else:
            cy, cx = rng.uniform(0, rows), rng.uniform(0, cols)
            sg = float(np.exp(rng.uniform(np.log(sigma_lo), np.log(sigma_hi))))
        amp = rng.uniform(40, 90) * (1 if rng.random() < 0.5 else -1)
        img += amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sg * sg))
    img += rng.normal(0, noise, img.shape)
    return _bgr_of(np.clip(np.rint(img), 0, 255), rng)


def checker(rows=168, cols=168, cell=8):
    """A periodic picture: cell x cell squares whose gray value steps with ((i mod 4) + 4 (j mod 4)) -- 16 distinct steps repeating
    every 32 px -- plus a seeded dither of the same period.  Without the dither the FAST score is flat around every junction and the
    strict 3 x 3 maximum keeps nothing; with it every period holds the same corners, with the same FAST score and the same Harris sums."""
    i, j = np.mgrid[0:rows, 0:cols]
    # a permutation of 0..15 so neighbouring squares differ by far more than the FAST threshold
    perm = np.array([0, 9, 3, 12, 14, 5, 10, 1, 7, 15, 4, 11, 8, 2, 13, 6])
    dither = np.random.default_rng(8).integers(0, 7, (4 * cell, 4 * cell))
    return (20 + 14 * perm[((i // cell) % 4) * 4 + (j // cell) % 4] + dither[i % (4 * cell), j % (4 * cell)]).astype(np.uint8)


def white_noise(rows, cols, seed):
    """Independent uniform pixels: a SURF maximum of the finest layers at about every 28th pixel once the threshold is near zero."""
    return np.random.default_rng(seed).integers(0, 256, (rows, cols), dtype=np.uint8)


ORB_CASES = [  # (name, BGR image, nfeatures)
    ("fountain256x320", fountain_crop, 500),
    ("blocks97x131", lambda: blocks(97, 131, 3), 300),
]

SURF_CASES = [  # (name, BGR image, hessian threshold)
    ("fountain256x320", fountain_crop, 300.0),
    ("blobs240x320", lambda: blobs(240, 320, 0, 260), 60.0),
    ("blobs33x40", lambda: blobs(33, 40, 3, 10, 1.5, 3.0), 10.0),
    ("border150x203", lambda: blobs(150, 203, 5, 48, border=True), 60.0),
]


def single_blob(side, ground, sigma, cx, cy):
    """One Gaussian blob of height 150 on a flat ground, rounded to uint8."""
    y, x = np.mgrid[0:side, 0:side].astype(np.float64)
    return np.rint(ground + 150 * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * sigma * sigma))).astype(np.uint8)


def blob11_symmetric():
    """11 x 11, centred exactly on pixel (5, 5): its keypoint lies in the octave of side 11, whose only searchable position is
    (5, 5).  The picture equals its own transpose, so whole diagonals of orientation samples have |dx| = |dy| exactly, where
    cv::fastAtan2 jumps from 44.990 to 45.010 degrees across a bin edge: which peaks exist turns on float32 round-off alone."""
    return single_blob(11, 100, 2.5, 5.0, 5.0)


def _gray3(gray):
    return np.repeat(gray[:, :, None], 3, axis=2)             # 1868 + 9617 + 4899 = 2^14: the gray of (g, g, g) is g


SIFT_CASES = [  # (name, BGR image, keypoints the CPU restatement returns)
    ("fountain256x320", fountain_crop, 299),                                          # octaves -1..4
    ("blobs240x320", lambda: blobs(240, 320, 0, 260), 197),                           # five octaves
    ("blobs33x40", lambda: blobs(33, 40, 3, 10, 1.5, 3.0), 7),                        # smallest general picture
    # orientation discs and descriptor windows that leave the image.  Seed 9, not SURF's 5: with seed 5 three of 61 keypoints
    # (4.9 %) turn on a decision within the float32 bound, above the cap of the reference tests
    ("border150x203", lambda: blobs(150, 203, 9, 48, border=True), 72),
    ("checker168", lambda: _gray3(checker()), 537),                                   # massive ties: 488 share a response
    # an octave with one searchable position.  blob11_symmetric moved off its axes of symmetry (see there): 2 orientations
    ("blob11", lambda: _gray3(single_blob(11, 100, 2.5, 5.1, 4.95)), 2),
    ("blob24", lambda: _gray3(single_blob(24, 60, 4.0, 11.8, 12.3)), 5),              # descriptor radius 36 clipped to the diagonal 33
]
