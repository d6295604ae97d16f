"""Inputs of the image-retrieval tests: the descriptor-only corridor scene and small descriptor sets at the kernels' edges."""
import numpy as np


def _unit(x):
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


def corridor(seed, n_images=24, step=20, span=200, dim=64, keep=0.9, noise=0.03, clutter=100):
    """A camera walks down a corridor and returns to its start.  A pool of step * n_images + span scene points, each with a random
    unit descriptor; image i sees points [step w, step w + span) with w = i, except the last two images, which revisit w = 0 and 1
    (the loop closure); each point is kept with probability `keep`, its descriptor gets Gaussian noise `noise` and is
    re-normalised; `clutter` rows of fresh random unit vectors are added and the rows are shuffled.
    Returns (sets: float32 [rows, dim] per image, ids: the scene points each image kept, as sorted int arrays)."""
    rng = np.random.default_rng(seed)
    pool = _unit(rng.normal(size=(step * n_images + span, dim)))
    sets, ids = [], []
    for i in range(n_images):
        w = i if i < n_images - 2 else i - (n_images - 2)
        seen = np.arange(step * w, step * w + span)
        seen = seen[rng.random(span) < keep]
        rows = _unit(pool[seen] + rng.normal(scale=noise, size=(len(seen), dim)))
        rows = np.concatenate([rows, _unit(rng.normal(size=(clutter, dim)))])
        sets.append(np.ascontiguousarray(rows[rng.permutation(len(rows))]))
        ids.append(seen)
    return sets, ids


def shared_points(ids):
    """[n, n] number of scene points two images both kept"""
    n = len(ids)
    return np.array([[len(np.intersect1d(ids[i], ids[j])) for j in range(n)] for i in range(n)])


def check_corridor(nearest, scores, ids):
    """the two conditions of the corridor scene on a nearest table; returns (selected neighbours, those sharing no scene point)"""
    shared = shared_points(ids)
    chosen = [(i, int(j)) for i in range(len(ids)) for j in nearest[i] if j >= 0]
    none = [(i, j) for i, j in chosen if shared[i, j] == 0]
    assert len(chosen) == nearest.size                       # 24 images with 4 neighbours each: no padding
    assert not none, none                                    # a cap of 0, not a measured number
    assert 1 in nearest[len(ids) - 1]                        # the loop closure: image 23 revisits image 1's window
    return len(chosen), len(none)


def float_sets(n_sets, width, seed, rows=(40, 70), empty=None, single=None, long=None):
    """n_sets float32 sets of `rows` rows each, clustered (noisy re-observations of 12 anchors plus uniform rows) so that k-means has
    something to find; set `empty` has 0 rows, set `single` 1 row, set `long` 1100 rows (more than one accumulation workgroup)."""
    rng = np.random.default_rng(seed)
    anchors = rng.normal(size=(12, width))
    sets = []
    for s in range(n_sets):
        n = int(rng.integers(rows[0], rows[1] + 1))
        n = 0 if s == empty else 1 if s == single else 1100 if s == long else n
        pick = rng.integers(0, 12, n)
        x = anchors[pick] * rng.uniform(0.5, 1.5, (n, 1)) + rng.normal(scale=0.2, size=(n, width))
        sets.append(np.ascontiguousarray(x, np.float32))
    return sets


def identical_rows_case(seed=5, width=8):
    """six images: image 4 is a copy of image 2 (equal scores must rank by index); every row of image 3 is the same vector, far from
    the others and exact in 16.16 fixed point, so that it forms a cluster of its own whose centre is that vector: S = 0, norm2 = 0"""
    sets = float_sets(6, width, seed, rows=(48, 48))
    sets[4] = sets[2].copy()
    sets[3] = np.full((48, width), 40.5, np.float32)
    return sets


def one_hot_vlads(n=33, D=200):
    """int8 rows with one or two non-zero entries, spread over every 16-byte lane group of the i8 matrix instruction's 64-wide
    steps; rows i and i + 20 share their first position (non-zero dots off the diagonal), the values differ per row"""
    V = np.zeros((n, D), np.int8)
    for i in range(n):
        V[i, (37 * (i % 20) + 5) % D] = (i % 7) + 1 if i % 2 else -((i % 7) + 1)
        if i % 3 == 0:
            V[i, (11 * i + 64) % D] += 3
    return V
