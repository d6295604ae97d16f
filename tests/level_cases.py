"""Scenes and measures shared by the seam-levelling tests (tests/test_mesh_texture_level_cpu.py, _gpu.py)."""
import numpy as np

import level_ref as L
import texture_cases as TC

F = np.float32
ROWS, COLS, FOCAL = 64, 96, 60.0
GAIN = (0.9, 1.05, 1.0, 0.95, 1.1)
OFFSET = (-24.0, 12.0, 0.0, -12.0, 24.0)


def exposure_images(images):
    """The scene's views as five cameras with different exposures would record them: clip(rint(gain I + offset))."""
    I = np.asarray(images, np.float64)
    shape = (len(I),) + (1,) * (I.ndim - 1)
    return np.clip(np.rint(np.reshape(GAIN[:len(I)], shape) * I + np.reshape(OFFSET[:len(I)], shape)), 0, 255).astype(np.uint8)


def welded(v, t):
    """The mesh with equal positions merged into one vertex (tests/texture_cases.py builds its grids quad by quad)."""
    u, inverse = np.unique(np.asarray(v, F), axis=0, return_inverse=True)
    return np.ascontiguousarray(u, F), np.ascontiguousarray(inverse.reshape(-1)[np.asarray(t)], np.int32)


def front_cameras(n, rows=ROWS, cols=COLS, focal=FOCAL):
    K4, P = TC.front_camera(rows, cols, focal)
    return np.tile(K4, (n, 1)), np.tile(P, (n, 1))


def flat_images(levels, rows=ROWS, cols=COLS):
    return np.stack([np.full((rows, cols), g, np.uint8) for g in levels])


def two_halves():
    """The welded far grid (25 vertices, 32 triangles), its left 16 triangles labelled view 0 and its right 16 view 1, under two
    identical front cameras whose images are flat 100 and 140: (v, t, label, images, K4, P)."""
    v, t = welded(*TC.far_grid())
    label = (v[t][:, :, 0].mean(axis=1) > 0).astype(np.int32)
    K4, P = front_cameras(2)
    return v, t, label, flat_images((100, 140)), K4, P


def striped(n_views, channels, seed=3):
    """The welded far grid with one label per column of quads, cycling through n_views views, and noise images."""
    v, t = welded(*TC.far_grid())
    column = np.floor(v[t][:, :, 0].mean(axis=1) + 2.0).astype(np.int32)
    K4, P = front_cameras(n_views)
    return v, t, (column % n_views).astype(np.int32), TC.noise_images(n_views, ROWS, COLS, channels, seed), K4, P


def _fan(centre, n, first):
    a = 2 * np.pi * np.arange(n) / n
    v = np.concatenate([[[centre[0], centre[1], 4.0]], np.stack([centre[0] + np.cos(a), centre[1] + np.sin(a), np.full(n, 4.0)], 1)]).astype(F)
    t = np.array([[0, 1 + k, 1 + (k + 1) % n] for k in range(n)], np.int32) + first
    return v, t


def fan():
    """Two fans: six triangles around vertex 0 with labels 0 0 1 1 2 2, eight around vertex 7 with labels 0 0 1 1 2 2 3 3.  The
    centres have three and four nodes; every second rim vertex lies between two labels.  28 nodes, 9 seam vertices."""
    v1, t1 = _fan((-1.2, 0.0), 6, 0)
    v2, t2 = _fan((1.2, 0.0), 8, len(v1))
    label = np.array([0, 0, 1, 1, 2, 2, 0, 0, 1, 1, 2, 2, 3, 3], np.int32)
    K4, P = front_cameras(4)
    return np.concatenate([v1, v2]), np.concatenate([t1, t2]), label, TC.noise_images(4, ROWS, COLS, 3, seed=5), K4, P


def degenerate_mix():
    """The striped grid with every fifth triangle unlabelled, then two triangles with a repeated index, one labelled triangle with a
    vertex behind its view (and so left out entirely) and one that reaches out of the plane to a vertex at z = 2."""
    v, t, label, images, K4, P = striped(2, 3, seed=9)
    label = label.copy()
    label[::5] = -1
    n = len(v)
    v = np.concatenate([v, np.array([[0.3, 0.2, -1.0], [0.1, -0.4, 2.0]], F)])
    t = np.concatenate([t, np.array([[0, 0, 6], [7, 12, 12], [5, 6, n], [11, 12, n + 1]], np.int32)])
    label = np.concatenate([label, np.array([0, 1, 0, 1], np.int32)])
    return v, t, label, images, K4, P


def plane_grid(n=260, stripes=13, channels=1, seed=11):
    """n x n vertices on the plane z = 4 over x in [-3, 3], y in [-2, 2] (inside the 64 x 96 image), 2 (n - 1)^2 triangles, labels in
    column stripes that alternate between two front cameras, noise images."""
    x, y = np.meshgrid(np.linspace(-3, 3, n), np.linspace(-2, 2, n))
    v = np.stack([x.reshape(-1), y.reshape(-1), np.full(n * n, 4.0)], 1).astype(F)
    r, c = np.mgrid[0:n - 1, 0:n - 1]
    i = (r * n + c).reshape(-1)
    t = np.concatenate([np.stack([i, i + n + 1, i + 1], 1), np.stack([i, i + n, i + n + 1], 1)]).astype(np.int32)
    label = ((c.reshape(-1) * stripes // (n - 1)) % 2).astype(np.int32)
    K4, P = front_cameras(2)
    return v, t, np.concatenate([label, label]), TC.noise_images(2, ROWS, COLS, channels, seed), K4, P


def node_values(nt, offsets, samples):
    """(f, g) [N, 3] f64 of the nodes, gathered from the per-corner outputs with the restatement's node table."""
    f, g = np.zeros((nt["nodes"], 3)), np.zeros((nt["nodes"], 3))
    part = nt["part"]
    f[nt["corner_node"][part]] = np.asarray(samples, np.float64)[part]
    g[nt["corner_node"][part]] = np.asarray(offsets, np.float64)[part]
    return f, g


def seam_step(nt, offsets, samples):
    """The mean over seam pairs and channels of |f_a + g_a - f_b - g_b| (0 without a seam)."""
    f, g = node_values(nt, offsets, samples)
    c = f + g
    total, count = 0.0, 0
    for j in range(nt["seam"].shape[1]):
        m = nt["seam_n"] > j
        total += np.abs(c[m] - c[nt["seam"][m, j]]).sum()
        count += 3 * int(m.sum())
    return total / count if count else 0.0


def check_level_chain(v, rgb, t, label, score, images, K4, P, plain, levelled, offsets, samples, scene):
    """The chain conditions on the scene's own images (the CPU test on the restatement, the GPU test): labels and shares as before,
    the levelled atlas within the texturing's error bound, the seam step not larger than before.  Returns (before, after, plain
    error, levelled error)."""
    import mvs_scene
    import texture_ref
    nt = L.node_table(v, t, label, images, K4, P)
    before, after = seam_step(nt, np.zeros_like(offsets), samples), seam_step(nt, offsets, samples)
    TC.check_chain(v, rgb, t, label, score, plain, 4, 32, scene)
    TC.check_chain(v, rgb, t, label, score, levelled, 4, 32, scene)
    e0 = TC.fidelity(mvs_scene, texture_ref, v, rgb, t, label, plain, 4, 32)[0]
    e1 = TC.fidelity(mvs_scene, texture_ref, v, rgb, t, label, levelled, 4, 32)[0]
    print(f"level, scene images: seam step {before:.3f} -> {after:.3f}, atlas error {e0:.3f} -> {e1:.3f}")
    assert after <= before and e1 <= TC.MAX_ATLAS_ERROR
    return before, after, e0, e1


def check_level_exposure(v, rgb, t, label, images, K4, P, plain, levelled, offsets, samples, stats):
    """The chain conditions under the exposure images: the step falls to a tenth, the atlas error to a half, the solve converges."""
    import mvs_scene
    import texture_ref
    nt = L.node_table(v, t, label, images, K4, P)
    before, after = seam_step(nt, np.zeros_like(offsets), samples), seam_step(nt, offsets, samples)
    e0 = TC.fidelity(mvs_scene, texture_ref, v, rgb, t, label, plain, 4, 32)[0]
    e1 = TC.fidelity(mvs_scene, texture_ref, v, rgb, t, label, levelled, 4, 32)[0]
    print(f"level, exposure images: seam step {before:.3f} -> {after:.3f}, atlas error {e0:.3f} -> {e1:.3f}, {stats['iterations']} iterations")
    assert after <= 0.1 * before and e1 <= 0.5 * e0 and stats["converged"] == 1
    return before, after, e0, e1
