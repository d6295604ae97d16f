"""Cameras, images and small meshes shared by the mesh-texturing tests (tests/test_mesh_texture_cpu.py, _gpu.py)."""
import os

import numpy as np

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def arc_views(n, rows, cols, centre, distance, focal, span_deg=40.0):
    """n cameras on a horizontal arc of span_deg degrees around `centre`, looking at it from `distance`: (K4 [n, 4], poses
    [n, 12]) in f32, built like tests/mvs_scene.py's."""
    poses = []
    for a in np.deg2rad(np.linspace(-span_deg / 2, span_deg / 2, n)):
        C = np.asarray(centre, np.float64) + distance * np.array([np.sin(a), 0.0, -np.cos(a)])
        R = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
        poses.append(np.concatenate([R, (-R @ C)[:, None]], axis=1).reshape(12))
    K4 = np.tile(np.array([focal, (cols - 1) / 2.0, focal, (rows - 1) / 2.0], F), (n, 1))
    return K4, np.stack(poses).astype(F)


def noise_images(n, rows, cols, channels, seed=3):
    """Seeded u8 noise: every bilinear weight meets unrelated neighbours, so a wrong tap or operation order shows."""
    shape = (n, rows, cols) if channels == 1 else (n, rows, cols, 3)
    return np.random.default_rng(seed).integers(0, 256, shape).astype(np.uint8)


def quad(x0, x1, y0, y1, z, first=0):
    """Two triangles facing -z (towards a camera at the origin looking along +z with y down): (vertices [4, 3], triangles [2, 3])."""
    v = np.array([[x0, y0, z], [x1, y0, z], [x1, y1, z], [x0, y1, z]], F)
    t = np.array([[0, 2, 1], [0, 3, 2]], np.int32) + first
    return v, t


def front_camera(rows, cols, focal):
    """One camera at the origin looking along +z: (K4 [1, 4], poses [1, 12])."""
    K4 = np.array([[focal, (cols - 1) / 2.0, focal, (rows - 1) / 2.0]], F)
    return K4, np.array([[1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]], F)


def big_triangle_scene(rows=64, cols=96, focal=60.0, n_small=300, seed=5):
    """One triangle at z = 2 whose projection covers the whole image, and n_small small ones scattered behind it at z = 3..4, all
    facing the front camera."""
    rng = np.random.default_rng(seed)
    v = [np.array([[-6.0, -4.0, 2.0], [6.0, -4.0, 2.0], [0.0, 8.0, 2.0]], F)]
    t = [np.array([[0, 2, 1]], np.int32)]
    for k in range(n_small):
        c = np.array([rng.uniform(-1.5, 1.5), rng.uniform(-1.0, 1.0), rng.uniform(3.0, 4.0)])
        d = rng.uniform(0.02, 0.15, 2)
        v.append((c + np.array([[0, 0, 0], [d[0], 0, 0.01], [0, d[1], -0.01]])).astype(F))
        t.append(np.array([[0, 2, 1]], np.int32) + 3 * (k + 1))
    return np.concatenate(v), np.concatenate(t)


def lane_limit_scene():
    """Right triangles at z = 64 under front_camera(64, 96, 64.0) -- one pixel per unit, exact in f32 -- whose boxes hold 56, 64,
    72 and 81 pixels: on both sides of the 64 pixels up to which one lane walks a box alone.  They face the camera and overlap."""
    v, t = [], []
    for k, (w, h) in enumerate(((6, 7), (7, 7), (8, 7), (7, 8), (8, 8), (7, 7), (8, 7))):
        x0, y0, z = -40.25 + 9 * k, -20.25 + 4 * k, 64.0 + k
        v.append(np.array([[x0, y0, z], [x0 + w, y0, z], [x0, y0 + h, z]], F) * F([z / 64.0, z / 64.0, 1]))
        t.append(np.array([[0, 2, 1]], np.int32) + 3 * k)
    return np.concatenate(v), np.concatenate(t)


def occlusion_share(scene, mvs_scene, vertices, triangles, label):
    """(share of labelled triangles whose centroid the true surface hides by more than 2 % in their chosen view, share of
    triangles that are labelled)."""
    v, t = np.asarray(vertices, np.float64), np.asarray(triangles)
    G = v[t].mean(axis=1)
    hidden = np.zeros(len(t), bool)
    for view in range(len(scene["poses"])):
        m = label == view
        if m.any():
            ray, own = mvs_scene.ray_depth(scene, view, G[m])
            hidden[m] = (own - ray) > 0.02 * ray
    labelled = label >= 0
    return float(hidden[labelled].mean()) if labelled.any() else 0.0, float(labelled.mean())


def fidelity(mvs_scene, texture_ref, vertices, rgb, triangles, label, atlas, texels, atlas_width):
    """Over the texels that lie inside their chart and belong to a labelled triangle: (mean |atlas grey level - true texture at the
    texel's world point|, the same for the barycentric mix of the vertex colours, the number of texels)."""
    v, t, S = np.asarray(vertices, np.float64), np.asarray(triangles), int(texels)
    H, W = atlas.shape[:2]
    Y, X = np.mgrid[0:H, 0:W]
    i, j = X % S, Y % S
    tri = 2 * (Y // S * atlas_width + X // S) + texture_ref.texel_owner(S)[j, i]
    b = [c[j, i].astype(np.float64) for c in texture_ref.texel_barycentrics(S)]
    tc = np.where(tri < len(t), tri, 0)
    m = (tri < len(t)) & (label[tc] >= 0) & (b[0] >= 0) & (b[1] >= 0) & (b[2] >= 0)
    c = t[tc[m]]
    w = [x[m][:, None] for x in b]
    Xw = w[0] * v[c[:, 0]] + w[1] * v[c[:, 1]] + w[2] * v[c[:, 2]]
    truth = mvs_scene.texture(Xw)
    col = np.asarray(rgb, np.float64)
    mix = (w[0] * col[c[:, 0]] + w[1] * col[c[:, 1]] + w[2] * col[c[:, 2]])[:, 0]
    baked = atlas[..., 0][m].astype(np.float64)
    return float(np.abs(baked - truth).mean()), float(np.abs(mix - truth).mean()), int(m.sum())


def far_grid():
    """4 x 4 quads on the plane z = 4 over x in [-2, 2], y in [-1.5, 1.5]: 32 triangles, all inside the 64 x 96 image."""
    vs, ts = [], []
    for r in range(4):
        for c in range(4):
            v, t = quad(-2.0 + c, -1.0 + c, -1.5 + 0.75 * r, -0.75 + 0.75 * r, 4.0, first=4 * len(vs))
            vs.append(v); ts.append(t)
    return np.concatenate(vs), np.concatenate(ts)


# The figures of the chain mesh under the scene's five views (the head comment of tests/test_mesh_texture_cpu.py says how they arose).
REF_LABELLED, REF_HIDDEN = 0.9925, 0.0081
REF_ATLAS_ERROR, REF_VERTEX_ERROR = 2.999, 4.801
MAX_HIDDEN, MIN_LABELLED = 0.01, 0.90                      # the conditions the defaults must meet
MAX_ATLAS_ERROR = 1.5 * REF_ATLAS_ERROR


def chain_mesh():
    z = np.load(os.path.join(ROOT, "tests", "golden", "texture_chain_mesh.npz"))
    return z["vertices"], z["rgb"], z["triangles"]


def check_chain(v, rgb, t, label, score, atlas, S_, A, scene):
    """The two scene figures, printed and held against the recorded ones (the CPU test on the restatement, the GPU test)."""
    import mvs_scene
    import texture_ref
    hidden, labelled = occlusion_share(scene, mvs_scene, v, t, label)
    atlas_err, vertex_err, n = fidelity(mvs_scene, texture_ref, v, rgb, t, label, atlas, S_, A)
    print(f"chain: {len(t)} triangles, {labelled:.4f} labelled, {hidden:.4f} of them hidden by more than 2 %; S = {S_}, atlas {atlas.shape[1]} x "
          f"{atlas.shape[0]}; {n} chart texels: atlas error {atlas_err:.3f}, vertex-colour error {vertex_err:.3f}")
    assert hidden <= MAX_HIDDEN and labelled >= MIN_LABELLED
    assert atlas_err < vertex_err and atlas_err <= MAX_ATLAS_ERROR
