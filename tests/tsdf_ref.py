"""numpy restatement of include/esfm.h, "Surface reconstruction": the integration of depth maps into a truncated signed
distance volume and the marching-tetrahedra extraction of an indexed triangle mesh.  Every f32 formula keeps the header's
operation order (numpy's f32 +, -, *, / and sqrt are correctly rounded and never contracted), so the GPU is compared with this
bit for bit.  The winding table is computed here from the header's integer rule, not copied from the product.  Volumes are
arrays of shape (nz, ny, nx): their C order is the header's linear index (k ny + j) nx + i."""
import itertools

import numpy as np

F = np.float32
PERMS = list(itertools.permutations(range(3)))                # lexicographic: xyz, xzy, yxz, yzx, zxy, zyx


class Rejected(ValueError):
    pass


def check_grid(origin, h, dims, trunc=0.0, min_weight=2):
    if not np.all(np.isfinite(np.asarray(origin, F))) or not (np.isfinite(F(h)) and F(h) > 0):
        raise Rejected("grid")
    if any(d < 2 or d > 1024 for d in dims) or int(dims[0]) * int(dims[1]) * int(dims[2]) > 2 ** 27:
        raise Rejected("dims")
    if F(trunc) != 0 and not (np.isfinite(F(trunc)) and F(trunc) >= F(h)):
        raise Rejected("trunc")
    if min_weight < 1:
        raise Rejected("min_weight")


def centres(origin, h, dims):
    """Voxel centres per axis, broadcastable over (nz, ny, nx): X_a = origin_a + ((float)i_a + 0.5f) * h."""
    nx, ny, nz = dims
    ax = [F(origin[a]) + (np.arange(n, dtype=F) + F(0.5)) * F(h) for a, n in enumerate((nx, ny, nz))]
    return ax[0].reshape(1, 1, nx), ax[1].reshape(1, ny, 1), ax[2].reshape(nz, 1, 1)


def integrate(images, K4, poses, depth, origin, h, dims, trunc=0.0):
    """esfm_tsdf_integrate.  images [n, rows, cols(, 1 | 3)] u8 (BGR or grey) or None.  Returns (tsdf f32, weight i32, rgb u8 or
    None), each (nz, ny, nx[, 3])."""
    check_grid(origin, h, dims, trunc)
    nx, ny, nz = dims
    depth = np.asarray(depth, F)
    n, rows, cols = depth.shape
    K4 = np.asarray(K4, F).reshape(n, 4)
    poses = np.asarray(poses, F).reshape(n, 12)
    tr = F(4.0) * F(h) if F(trunc) == 0 else F(trunc)
    X0, X1, X2 = centres(origin, h, dims)
    shape = (nz, ny, nx)
    S = np.zeros(shape, F)
    W = np.zeros(shape, np.int32)
    if images is not None:
        images = np.asarray(images, np.uint8).reshape(n, rows, cols, -1)
        csum = np.zeros(shape + (3,), np.int32)
        Wc = np.zeros(shape, np.int32)
    for v in range(n):
        if not np.any(depth[v] > 0):
            continue
        P = poses[v]
        fx, cx, fy, cy = K4[v]
        with np.errstate(all="ignore"):
            p = [np.broadcast_to(((P[4 * i] * X0 + P[4 * i + 1] * X1) + P[4 * i + 2] * X2) + P[4 * i + 3], shape) for i in range(3)]
            ok = p[2] > 0
            u = fx * (p[0] / p[2]) + cx
            w = fy * (p[1] / p[2]) + cy
            px, py = np.floor(u + F(0.5)), np.floor(w + F(0.5))
            ok &= (px >= 0) & (px < F(cols)) & (py >= 0) & (py < F(rows))
            ix = np.where(ok, px, 0).astype(np.int64)
            iy = np.where(ok, py, 0).astype(np.int64)
            d = depth[v][iy, ix]
            ok &= d > 0
            s = d - p[2]
            ok &= ~(s < -tr)
            term = np.minimum(F(1.0), s / tr)
        assert term.dtype == F
        S[ok] = S[ok] + term[ok]
        W[ok] += 1
        if images is not None:
            c = ok & (s <= tr)
            pix = images[v][iy[c], ix[c]].astype(np.int32)
            csum[c] += pix[:, ::-1] if pix.shape[1] == 3 else np.repeat(pix, 3, axis=1)
            Wc[c] += 1
    with np.errstate(all="ignore"):
        tsdf = np.where(W > 0, S / np.maximum(W, 1).astype(F), F(1.0)).astype(F)
    rgb = None
    if images is not None:
        den = np.maximum(Wc, 1)[..., None]
        rgb = np.where(Wc[..., None] > 0, (csum + (Wc // 2)[..., None]) // den, 0).astype(np.uint8)
    return tsdf, W, rgb


def tet_corners(t):
    """The ordered corners q0..q3 of tetrahedron t as lattice vectors."""
    a, b, _ = PERMS[t]
    q = np.zeros((4, 3), np.int64)
    q[1, a] = 1
    q[2] = q[1]
    q[2, b] = 1
    q[3] = 1
    return q


def tet_triangles(t, m):
    """Triangles of tetrahedron t with inside mask m (bit l = local corner l inside): a list of triangles, each three edges as
    pairs of local corners, wound by the integer rule."""
    q = tet_corners(t)
    ins = [l for l in range(4) if m >> l & 1]
    out = [l for l in range(4) if not m >> l & 1]
    if not ins or not out:
        return []
    if len(ins) == 2:
        (a, b), (c, d) = ins, out
        tris = [[(a, c), (a, d), (b, d)], [(a, c), (b, d), (b, c)]]
    else:
        a = ins[0] if len(ins) == 1 else out[0]
        tris = [[(a, o) for o in (out if len(ins) == 1 else ins)]]
    s = len(ins) * q[out].sum(0) - len(out) * q[ins].sum(0)
    wound = []
    for tri in tris:
        mid = [q[e[0]] + q[e[1]] for e in tri]
        ns = int(np.dot(np.cross(mid[1] - mid[0], mid[2] - mid[0]), s))
        assert ns != 0
        wound.append(tri if ns > 0 else [tri[0], tri[2], tri[1]])
    return wound


def _shifted(a, dx, dy, dz, fill=False):
    """a at (i + dx, j + dy, k + dz) for offsets in {0, 1}; `fill` outside the grid."""
    nz, ny, nx = a.shape
    out = np.full(a.shape, fill, a.dtype)
    out[:nz - dz, :ny - dy, :nx - dx] = a[dz:, dy:, dx:]
    return out


def gradient(tsdf, valid):
    """Per voxel and axis: central difference where both axis neighbours are in the grid and valid, one-sided with one, else 0.
    Returns [nz, ny, nx, 3] f32 (x, y, z)."""
    g = np.zeros(tsdf.shape + (3,), F)
    for x, axis in enumerate((2, 1, 0)):
        f = np.moveaxis(tsdf, axis, 0)
        ok = np.moveaxis(valid, axis, 0)
        fp, fm = np.zeros_like(f), np.zeros_like(f)
        hi, lo = np.zeros(f.shape, bool), np.zeros(f.shape, bool)
        fp[:-1], hi[:-1] = f[1:], ok[1:]
        fm[1:], lo[1:] = f[:-1], ok[:-1]
        with np.errstate(all="ignore"):
            ga = np.where(hi & lo, F(0.5) * (fp - fm), np.where(hi, fp - f, np.where(lo, f - fm, F(0.0)))).astype(F)
        np.moveaxis(g[..., x], axis, 0)[...] = ga
    return g


def extract(tsdf, weight, rgb, origin, h, min_weight=2, return_cases=False):
    """esfm_tsdf_extract on a volume of shape (nz, ny, nx).  Returns (vertices [V, 3] f32, normals [V, 3] f32, vertex_rgb [V, 3] u8
    or None, triangles [T, 3] i32); with return_cases also the set of (tetrahedron, mask) pairs that emitted a triangle."""
    tsdf = np.asarray(tsdf, F)
    weight = np.asarray(weight, np.int32)
    nz, ny, nx = tsdf.shape
    check_grid(origin, h, (nx, ny, nz), 0.0, min_weight)
    h = F(h)
    valid = weight >= min_weight
    inside = valid & (tsdf < 0)
    live = np.ones((nz, ny, nx), bool)                          # by origin voxel; no cell starts in the last layer of an axis
    for dz, dy, dx in itertools.product((0, 1), repeat=3):
        live &= _shifted(valid, dx, dy, dz)
    lin = np.arange(nz * ny * nx, dtype=np.int64).reshape(nz, ny, nx)

    # used edges: a sign change and a live cell that holds both ends (a gather)
    keys = []
    for e in range(7):
        dx, dy, dz = (e + 1) & 1, (e + 1) >> 1 & 1, (e + 1) >> 2
        any_live = live.copy()
        for axis, delta in ((2, dx), (1, dy), (0, dz)):
            if not delta:                                       # the cell may also start one voxel lower along this axis
                lower = np.zeros_like(any_live)
                sl = [slice(None)] * 3
                src = list(sl)
                sl[axis], src[axis] = slice(1, None), slice(None, -1)
                lower[tuple(sl)] = any_live[tuple(src)]
                any_live = any_live | lower
        used = (inside != _shifted(inside, dx, dy, dz)) & any_live
        keys.append(lin[used] * 7 + e)
    vkeys = np.sort(np.concatenate(keys))
    owner, e = vkeys // 7, vkeys % 7
    delta = np.stack([(e + 1) & 1, (e + 1) >> 1 & 1, (e + 1) >> 2], 1)
    other = owner + (delta[:, 2] * ny + delta[:, 1]) * nx + delta[:, 0]
    i, j, k = owner % nx, owner // nx % ny, owner // (nx * ny)
    X0, X1, X2 = centres(origin, h, (nx, ny, nz))
    Xa = np.stack([X0.ravel()[i], X1.ravel()[j], X2.ravel()[k]], 1)
    f = tsdf.ravel()
    fa, fb = f[owner], f[other]
    with np.errstate(all="ignore"):
        tt = fa / (fa - fb)
        vertices = (Xa + tt[:, None] * (delta.astype(F) * h)).astype(F)
        g = gradient(tsdf, valid).reshape(-1, 3)
        ga, gb = g[owner], g[other]
        gv = ga + tt[:, None] * (gb - ga)
        L = np.sqrt((gv[:, 0] * gv[:, 0] + gv[:, 1] * gv[:, 1]) + gv[:, 2] * gv[:, 2])
        ok = (L > 0) & np.isfinite(L)
        normals = np.where(ok[:, None], gv / np.where(ok, L, F(1.0))[:, None], F(0.0)).astype(F)
        vrgb = None
        if rgb is not None:
            c = np.asarray(rgb, np.uint8).reshape(-1, 3).astype(F)
            ca, cb = c[owner], c[other]
            vrgb = np.floor((ca + tt[:, None] * (cb - ca)) + F(0.5)).astype(np.uint8)
    assert tt.dtype == F and gv.dtype == F and L.dtype == F

    # triangles: by (cell, tetrahedron, listed order); a vertex id is the rank of its edge key
    tri_key, tri_edges, cases = [], [], set()
    for t in range(6):
        q = tet_corners(t)
        m = np.zeros((nz, ny, nx), np.int64)
        for l in range(4):
            m |= _shifted(inside, *q[l]).astype(np.int64) << l
        for mask in range(1, 15):
            cells = lin[live & (m == mask)]
            if not len(cells):
                continue
            cases.add((t, mask))
            for r, tri in enumerate(tet_triangles(t, mask)):
                ek = []
                for a, b in tri:
                    lo, hi = min(a, b), max(a, b)
                    d = q[hi] - q[lo]
                    own = cells + (q[lo][2] * ny + q[lo][1]) * nx + q[lo][0]
                    ek.append(own * 7 + ((d[0] | d[1] << 1 | d[2] << 2) - 1))
                tri_key.append((cells * 6 + t) * 2 + r)
                tri_edges.append(np.stack(ek, 1))
    if tri_key:
        tri_key, tri_edges = np.concatenate(tri_key), np.concatenate(tri_edges)
        tri_edges = tri_edges[np.argsort(tri_key, kind="stable")]
        ids = np.searchsorted(vkeys, tri_edges)
        assert np.array_equal(vkeys[ids], tri_edges)            # every triangle corner sits on a used edge ...
        assert len(np.unique(ids)) == len(vkeys)                # ... and every used edge carries a triangle corner
        triangles = ids.astype(np.int32)
    else:
        assert len(vkeys) == 0
        triangles = np.zeros((0, 3), np.int32)
    out = (vertices.reshape(-1, 3), normals.reshape(-1, 3), vrgb, triangles)
    return out + (cases,) if return_cases else out


# ---- volumes and mesh measures the CPU and GPU tests share ----------------------------------------------------------------------
def sphere_volume(dims, h=0.1, centre_voxel=None, radius_voxels=None, shell=None):
    """Exact signed distance to a sphere (negative inside) sampled at the voxel centres of a grid with origin 0, f32, weight 2
    everywhere.  shell = s keeps weight 2 only where |distance| <= s h (a band around the surface), 0 elsewhere."""
    nx, ny, nz = dims
    X0, X1, X2 = centres((0, 0, 0), h, dims)
    c = np.array(centre_voxel if centre_voxel is not None else [nx / 2 + 0.13, ny / 2 - 0.21, nz / 2 + 0.37], np.float64) * h
    r = (radius_voxels if radius_voxels is not None else 0.36 * min(dims)) * h
    d = np.sqrt((X0.astype(np.float64) - c[0]) ** 2 + (X1.astype(np.float64) - c[1]) ** 2 + (X2.astype(np.float64) - c[2]) ** 2) - r
    weight = np.full((nz, ny, nx), 2, np.int32)
    if shell is not None:
        weight[np.abs(d) > shell * h] = 0
    return d.astype(F), weight, c, r


def plane_views(reverse=False):
    """Three identity-rotation views of a fronto-parallel plane whose depth puts the surface exactly on a layer of voxel
    centres: (K4, poses, depth, origin, h, dims, z of the layer).  All values are exact in binary."""
    n, rows, cols = 3, 48, 64
    K4 = np.tile(np.array([32.0, 31.5, 32.0, 23.5], F), (n, 1))
    poses = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], F), (n, 1))
    poses[:, 3] = [-0.25, 0.0, 0.25]
    h, dims = F(0.125), (15, 13, 12)
    origin = np.array([-0.9375, -0.8125, 1.4375], F)
    layer = 7
    z = F(origin[2]) + (F(layer) + F(0.5)) * h                   # 2.375
    depth = np.full((n, rows, cols), z, F)
    order = slice(None, None, -1) if reverse else slice(None)
    return K4[order], poses[order], depth[order], origin, h, dims, z


def mesh_topology(triangles):
    """(directed edges used more than once, directed edges without their reverse, undirected edges, edges shared by more than two
    triangles) of an indexed mesh."""
    t = np.asarray(triangles, np.int64)
    d = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    n = int(t.max()) + 1 if len(t) else 1
    key = d[:, 0] * n + d[:, 1]
    uniq, count = np.unique(key, return_counts=True)
    rev = d[:, 1] * n + d[:, 0]
    unpaired = int(np.count_nonzero(~np.isin(rev, uniq)))
    und = np.minimum(d[:, 0], d[:, 1]) * n + np.maximum(d[:, 0], d[:, 1])
    u2, c2 = np.unique(und, return_counts=True)
    return int(np.count_nonzero(count > 1)), unpaired, len(u2), int(np.count_nonzero(c2 > 2))


# ---- the synthetic-scene chain (tests/mvs_scene.py) ------------------------------------------------------------------------------
CHAIN_GRID = ((-1.5, -1.2, 3.4), 0.04, (76, 61, 80))            # origin, h, dims: the sphere and the plane behind it


def chain_plan(scene, mvs_ref):
    """The plan tests/test_mvs_merge_gpu.py sweeps with: a 400-point sparse cloud from view 2's exact depth that every view
    observes, 48 planes.  Returns (neighbours, depth_range, reference options)."""
    n = len(scene["images"])
    rng = np.random.default_rng(11)
    ys, xs = rng.integers(20, scene["depth"].shape[1] - 20, 400), rng.integers(20, scene["depth"].shape[2] - 20, 400)
    P = scene["poses"][2].reshape(3, 4).astype(np.float64)
    fx, cx, fy, cy = (float(v) for v in scene["K4"][2])
    d = scene["depth"][2][ys, xs]
    Xc = np.stack([(xs - cx) / fx * d, (ys - cy) / fy * d, d], 1)
    sparse = ((Xc - P[:, 3]) @ P[:, :3]).astype(F)
    m = len(sparse)
    off = (np.arange(n + 1) * m).astype(np.int32)
    pts = np.tile(np.arange(m, dtype=np.int32), n)
    ro = mvs_ref.options(num_planes=48)
    nb, dr = mvs_ref.plan(np.ones(n, bool), scene["poses"], sparse, off, pts, ro)
    return nb, dr, ro


def masked_depth(depth, pixel_index):
    """Depth maps with every pixel outside pixel_index (the fusion's kept pixels) set to 0."""
    out = np.zeros(depth.size, F)
    idx = np.asarray(pixel_index, np.int64)
    out[idx] = depth.reshape(-1)[idx]
    return out.reshape(depth.shape)


def chain_quality(scene, mvs_scene, vertices, view=2, margin=4):
    """Over the vertices whose projection into `view` lies at least `margin` px from an occlusion edge: (their number, the
    median of |ray depth - own depth| / ray depth, the share within 1 %)."""
    P = scene["poses"][view].reshape(3, 4).astype(np.float64)
    fx, cx, fy, cy = (float(v) for v in scene["K4"][view])
    X = np.asarray(vertices, np.float64)
    p = X @ P[:, :3].T + P[:, 3]
    u, w = np.rint(fx * p[:, 0] / p[:, 2] + cx).astype(int), np.rint(fy * p[:, 1] / p[:, 2] + cy).astype(int)
    rows, cols = scene["depth"].shape[1:]
    ins = (p[:, 2] > 0) & (u >= 0) & (u < cols) & (w >= 0) & (w < rows)
    far = mvs_scene.edge_distance_mask(scene["obj"][view], scene["depth"][view], margin)
    sel = ins & far[np.clip(w, 0, rows - 1), np.clip(u, 0, cols - 1)]
    ray, own = mvs_scene.ray_depth(scene, view, X[sel])
    rel = np.abs(ray - own) / ray
    return int(sel.sum()), float(np.median(rel)), float(np.mean(rel < 0.01))
