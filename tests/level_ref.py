"""numpy restatement of include/esfm.h, "Mesh texturing", seam levelling: the vertex samples, the node table, the seam and
smoothness neighbours, the normal equations, tree_sum, the Jacobi-preconditioned conjugate gradients and the bake with offsets.
Samples are f32 in the bake's operation order (tests/texture_ref.py supplies projection and layout); everything from the node
table on is f64, every operation written in the header's order (numpy rounds each one, nothing is fused), so the GPU's outputs
are compared with these as bit patterns."""
import numpy as np

import texture_ref as X

F = np.float32
D = np.float64
Rejected = X.Rejected


def options(lam=0.1, mu=0.001, tolerance=1e-4, max_iterations=200):
    return dict(lam=D(lam), mu=D(mu), tolerance=D(tolerance), max_iterations=int(max_iterations))


def _options(opt):
    o = opt or options()
    X._require(np.isfinite(o["lam"]) and o["lam"] > 0, "lambda must be finite and > 0")
    X._require(np.isfinite(o["mu"]) and o["mu"] > 0, "mu must be finite and > 0")
    X._require(0 <= o["tolerance"] < 1, "tolerance must be in [0, 1)")
    X._require(0 <= o["max_iterations"] <= 10000, "max_iterations must be 0..10000")
    return o


def tree_sum(x):
    """The header's tree_sum over the last axis of x [..., n] (f64)."""
    x = np.array(x, D)
    if x.shape[-1] == 0:
        return np.zeros(x.shape[:-1], D)
    while True:
        n = x.shape[-1]
        blocks = (n + 255) // 256
        pad = np.zeros(x.shape[:-1] + (blocks * 256,), D)
        pad[..., :n] = x
        pad = pad.reshape(x.shape[:-1] + (blocks, 256))
        h = 128
        while h >= 1:
            pad[..., :h] = pad[..., :h] + pad[..., h:2 * h]
            h //= 2
        x = pad[..., 0]
        if blocks == 1:
            return x[..., 0]


def _images(images):
    imgs = np.ascontiguousarray(images, np.uint8)
    if imgs.ndim == 3:
        imgs = imgs[..., None]
    X._require(imgs.ndim == 4 and imgs.shape[3] in (1, 3), "channels must be 1 or 3")
    return imgs


def vertex_samples(v, view, imgs, K, P):
    """(f [len(v), 3] f32 RGB: the bake's bilinear value at every vertex' projection into `view`, p2 > 0 [len(v)])."""
    _, rows, cols, ch = imgs.shape
    u, w, _, p2, _ = X.project(v, K, P)
    good = p2 > 0
    with np.errstate(all="ignore"):
        uc = np.fmin(np.fmax(u, F(0)), F(cols - 1)); wc = np.fmin(np.fmax(w, F(0)), F(rows - 1))
        x0 = np.fmin(np.floor(uc), F(cols - 2)); y0 = np.fmin(np.floor(wc), F(rows - 2))
        ax, ay = uc - x0, wc - y0
    xi, yi = np.where(good, x0, 0).astype(np.int64), np.where(good, y0, 0).astype(np.int64)
    f = np.zeros((len(v), 3), F)
    for k in range(3):
        I = imgs[view, :, :, (2 - k) if ch == 3 else 0].astype(F)
        with np.errstate(all="ignore"):
            f[:, k] = (F(1.0) - ay) * ((F(1.0) - ax) * I[yi, xi] + ax * I[yi, xi + 1]) + ay * ((F(1.0) - ax) * I[yi + 1, xi] + ax * I[yi + 1, xi + 1])
    return f, good


def _padded(rows, cols, n):
    """Row-wise neighbour lists in ascending order as a padded table: (table [n, k], count [n])."""
    count = np.bincount(rows, minlength=n).astype(np.int64)
    k = int(count.max()) if len(rows) else 0
    table = np.zeros((n, max(k, 1)), np.int64)
    start = np.concatenate([[0], np.cumsum(count)])[:-1]
    table[rows, np.arange(len(rows)) - start[rows]] = cols
    return table, count


def node_table(vertices, triangles, label, images, K4, poses):
    """Steps 1 and 2: a dict with part [T] bool, corner_node [T, 3] (-1 outside), key [N], f [N, 3] f32, the seam and smoothness
    neighbour tables and seam_vertices."""
    imgs = _images(images)
    n = imgs.shape[0]
    v, t = X._mesh(vertices, triangles)
    K, P = X._cameras(n, imgs.shape[1], imgs.shape[2], K4, poses)
    lab = np.ascontiguousarray(label, np.int32).reshape(-1)
    T = len(t)
    X._require(len(lab) == T and (T == 0 or (lab.min() >= -1 and lab.max() < n)), "a label is outside -1..n_views-1")
    part = np.zeros(T, bool)
    fv = np.zeros((n, len(v), 3), F)
    for view in range(n):
        m = lab == view
        if not m.any():
            continue
        fv[view], good = vertex_samples(v, view, imgs, K[view], P[view])
        part[m] = good[t[m]].all(axis=1)
    keys = (t.astype(np.int64) * 64 + lab[:, None].astype(np.int64))[part]                  # [Tp, 3]
    key, inverse = np.unique(keys.reshape(-1), return_inverse=True)
    N = len(key)
    corner_node = np.full((T, 3), -1, np.int64)
    corner_node[part] = inverse.reshape(-1, 3)
    f = fv[key % 64, key // 64] if N else np.zeros((0, 3), F)
    vertex = key // 64
    first = np.searchsorted(vertex, vertex, side="left")
    last = np.searchsorted(vertex, vertex, side="right")
    a = np.repeat(np.arange(N), last - first)
    b = np.arange(len(a)) - np.repeat(np.cumsum(last - first) - (last - first), last - first) + np.repeat(first, last - first)
    keep = a != b
    seam, seam_n = _padded(a[keep], b[keep], N)
    tri = corner_node[part]
    p = np.concatenate([tri[:, [0, 1, 2]].reshape(-1), tri[:, [1, 2, 0]].reshape(-1)])
    q = np.concatenate([tri[:, [1, 2, 0]].reshape(-1), tri[:, [0, 1, 2]].reshape(-1)])
    pairs = np.unique((p << 32 | q)[p != q])
    smooth, smooth_n = _padded(pairs >> 32, pairs & 0xFFFFFFFF, N)
    seam_vertices = int(np.count_nonzero((first == np.arange(N)) & (last - first >= 2)))
    return dict(part=part, corner_node=corner_node, key=key, f=f, seam=seam, seam_n=seam_n, smooth=smooth, smooth_n=smooth_n,
                seam_vertices=seam_vertices, nodes=N)


def _ordered_difference_sum(x, table, count):
    """Per node a and channel: the sum over its neighbours b, in table order and starting from 0.0, of (x_a - x_b).  x [N, 3]."""
    s = np.zeros_like(x)
    for j in range(table.shape[1] if count.size and count.max() else 0):
        m = count > j
        s[m] = s[m] + (x[m] - x[table[m, j]])
    return s


def solve(nt, opt=None):
    """Steps 3 to 5 on a node table: (g [N, 3] f64, iterations, converged)."""
    o = _options(opt)
    lam, mu, N = o["lam"], o["mu"], nt["nodes"]
    g = np.zeros((N, 3), D)
    if N == 0:
        return g, 0, 1
    f = nt["f"].astype(D)
    rhs = np.zeros((N, 3), D)
    for j in range(nt["seam"].shape[1] if nt["seam_n"].max() else 0):
        m = nt["seam_n"] > j
        rhs[m] = rhs[m] + (f[nt["seam"][m, j]] - f[m])
    d = ((nt["seam_n"].astype(D) + lam * nt["smooth_n"].astype(D)) + mu)[:, None]
    dot = lambda a, b: tree_sum((a * b).T)
    safe = lambda num, den: np.where(den == 0, D(0), num / np.where(den == 0, D(1), den))

    def apply(p):
        return (_ordered_difference_sum(p, nt["seam"], nt["seam_n"]) + lam * _ordered_difference_sum(p, nt["smooth"], nt["smooth_n"])) + mu * p
    r = rhs.copy()
    z = r / d
    p = z.copy()
    rz = dot(r, z)
    bb = dot(rhs, rhs)
    if np.all(bb == 0):
        return g, 0, 1
    limit = (o["tolerance"] * o["tolerance"]) * bb
    for k in range(1, o["max_iterations"] + 1):
        q = apply(p)
        alpha = safe(rz, dot(p, q))
        g = g + alpha * p
        r = r - alpha * q
        rr = dot(r, r)
        if np.all(rr <= limit):
            return g, k, 1
        z = r / d
        rz2 = dot(r, z)
        beta = safe(rz2, rz)
        p = z + beta * p
        rz = rz2
    return g, o["max_iterations"], 0


def texture_level(vertices, triangles, label, images, K4, poses, opt=None):
    """esfm_mesh_texture_level: (offsets [T, 3, 3] f32, samples [T, 3, 3] f32, stats dict nodes / seam_vertices / iterations /
    converged)."""
    o = _options(opt)
    nt = node_table(vertices, triangles, label, images, K4, poses)
    g, iterations, converged = solve(nt, o)
    T = len(nt["part"])
    offsets, samples = np.zeros((T, 3, 3), F), np.zeros((T, 3, 3), F)
    if nt["nodes"]:
        with np.errstate(over="ignore"):
            offsets[nt["part"]] = g.astype(F)[nt["corner_node"][nt["part"]]]
        samples[nt["part"]] = nt["f"][nt["corner_node"][nt["part"]]]
    return offsets, samples, dict(nodes=nt["nodes"], seam_vertices=nt["seam_vertices"], iterations=iterations, converged=converged)


def texture_bake(vertices, vertex_rgb, triangles, label, images, K4, poses, texels, atlas_width, offsets=None, max_atlas_rows=None):
    """esfm_mesh_texture_bake_ex: tests/texture_ref.py's bake, and with offsets [T, 3, 3] the levelled one: (atlas, uv)."""
    if offsets is None:
        return X.texture_bake(vertices, vertex_rgb, triangles, label, images, K4, poses, texels, atlas_width, max_atlas_rows)
    imgs = _images(images)
    n, rows, cols, ch = imgs.shape
    v, t = X._mesh(vertices, triangles)
    K, P = X._cameras(n, rows, cols, K4, poses)
    lab = np.ascontiguousarray(label, np.int32).reshape(-1)
    T, S = len(t), int(texels)
    off = np.ascontiguousarray(offsets, F).reshape(-1, 3, 3)
    X._require(len(off) == T and np.all(np.isfinite(off)), "an offset is not finite")
    atlas, uv = X.texture_bake(v, vertex_rgb, t, lab, imgs, K, P, S, atlas_width, max_atlas_rows)
    if T == 0:
        return atlas, uv
    H, W = atlas.shape[:2]
    Y, Xc = np.mgrid[0:H, 0:W]
    i, j = Xc % S, Y % S
    tri = 2 * (Y // S * atlas_width + Xc // S) + X.texel_owner(S)[j, i]
    b0, b1, b2 = (b[j, i] for b in X.texel_barycentrics(S))
    real = tri < T
    tc = np.where(real, tri, 0)
    c = t[tc]
    Xw = (b0[..., None] * v[c[..., 0]] + b1[..., None] * v[c[..., 1]]) + b2[..., None] * v[c[..., 2]]
    lt = lab[tc]
    for view in range(n):
        m = real & (lt == view)
        if not m.any():
            continue
        val, good = vertex_samples(Xw[m], view, imgs, K[view], P[view])
        o = off[tc[m]]                                                  # [m, corner, channel]
        w0, w1, w2 = b0[m][:, None], b1[m][:, None], b2[m][:, None]
        with np.errstate(all="ignore"):
            val = val + ((w0 * o[:, 0] + w1 * o[:, 1]) + w2 * o[:, 2])
            out = np.floor(np.fmin(np.fmax(val, F(0)), F(255)) + F(0.5))
        sel = atlas[m]
        sel[good] = np.where(good[:, None], out, 0).astype(np.uint8)[good]
        atlas[m] = sel
    return atlas, uv
