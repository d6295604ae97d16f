"""numpy restatement of include/esfm.h, "Mesh texturing": the per-view buffers of inverse depth, the per-triangle view choice, the
atlas layout and the bake.  Every f32 operation is written in the header's order (numpy rounds each one; np.fmin / np.fmax are
fminf / fmaxf), so the GPU's outputs are compared with these as bit patterns.  The rasteriser is vectorised over the triangles
and loops over the offsets inside their bounding boxes."""
import numpy as np

F = np.float32
MAX_VIEWS = 64
MAX_ATLAS = 16384
MAX_TRIANGLES = 1 << 25
FRONT_LIMIT = F(1 << 20)


class Rejected(ValueError):
    """What the library answers with ESFM_ERR_INVALID_ARG."""


def options(min_cos=0.2, occlusion_tol=0.02):
    return dict(min_cos=F(min_cos), occlusion_tol=F(occlusion_tol))


def _require(cond, what):
    if not cond:
        raise Rejected(what)


def _mesh(vertices, triangles):
    v = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    t = np.ascontiguousarray(triangles, np.int32).reshape(-1, 3)
    _require(len(v) <= 1 << 30 and len(t) <= MAX_TRIANGLES, "count out of range")
    _require(np.all(np.isfinite(v)), "a vertex is not finite")
    _require(len(t) == 0 or (t.min() >= 0 and t.max() < len(v)), "a triangle index is outside 0..V-1")
    return v, t


def _cameras(n_views, rows, cols, K4, poses):
    _require(1 <= n_views <= MAX_VIEWS, "n_views must be 1..64")
    _require(2 <= rows <= MAX_ATLAS and 2 <= cols <= MAX_ATLAS, "rows and cols must be 2..16384")
    K = np.ascontiguousarray(K4, F).reshape(n_views, 4)
    P = np.ascontiguousarray(poses, F).reshape(n_views, 12)
    _require(np.all(np.isfinite(K)) and np.all(np.isfinite(P)), "K4 and poses must be finite")
    _require(np.all(K[:, 0] != 0) and np.all(K[:, 2] != 0), "a focal length is 0")
    return K, P


def _options(opt):
    o = opt or options()
    for name in ("min_cos", "occlusion_tol"):
        _require(np.isfinite(o[name]) and 0 <= o[name] < 1, name + " must be in [0, 1)")
    return o


def project(X, K, P):
    """(u, w, z, p2, front) of the world points X [m, 3] in the view with K (4) and P (12)."""
    with np.errstate(all="ignore"):
        p = [((P[4 * i] * X[:, 0] + P[4 * i + 1] * X[:, 1]) + P[4 * i + 2] * X[:, 2]) + P[4 * i + 3] for i in range(3)]
        u = K[0] * (p[0] / p[2]) + K[1]
        w = K[2] * (p[1] / p[2]) + K[3]
        z = F(1.0) / p[2]
        front = (p[2] > 0) & (np.abs(u) <= FRONT_LIMIT) & (np.abs(w) <= FRONT_LIMIT)
    return u, w, z, p[2], front


def _screen(v, t, K, P):
    """Per triangle: x, y, z [T, 3], whether the screen triangle exists, area2."""
    u, w, z, _, front = project(v, K, P)
    x, y, zz, fr = u[t], w[t], z[t], front[t].all(axis=1) if len(t) else np.zeros(0, bool)
    x = np.where(fr[:, None], x, F(0)); y = np.where(fr[:, None], y, F(0)); zz = np.where(fr[:, None], zz, F(1))
    area2 = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (y[:, 1] - y[:, 0]) * (x[:, 2] - x[:, 0])
    return x, y, zz, fr, area2


def rasterise(v, t, K, P, rows, cols):
    """The view's buffer [rows, cols] uint32."""
    buf = np.zeros(rows * cols, np.uint32)
    x, y, z, fr, area2 = _screen(v, t, K, P)
    live = np.nonzero(fr & (area2 != 0))[0]
    if len(live) == 0:
        return buf.reshape(rows, cols)
    x, y, z, area2 = x[live], y[live], z[live], area2[live]
    s = np.where(area2 > 0, F(1), F(-1))
    bx0 = np.fmax(np.ceil(x.min(axis=1) - F(0.5)), F(0)).astype(np.int64)
    bx1 = np.fmin(np.floor(x.max(axis=1) + F(0.5)), F(cols - 1)).astype(np.int64)
    by0 = np.fmax(np.ceil(y.min(axis=1) - F(0.5)), F(0)).astype(np.int64)
    by1 = np.fmin(np.floor(y.max(axis=1) + F(0.5)), F(rows - 1)).astype(np.int64)
    bw, bh = bx1 - bx0 + 1, by1 - by0 + 1
    zmin, zmax = z.min(axis=1), z.max(axis=1)
    ex = np.stack([x[:, (k + 1) % 3] - x[:, k] for k in range(3)], 1)
    ey = np.stack([y[:, (k + 1) % 3] - y[:, k] for k in range(3)], 1)
    rim = F(-0.5) * (np.abs(ex) + np.abs(ey))
    some = np.nonzero((bw > 0) & (bh > 0))[0]
    for dy in range(int(bh[some].max()) if len(some) else 0):
        rows_in = some[bh[some] > dy]
        for dx in range(int(bw[rows_in].max())):
            m = rows_in[bw[rows_in] > dx]
            px, py = bx0[m] + dx, by0[m] + dy
            fx, fy = px.astype(F), py.astype(F)
            with np.errstate(all="ignore"):
                e = [ex[m, k] * (fy - y[m, k]) - ey[m, k] * (fx - x[m, k]) for k in range(3)]
                inside = (s[m] * e[0] >= rim[m, 0]) & (s[m] * e[1] >= rim[m, 1]) & (s[m] * e[2] >= rim[m, 2])
                b0, b1, b2 = e[1] / area2[m], e[2] / area2[m], e[0] / area2[m]
                zz = (b0 * z[m, 0] + b1 * z[m, 1]) + b2 * z[m, 2]
                zz = np.fmin(np.fmax(zz, zmin[m]), zmax[m])
            np.maximum.at(buf, (py * cols + px)[inside], zz[inside].view(np.uint32))
    return buf.reshape(rows, cols)


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def _norm(a):
    return np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])


def texture_views(vertices, triangles, rows, cols, K4, poses, opt=None):
    """esfm_mesh_texture_views: (label [T] int32, score [T] f32, buffers [n, rows, cols] uint32)."""
    n = len(np.asarray(K4).reshape(-1, 4))
    v, t = _mesh(vertices, triangles)
    K, P = _cameras(n, rows, cols, K4, poses)
    o = _options(opt)
    T = len(t)
    label, best = np.full(T, -1, np.int32), np.zeros(T, F)
    buffers = np.zeros((n, rows, cols), np.uint32)
    keep = F(1.0) - o["occlusion_tol"]
    P0, P1, P2 = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    N = _cross(P1 - P0, P2 - P0)
    G = ((P0 + P1) + P2) / F(3.0)
    lN = _norm(N)
    for view in range(n):
        buffers[view] = rasterise(v, t, K[view], P[view], rows, cols)
        if T == 0:
            continue
        flat = buffers[view].reshape(-1).view(F)
        x, y, z, fr, area2 = _screen(v, t, K[view], P[view])
        score = F(0.5) * np.abs(area2)
        ok = fr & np.all((x >= 1) & (x <= F(cols - 2)) & (y >= 1) & (y <= F(rows - 2)), axis=1) & (score > 0)
        R, tr = P[view].reshape(3, 4)[:, :3], P[view].reshape(3, 4)[:, 3]
        C = np.array([-((R[0, j] * tr[0] + R[1, j] * tr[1]) + R[2, j] * tr[2]) for j in range(3)], F)
        D = C[None, :] - G
        with np.errstate(all="ignore"):
            d = (N[:, 0] * D[:, 0] + N[:, 1] * D[:, 1]) + N[:, 2] * D[:, 2]
            ok &= (d > 0) & (d >= o["min_cos"] * (lN * _norm(D)))
        gu, gw, gz, _, gfront = project(G, K[view], P[view])
        ok &= gfront
        points = [(x[:, k], y[:, k], z[:, k]) for k in range(3)] + [(np.where(gfront, gu, F(0)), np.where(gfront, gw, F(0)), gz)]
        for pu, pw, pz in points:
            px, py = np.floor(pu + F(0.5)), np.floor(pw + F(0.5))
            inside = (px >= 0) & (px < cols) & (py >= 0) & (py < rows)
            pix = np.where(inside, py.astype(np.int64) * cols + px.astype(np.int64), 0)
            with np.errstate(all="ignore"):
                ok &= inside & (pz >= flat[pix] * keep)
        better = ok & (score > best)
        best = np.where(better, score, best)
        label = np.where(better, np.int32(view), label)
    return label, best, buffers


def atlas_shape(T, texels, atlas_width):
    """(H, W) of the atlas; Rejected if the layout is not allowed."""
    _require(4 <= texels <= 64, "texels must be 4..64")
    _require(atlas_width >= 1, "atlas_width must be >= 1")
    _require(atlas_width * texels <= MAX_ATLAS, "the atlas is wider than 16384 texels")
    squares = (T + 1) // 2
    H = (squares + atlas_width - 1) // atlas_width * texels
    _require(H <= MAX_ATLAS, "the atlas is higher than 16384 texels")
    return H, atlas_width * texels


def chart_corners(S, odd):
    """The three chart corners in the square's texel units."""
    if odd:
        return np.array([[S - 0.5, S - 0.5], [2.5, S - 0.5], [S - 0.5, 2.5]], F)
    return np.array([[0.5, 0.5], [S - 1.5, 0.5], [0.5, S - 1.5]], F)


def texture_uv(T, texels, atlas_width):
    """uv [T, 3, 2] f32."""
    H, W = atlas_shape(T, texels, atlas_width)
    uv = np.zeros((T, 3, 2), F)
    tt = np.arange(T)
    q = tt // 2
    X0, Y0 = (q % atlas_width * texels).astype(F), (q // atlas_width * texels).astype(F)
    for odd in (0, 1):
        c = chart_corners(texels, odd)
        m = tt % 2 == odd
        for k in range(3):
            uv[m, k, 0] = (X0[m] + c[k, 0]) / F(W)
            uv[m, k, 1] = (Y0[m] + c[k, 1]) / F(H)
    return uv


def texel_owner(S):
    """[S, S] (row j, column i): 0 where the texel belongs to the square's even triangle, 1 where to the odd one."""
    j, i = np.mgrid[0:S, 0:S]
    return (i + j > S - 1).astype(np.int32)


def texel_barycentrics(S):
    """b0, b1, b2 [S, S] (row j, column i) of every texel of a square with respect to its owner's chart."""
    j, i = np.mgrid[0:S, 0:S]
    odd = texel_owner(S) == 1
    with np.errstate(all="ignore"):
        b1 = np.where(odd, (S - 1 - i).astype(F) / F(S - 3), i.astype(F) / F(S - 2))
        b2 = np.where(odd, (S - 1 - j).astype(F) / F(S - 3), j.astype(F) / F(S - 2))
    return (F(1.0) - b1) - b2, b1, b2


def texture_bake(vertices, vertex_rgb, triangles, label, images, K4, poses, texels, atlas_width, max_atlas_rows=None):
    """esfm_mesh_texture_bake: (atlas [H, W, 3] u8, uv [T, 3, 2] f32)."""
    imgs = np.ascontiguousarray(images, np.uint8)
    if imgs.ndim == 3:
        imgs = imgs[..., None]
    n, rows, cols, ch = imgs.shape
    _require(ch in (1, 3), "channels must be 1 or 3")
    v, t = _mesh(vertices, triangles)
    K, P = _cameras(n, rows, cols, K4, poses)
    lab = np.ascontiguousarray(label, np.int32).reshape(-1)
    T, S = len(t), int(texels)
    _require(len(lab) == T and (T == 0 or (lab.min() >= -1 and lab.max() < n)), "a label is outside -1..n_views-1")
    H, W = atlas_shape(T, S, atlas_width)
    if max_atlas_rows is not None:
        _require(H <= max_atlas_rows, "the atlas needs %d rows" % H)
    uv = texture_uv(T, S, atlas_width)
    if T == 0:
        return np.zeros((0, W, 3), np.uint8), uv
    Y, X = np.mgrid[0:H, 0:W]
    i, j = X % S, Y % S
    tri = 2 * (Y // S * atlas_width + X // S) + texel_owner(S)[j, i]
    b0, b1, b2 = (b[j, i] for b in texel_barycentrics(S))
    real = tri < T
    tc = np.where(real, tri, 0)
    c = t[tc]                                                          # [H, W, 3] vertex indices
    if vertex_rgb is not None:
        col = np.ascontiguousarray(vertex_rgb, np.uint8).reshape(-1, 3).astype(F)
        mix = (b0[..., None] * col[c[..., 0]] + b1[..., None] * col[c[..., 1]]) + b2[..., None] * col[c[..., 2]]
        fallback = np.floor(np.fmin(np.fmax(mix, F(0)), F(255)) + F(0.5)).astype(np.uint8)
    else:
        fallback = np.full((H, W, 3), 128, np.uint8)
    Xw = (b0[..., None] * v[c[..., 0]] + b1[..., None] * v[c[..., 1]]) + b2[..., None] * v[c[..., 2]]
    atlas = fallback.copy()
    lt = lab[tc]
    for view in range(n):
        m = real & (lt == view)
        if not m.any():
            continue
        u, w, _, p2, _ = project(Xw[m], K[view], P[view])
        good = p2 > 0
        with np.errstate(all="ignore"):
            uc = np.fmin(np.fmax(u, F(0)), F(cols - 1)); wc = np.fmin(np.fmax(w, F(0)), F(rows - 1))
            x0 = np.fmin(np.floor(uc), F(cols - 2)); y0 = np.fmin(np.floor(wc), F(rows - 2))
            ax, ay = uc - x0, wc - y0
        xi, yi = np.where(good, x0, 0).astype(np.int64), np.where(good, y0, 0).astype(np.int64)
        out = np.zeros((len(u), 3), np.uint8)
        for k in range(3):
            I = imgs[view, :, :, (2 - k) if ch == 3 else 0].astype(F)
            with np.errstate(all="ignore"):
                val = (F(1.0) - ay) * ((F(1.0) - ax) * I[yi, xi] + ax * I[yi, xi + 1]) + ay * ((F(1.0) - ax) * I[yi + 1, xi] + ax * I[yi + 1, xi + 1])
                out[:, k] = np.where(good, np.floor(val + F(0.5)), 0).astype(np.uint8)
        sel = atlas[m]
        sel[good] = out[good]
        atlas[m] = sel
    atlas[~real] = 0
    return atlas, uv


def auto_texels(label, score):
    """The S mesh_texture derives: the median over labelled triangles of sqrt(2 score), rounded up, clamped to 4..64."""
    s = np.asarray(score, np.float64)[np.asarray(label) >= 0]
    if len(s) == 0:
        return 4
    return int(min(64, max(4, np.ceil(np.median(np.sqrt(2.0 * s))))))
