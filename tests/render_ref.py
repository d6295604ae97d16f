"""numpy restatement of include/esfm.h, "Mesh rendering": screen vertices in 1/256-pixel fixed point, exact int64 coverage with the
ownership rule, the 64-bit key buffer and the per-pixel shading.  Every f32 operation is written in the header's order (numpy
rounds each one; an int64 becomes f32 by one rounding), so the GPU's outputs are compared with these as bit patterns.  The
rasteriser is vectorised over the triangles and loops over the offsets inside their bounding boxes."""
import numpy as np

import texture_ref as X

F = np.float32
I = np.int64
Rejected = X.Rejected


def screen(v, K, P):
    """Per vertex: sx, sy int64, z f32, front."""
    u, w, z, _, front = X.project(v, K, P)
    with np.errstate(all="ignore"):
        sx = np.rint(np.where(front, u, F(0)) * F(256.0)).astype(I)
        sy = np.rint(np.where(front, w, F(0)) * F(256.0)).astype(I)
    return sx, sy, np.where(front, z, F(0)), front


class Tris:
    """The screen triangles of one view that take part: all vertices in front, area2 != 0."""

    def __init__(self, v, t, K, P, rows, cols):
        sx, sy, z, front = screen(v, K, P)
        if len(t):
            x, y, zz, fr = sx[t], sy[t], z[t], front[t].all(axis=1)
        else:
            x, y, zz, fr = np.zeros((0, 3), I), np.zeros((0, 3), I), np.zeros((0, 3), F), np.zeros(0, bool)
        area2 = (x[:, 1] - x[:, 0]) * (y[:, 2] - y[:, 0]) - (y[:, 1] - y[:, 0]) * (x[:, 2] - x[:, 0])
        self.x, self.y, self.z, self.area2 = x, y, zz, area2
        self.live = np.nonzero(fr & (area2 != 0))[0]
        self.bx0 = np.maximum(-((-x.min(axis=1)) // 256), 0) if len(t) else np.zeros(0, I)      # ceil by floor division
        self.bx1 = np.minimum(x.max(axis=1) // 256, cols - 1) if len(t) else np.zeros(0, I)
        self.by0 = np.maximum(-((-y.min(axis=1)) // 256), 0) if len(t) else np.zeros(0, I)
        self.by1 = np.minimum(y.max(axis=1) // 256, rows - 1) if len(t) else np.zeros(0, I)

    def cover(self, m, px, py):
        """Triangles m at pixels (px, py), elementwise: (covered, q [3], iz)."""
        s = np.sign(self.area2[m])
        X_, Y_ = 256 * px.astype(I), 256 * py.astype(I)
        e, covered = [], np.ones(len(m), bool)
        for k in range(3):
            k1 = (k + 1) % 3
            dx, dy = self.x[m, k1] - self.x[m, k], self.y[m, k1] - self.y[m, k]
            ek = dx * (Y_ - self.y[m, k]) - dy * (X_ - self.x[m, k])
            owns = (s * dy > 0) | ((s * dy == 0) & (s * dx < 0))
            covered &= (s * ek > 0) | ((s * ek == 0) & owns)
            e.append(ek)
        with np.errstate(all="ignore"):
            fa = self.area2[m].astype(F)
            b = [e[1].astype(F) / fa, e[2].astype(F) / fa, e[0].astype(F) / fa]
            q = [b[k] * self.z[m, k] for k in range(3)]
            iz = (q[0] + q[1]) + q[2]
        return covered, q, iz

    def boxes(self):
        """Yields (m, px, py): for every offset inside the boxes, the live triangles whose box holds it and their pixel there."""
        live = self.live
        bw, bh = self.bx1[live] - self.bx0[live] + 1, self.by1[live] - self.by0[live] + 1
        some = live[(bw > 0) & (bh > 0)]
        bw, bh = self.bx1[some] - self.bx0[some] + 1, self.by1[some] - self.by0[some] + 1
        for dy in range(int(bh.max()) if len(some) else 0):
            in_y = bh > dy
            for dx in range(int(bw[in_y].max())):
                m = some[in_y & (bw > dx)]
                yield m, self.bx0[m] + dx, self.by0[m] + dy


def coverage_count(vertices, triangles, K, P, rows, cols):
    """[rows, cols] int32: how many triangles cover each pixel (depth plays no part)."""
    v, t = X._mesh(vertices, triangles)
    tr = Tris(v, t, np.asarray(K, F).reshape(4), np.asarray(P, F).reshape(12), rows, cols)
    cnt = np.zeros(rows * cols, np.int32)
    for m, px, py in tr.boxes():
        covered = tr.cover(m, px, py)[0]
        np.add.at(cnt, (py * cols + px)[covered], 1)
    return cnt.reshape(rows, cols)


def key_buffer(tr, rows, cols):
    keys = np.zeros(rows * cols, np.uint64)
    for m, px, py in tr.boxes():
        covered, _, iz = tr.cover(m, px, py)
        bits = iz.view(np.uint32)
        ok = covered & (bits != 0)
        key = (bits.astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - m.astype(np.uint64))
        np.maximum.at(keys, (py * cols + px)[ok], key[ok])
    return keys


def _round_u8(c):
    return np.floor(c + F(0.5)).astype(np.uint8)


def mesh_render(vertices, triangles, K4, poses, rows, cols, vertex_rgb=None, uv=None, atlas=None, background=(0, 0, 0)):
    """esfm_mesh_render: (rgb [n, rows, cols, 3] u8, depth [n, rows, cols] f32, triangle_id [n, rows, cols] int32)."""
    n = len(np.asarray(K4).reshape(-1, 4))
    v, t = X._mesh(vertices, triangles)
    K, P = X._cameras(n, rows, cols, K4, poses)
    X._require((uv is None) == (atlas is None), "uv and atlas must both be given or both be None")
    if atlas is not None:
        at = np.ascontiguousarray(atlas, np.uint8)
        X._require(at.ndim == 3 and at.shape[2] == 3 and 2 <= at.shape[0] <= X.MAX_ATLAS and 2 <= at.shape[1] <= X.MAX_ATLAS, "the atlas must be 2..16384 texels per side")
        g = np.ascontiguousarray(uv, F).reshape(-1, 3, 2)
        X._require(len(g) == len(t) and np.all(np.isfinite(g)), "a texture coordinate is not finite")
        H, W = at.shape[:2]
    col = np.ascontiguousarray(vertex_rgb, np.uint8).reshape(-1, 3).astype(F) if vertex_rgb is not None else None
    rgb = np.zeros((n, rows * cols, 3), np.uint8)
    rgb[:] = np.asarray(background, np.uint8)
    depth = np.zeros((n, rows * cols), F)
    tid = np.full((n, rows * cols), -1, np.int32)
    for view in range(n):
        tr = Tris(v, t, K[view], P[view], rows, cols)
        keys = key_buffer(tr, rows, cols)
        pix = np.nonzero(keys)[0]
        if len(pix) == 0:
            continue
        m = (np.uint64(0xFFFFFFFF) - (keys[pix] & np.uint64(0xFFFFFFFF))).astype(I)
        _, q, iz = tr.cover(m, pix % cols, pix // cols)
        tid[view, pix] = m.astype(np.int32)
        with np.errstate(all="ignore"):
            depth[view, pix] = F(1.0) / iz
            attr = lambda a0, a1, a2: ((q[0] * a0 + q[1] * a1) + q[2] * a2) / iz
            if atlas is not None:
                uu, vv = attr(g[m, 0, 0], g[m, 1, 0], g[m, 2, 0]), attr(g[m, 0, 1], g[m, 1, 1], g[m, 2, 1])
                a, c = uu * F(W) - F(0.5), vv * F(H) - F(0.5)
                uc = np.fmin(np.fmax(a, F(0)), F(W - 1)); wc = np.fmin(np.fmax(c, F(0)), F(H - 1))
                x0 = np.fmin(np.floor(uc), F(W - 2)); y0 = np.fmin(np.floor(wc), F(H - 2))
                ax, ay = uc - x0, wc - y0
                xi, yi = x0.astype(I), y0.astype(I)
                for ch in range(3):
                    A = at[:, :, ch].astype(F)
                    val = (F(1.0) - ay) * ((F(1.0) - ax) * A[yi, xi] + ax * A[yi, xi + 1]) + ay * ((F(1.0) - ax) * A[yi + 1, xi] + ax * A[yi + 1, xi + 1])
                    rgb[view, pix, ch] = _round_u8(val)
            elif col is not None:
                c0, c1, c2 = col[t[m, 0]], col[t[m, 1]], col[t[m, 2]]
                for ch in range(3):
                    rgb[view, pix, ch] = _round_u8(np.fmin(np.fmax(attr(c0[:, ch], c1[:, ch], c2[:, ch]), F(0)), F(255)))
            else:
                rgb[view, pix] = 128
    return rgb.reshape(n, rows, cols, 3), depth.reshape(n, rows, cols), tid.reshape(n, rows, cols)
