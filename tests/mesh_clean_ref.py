"""numpy restatement of include/esfm.h, "Mesh clean-up": connected components with the component's smallest vertex as label,
the component filter and ordered compaction, the sorted-key adjacency with pinned vertices, Taubin smoothing with sequential
f32 neighbour sums, and vertex normals as sequential f32 sums of face vectors in incidence order.  Imports nothing from the
library; the GPU tests compare bit patterns against it."""
import numpy as np

F = np.float32


class Rejected(ValueError):
    pass


def options(min_component_triangles=64, min_component_permille=10, smooth_iterations=5, smooth_lambda=0.5, smooth_mu=-0.53,
            pin_boundary=1):
    return dict(min_component_triangles=min_component_triangles, min_component_permille=min_component_permille,
                smooth_iterations=smooth_iterations, smooth_lambda=smooth_lambda, smooth_mu=smooth_mu, pin_boundary=pin_boundary)


def check_options(o):
    lam, mu = F(o["smooth_lambda"]), F(o["smooth_mu"])
    ok = (o["min_component_triangles"] >= 1 and 0 <= o["min_component_permille"] <= 1000 and 0 <= o["smooth_iterations"] <= 1000
          and np.isfinite(lam) and 0 < lam <= 1 and np.isfinite(mu) and -1.5 <= mu <= 0 and o["pin_boundary"] in (0, 1))
    if not ok:
        raise Rejected(str(o))


def _triangles(triangles, n_vertices):
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    if n_vertices < 0 or (len(t) and (t.min() < 0 or t.max() >= n_vertices)):
        raise Rejected("a triangle index is outside 0..n_vertices-1")
    return t


def components(triangles, n_vertices):
    """(labels [V] int32, tri_count [V] int32 -- a component's count at its label vertex --, number of components).  Roots hook
    onto the smallest root they touch, then every path is compressed; the number of rounds grows with the logarithm of the
    component count, not with the mesh diameter."""
    t = _triangles(triangles, n_vertices)
    p = np.arange(n_vertices, dtype=np.int64)
    a = np.concatenate([t[:, 0], t[:, 0]])
    b = np.concatenate([t[:, 1], t[:, 2]])
    while True:
        pa, pb = p[a], p[b]
        if np.array_equal(pa, pb):
            break
        np.minimum.at(p, np.maximum(pa, pb), np.minimum(pa, pb))
        while True:
            pp = p[p]
            if np.array_equal(pp, p):
                break
            p = pp
    count = np.bincount(p[t[:, 0]], minlength=n_vertices) if len(t) else np.zeros(n_vertices, np.int64)
    return p.astype(np.int32), count.astype(np.int32), int(np.count_nonzero(p == np.arange(n_vertices)))


def kept_components(tri_count, o):
    """Per label vertex: is its component kept."""
    c = np.asarray(tri_count, np.int64)
    largest = int(c.max()) if len(c) else 0
    return (c >= o["min_component_triangles"]) & (1000 * c >= o["min_component_permille"] * largest)


def adjacency(triangles, n_vertices):
    """(row_start [V + 1], columns, pinned [V] bool) of the mesh's distinct directed keys."""
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    pairs = [(0, 1), (1, 0), (1, 2), (2, 1), (2, 0), (0, 2)]
    a = np.concatenate([t[:, i] for i, _ in pairs])
    b = np.concatenate([t[:, j] for _, j in pairs])
    keys = np.sort(((a << 32) | b)[a != b])
    uniq, mult = np.unique(keys, return_counts=True)
    row, col = uniq >> 32, uniq & 0xFFFFFFFF
    pinned = np.zeros(n_vertices, bool)
    pinned[row[mult != 2]] = True
    return np.searchsorted(row, np.arange(n_vertices + 1)), col, pinned


def _sequential_row_sums(start, gather):
    """Per row i the f32 sum of gather(j) over j = start[i] .. start[i + 1] - 1 in that order, starting from the first;
    vectorised over the rank within the row.  Rows without entries give 0."""
    n = len(start) - 1
    k = np.diff(start)
    acc = np.zeros((n, 3), F)
    for r in range(int(k.max()) if n else 0):
        has = np.nonzero(k > r)[0]
        term = gather(start[has] + r)
        acc[has] = term if r == 0 else acc[has] + term
    assert acc.dtype == F
    return acc, k


def smooth(vertices, triangles, o):
    p = np.ascontiguousarray(vertices, F).reshape(-1, 3).copy()
    if o["smooth_iterations"] == 0 or len(p) == 0:
        return p
    start, col, pinned = adjacency(triangles, len(p))
    for s in range(2 * o["smooth_iterations"]):
        w = F(o["smooth_lambda"]) if s % 2 == 0 else F(o["smooth_mu"])
        m, k = _sequential_row_sums(start, lambda j: p[col[j]])
        move = k > 0
        if o["pin_boundary"]:
            move &= ~pinned
        c = m[move] / k[move].astype(F)[:, None]
        q = p.copy()
        q[move] = p[move] + w * (c - p[move])
        assert q.dtype == F
        p = q
    return p


def normals(vertices, triangles):
    p = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    t = np.asarray(triangles, np.int64).reshape(-1, 3)
    e1, e2 = p[t[:, 1]] - p[t[:, 0]], p[t[:, 2]] - p[t[:, 0]]
    f = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    assert f.dtype == F
    keys = np.sort((t.reshape(-1) << 32) | np.arange(3 * len(t), dtype=np.int64))
    start = np.searchsorted(keys >> 32, np.arange(len(p) + 1))
    tri_of = (keys & 0xFFFFFFFF) // 3
    n, _ = _sequential_row_sums(start, lambda j: f[tri_of[j]])
    with np.errstate(all="ignore"):
        L = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        ok = (L > 0) & np.isfinite(L)
        out = np.zeros_like(n)
        out[ok] = n[ok] / L[ok][:, None]
    assert out.dtype == F
    return out


def clean(vertices, rgb, triangles, o=None):
    """esfm_mesh_clean: (vertices, normals, rgb or None, triangles, vertex_map, triangle_map)."""
    o = o or options()
    check_options(o)
    v = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    t = _triangles(triangles, len(v))
    labels, count, _ = components(t, len(v))
    keep = kept_components(count, o)
    vmap = np.nonzero(keep[labels])[0]
    tmap = np.nonzero(keep[labels[t[:, 0]]])[0] if len(t) else np.zeros(0, np.int64)
    remap = np.full(len(v), -1, np.int64)
    remap[vmap] = np.arange(len(vmap))
    tri = remap[t[tmap]]
    assert tri.min(initial=0) >= 0
    pos = smooth(v[vmap], tri, o)
    col = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)[vmap] if rgb is not None else None
    return pos, normals(pos, tri), col, tri.astype(np.int32), vmap.astype(np.int32), tmap.astype(np.int32)
