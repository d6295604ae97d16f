"""numpy restatement of include/esfm.h, "Mesh simplification": grid vertex clustering with the representative placed by the
cell's summed plane quadrics.  It follows the header line by line: f32 cell indices, f64 sums that run sequentially over sorted
lists from +0.0, the LDL^T elimination in the stated order, the orientation vote among triangles on the same three cells, the
ordered compaction, and the clean-up's normals on the output.  numpy's +, -, *, / and sqrt are correctly rounded and never
contracted.  Imports nothing from the library; the GPU tests compare bit patterns against it."""
import numpy as np

import mesh_clean_ref

F = np.float32
D = np.float64
MAX_INDEX = 2 ** 21 - 1
MAX_CELLS = 2 ** 21
LONG_RUN = 64                                                     # runs above this are summed one by one with cumsum


class Rejected(ValueError):
    pass


class Unsupported(ValueError):
    pass


def options(regularisation=1e-3, use_quadric=1):
    return dict(regularisation=regularisation, use_quadric=use_quadric)


def check_options(o):
    eps = F(o["regularisation"])
    if not (np.isfinite(eps) and 0 < eps <= 1 and o["use_quadric"] in (0, 1)):
        raise Rejected(str(o))


def cell_indices(vertices, origin, cell):
    """Per vertex and axis (int)floorf((p - origin) / cell) in f32; a vertex outside 0 .. 2^21 - 1 (or not finite) is rejected."""
    p = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    o, c = np.asarray(origin, F).reshape(3), F(cell)
    if not (np.isfinite(c) and c > 0) or not np.all(np.isfinite(o)):
        raise Rejected("cell must be finite and > 0, origin finite")
    with np.errstate(all="ignore"):
        q = np.floor((p - o) / c)
    assert q.dtype == F
    if not np.all((q >= 0) & (q <= MAX_INDEX)):                   # (NaN fails both comparisons)
        raise Rejected("a vertex lies outside the grid's 2^21 cells per axis")
    return q.astype(np.int64)


def _sequential_segment_sums(start, terms):
    """Per segment s the f64 sum, from +0.0 and in list order, of terms[start[s] .. start[s + 1] - 1]; vectorised over the rank
    within the segment, long segments one by one (cumsum adds in order)."""
    terms = np.asarray(terms)
    n = len(start) - 1
    k = np.diff(start)
    acc = np.zeros((n,) + terms.shape[1:], terms.dtype)
    long_runs = np.nonzero(k > LONG_RUN)[0]
    short = k.copy()
    short[long_runs] = 0
    for r in range(int(short.max()) if n else 0):
        has = np.nonzero(short > r)[0]
        acc[has] = acc[has] + terms[start[has] + r]
    for s in long_runs:
        lead = np.zeros((1,) + terms.shape[1:], terms.dtype)
        acc[s] = np.cumsum(np.concatenate([lead, terms[start[s]:start[s + 1]]]), axis=0)[-1]
    return acc


def cells_of(vertices, origin, cell):
    """(cell_of [V], per-cell integer index [C, 3], the vertex list in (cell, vertex) order, its segment starts [C + 1])."""
    idx = cell_indices(vertices, origin, cell)
    key = (idx[:, 0] << 42) | (idx[:, 1] << 21) | idx[:, 2]
    order = np.argsort(key, kind="stable")                        # ascending vertex index inside a cell
    uniq, first, cell_of = np.unique(key, return_index=True, return_inverse=True)
    start = np.searchsorted(key[order], np.append(uniq, np.iinfo(np.int64).max))
    return cell_of.reshape(-1).astype(np.int64), idx[first], order, start


def quadrics(p, t, cell_of, cc, n_cells):
    """(A [C, 6] in the order 00 01 02 11 12 22, b [C, 3]) about the cell centres cc."""
    keys = np.sort((cell_of[t.reshape(-1)] << 32) | np.arange(3 * len(t), dtype=np.int64))
    start = np.searchsorted(keys >> 32, np.arange(n_cells + 1))
    tri = (keys & 0xFFFFFFFF) // 3
    c = keys >> 32
    p0, p1, p2 = (p[t[tri, k]].astype(D) for k in range(3))
    e1, e2 = p1 - p0, p2 - p0
    N = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                  e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    with np.errstate(all="ignore"):
        L = np.sqrt((N[:, 0] * N[:, 0] + N[:, 1] * N[:, 1]) + N[:, 2] * N[:, 2])
        d0 = p0 - cc[c]
        Dp = -((N[:, 0] * d0[:, 0] + N[:, 1] * d0[:, 1]) + N[:, 2] * d0[:, 2])
        terms = np.stack([N[:, 0] * N[:, 0] / L, N[:, 0] * N[:, 1] / L, N[:, 0] * N[:, 2] / L, N[:, 1] * N[:, 1] / L,
                          N[:, 1] * N[:, 2] / L, N[:, 2] * N[:, 2] / L, N[:, 0] * Dp / L, N[:, 1] * Dp / L, N[:, 2] * Dp / L], 1)
    terms[~(L > 0)] = 0.0                                         # such a corner adds nothing (a sum from +0.0 never holds -0.0)
    assert terms.dtype == D
    s = _sequential_segment_sums(start, terms)
    return s[:, :6], s[:, 6:]


def place(A, b, m, eps, cell, use_quadric):
    """x per cell: the regularised minimiser by LDL^T in the header's order, or m."""
    with np.errstate(all="ignore"):
        tau = (A[:, 0] + A[:, 3]) + A[:, 5]
        r = D(F(eps)) * tau
        M00, M01, M02, M11, M12, M22 = A[:, 0] + r, A[:, 1], A[:, 2], A[:, 3] + r, A[:, 4], A[:, 5] + r
        g = [r * m[:, a] - b[:, a] for a in range(3)]
        d0 = M00
        l10, l20 = M01 / d0, M02 / d0
        d1 = M11 - l10 * M01
        u = M12 - l20 * M01
        l21 = u / d1
        d2 = (M22 - l20 * M02) - l21 * u
        y0 = g[0]
        y1 = g[1] - l10 * y0
        y2 = (g[2] - l20 * y0) - l21 * y1
        x2 = y2 / d2
        x1 = y1 / d1 - l21 * x2
        x0 = (y0 / d0 - l10 * x1) - l20 * x2
        x = np.stack([x0, x1, x2], 1)
        ok = (tau > 0) & np.all(np.abs(x) <= D(F(cell)), axis=1)  # (NaN and inf fail the comparison)
    if not use_quadric:
        ok[:] = False
    return np.where(ok[:, None], x, m)


def vote(t_cells):
    """keep [T] bool by the rule "Triangles", and the number of groups whose orientation surplus is two or more."""
    T = len(t_cells)
    keep = np.zeros(T, bool)
    a, b, c = t_cells[:, 0], t_cells[:, 1], t_cells[:, 2]
    alive = np.nonzero((a != b) & (b != c) & (a != c))[0]
    if len(alive) == 0:
        return keep, 0
    tc = t_cells[alive]
    rot = np.argmin(tc, axis=1)
    r = np.stack([tc[np.arange(len(tc)), (rot + k) % 3] for k in range(3)], 1)
    odd = r[:, 1] > r[:, 2]
    key = (r[:, 0] << 42) | (np.minimum(r[:, 1], r[:, 2]) << 21) | np.maximum(r[:, 1], r[:, 2])
    uniq, inv = np.unique(key, return_inverse=True)
    inv = inv.reshape(-1)
    n_odd = np.bincount(inv, weights=odd, minlength=len(uniq)).astype(np.int64)
    n_even = np.bincount(inv, minlength=len(uniq)) - n_odd
    first = np.full((len(uniq), 2), T, np.int64)                  # lowest triangle number per group and orientation
    np.minimum.at(first, (inv, odd.astype(np.int64)), alive)
    keep[first[n_even > n_odd, 0]] = True
    keep[first[n_odd > n_even, 1]] = True
    return keep, int(np.count_nonzero(np.abs(n_even - n_odd) >= 2))


def simplify_detail(vertices, rgb, triangles, cell, origin, o=None, want_rgb=None):
    """esfm_mesh_simplify with what the tests look at besides its outputs."""
    o = o or options()
    check_options(o)
    if want_rgb and rgb is None:
        raise Rejected("an output array is requested without its input")
    p = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    try:
        t = mesh_clean_ref._triangles(triangles, len(p))
    except mesh_clean_ref.Rejected as e:
        raise Rejected(str(e))
    cell_of, idx, order, start = cells_of(p, origin, cell)
    C = len(idx)
    empty = dict(vertices=np.zeros((0, 3), F), normals=np.zeros((0, 3), F), rgb=np.zeros((0, 3), np.uint8) if rgb is not None else None,
                 triangles=np.zeros((0, 3), np.int32), vertex_map=np.full(len(p), -1, np.int32), triangle_map=np.zeros(0, np.int32),
                 n_cells=C, surplus2=0, A=np.zeros((0, 6)), b=np.zeros((0, 3)), cell_of=cell_of)
    if len(t) == 0 or C == 0:
        return empty
    if C > MAX_CELLS:
        raise Unsupported(f"{C} cells")
    cc = np.asarray(origin, F).reshape(3).astype(D) + (idx.astype(D) + 0.5) * D(F(cell))
    n = np.diff(start)
    m = _sequential_segment_sums(start, p[order].astype(D) - cc[cell_of[order]]) / n[:, None].astype(D)
    col = None
    if rgb is not None:
        c8 = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3).astype(np.int64)
        sums = np.stack([np.bincount(cell_of, weights=c8[:, k], minlength=C) for k in range(3)], 1).astype(np.int64)
        col = ((2 * sums + n[:, None]) // (2 * n[:, None])).astype(np.uint8)
    A, b = quadrics(p, t, cell_of, cc, C)
    x = place(A, b, m, o["regularisation"], cell, o["use_quadric"])
    rep = (cc + x).astype(F)
    keep, surplus2 = vote(cell_of[t])
    tmap = np.nonzero(keep)[0]
    if len(tmap) == 0:
        empty.update(A=A, b=b)
        return empty
    used = np.zeros(C, bool)
    used[cell_of[t[tmap]].reshape(-1)] = True
    new_of_cell = np.where(used, np.cumsum(used) - 1, -1)
    out_v = rep[used]
    out_t = new_of_cell[cell_of[t[tmap]]]
    return dict(vertices=out_v, normals=mesh_clean_ref.normals(out_v, out_t), rgb=col[used] if col is not None else None,
                triangles=out_t.astype(np.int32), vertex_map=new_of_cell[cell_of].astype(np.int32), triangle_map=tmap.astype(np.int32),
                n_cells=C, surplus2=surplus2, A=A, b=b, cell_of=cell_of)


def simplify(vertices, rgb, triangles, cell, origin, o=None, want_rgb=None):
    """esfm_mesh_simplify: (vertices, normals, rgb or None, triangles, vertex_map [V], triangle_map)."""
    d = simplify_detail(vertices, rgb, triangles, cell, origin, o, want_rgb)
    return d["vertices"], d["normals"], d["rgb"], d["triangles"], d["vertex_map"], d["triangle_map"]
