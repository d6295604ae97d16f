"""Numpy f32 restatement of include/esfm.h "Dense reconstruction", written from the header text: the plan rules, the plane
inverse depths and homographies, the plane sweep and the fusion.  It vectorises over pixels and loops over taps, sources
and planes in the stated order; window sums are explicit loops (never np.sum / np.mean over a window, whose pairwise
summation would reorder the adds).  It calls no product code."""
import math

import numpy as np

F = np.float32
INF = F(np.inf)

DEFAULTS = dict(num_planes=128, window_radius=3, max_neighbours=4, min_shared_points=20, best_k=2, depth_margin=0.25, max_cost=0.5,
                min_var=4.0, fuse_min_views=2, fuse_reproj_px=1.0, fuse_rel_depth=0.01)


def options(**kw):
    o = dict(DEFAULTS)
    o.update(kw)
    return o


def grey(images):
    """[n, rows, cols(, 1 | 3)] u8 -> [n, rows, cols] f32 grey levels (cvtColor BGR2GRAY's 14-bit fixed point for BGR)."""
    im = np.asarray(images, np.uint8)
    if im.ndim == 3:
        return im.astype(F)
    if im.shape[3] == 1:
        return im[..., 0].astype(F)
    b, g, r = (im[..., c].astype(np.int32) for c in range(3))
    return ((b * 1868 + g * 9617 + r * 4899 + 8192) >> 14).astype(F)


# ---- plan -----------------------------------------------------------------------------------------------------------------
def plan(registered, poses, xyz, obs_offsets, obs_points, opt):
    n = len(registered)
    nb = opt["max_neighbours"]
    P = np.asarray(poses, F).reshape(n, 12)
    X = np.asarray(xyz, F).reshape(-1, 3)
    obs = [set(int(p) for p in obs_points[obs_offsets[v]:obs_offsets[v + 1]]) if registered[v] else set() for v in range(n)]
    neighbours = np.full((n, nb), -1, np.int32)
    rng = np.zeros((n, 2), F)
    for r in range(n):
        if not registered[r]:
            continue
        cand = [(-len(obs[r] & obs[v]), v) for v in range(n) if v != r and registered[v]]
        cand = sorted(c for c in cand if -c[0] >= opt["min_shared_points"])
        for j, (_, v) in enumerate(cand[:nb]):
            neighbours[r, j] = v
        if not cand:
            continue
        idx = np.array(sorted(obs[r]), np.int64)
        if len(idx) == 0:
            continue
        Xr = X[idx]
        z = ((P[r, 8] * Xr[:, 0] + P[r, 9] * Xr[:, 1]) + P[r, 10] * Xr[:, 2]) + P[r, 11]
        z = np.sort(z[z > 0])
        if len(z) < 10:
            continue
        lo, hi = z[math.floor(0.02 * (len(z) - 1))], z[math.ceil(0.98 * (len(z) - 1))]
        g = F(1) + F(opt["depth_margin"])
        rng[r] = (lo / g, hi * g)
    return neighbours, rng


# ---- planes and homographies ----------------------------------------------------------------------------------------------
def planes(d_min, d_max, D):
    """(step, [invd_k] as Python floats (double))."""
    step = (1.0 / float(d_min) - 1.0 / float(d_max)) / (D - 1)
    return step, [1.0 / float(d_max) + k * step for k in range(D)]


def homography(Kr, Pr, Ks, Ps, invd):
    """H_k of source s for reference r, double with explicit scalar loops, each entry rounded to f32 once."""
    Pr = [float(v) for v in np.asarray(Pr, F).reshape(12)]
    Ps = [float(v) for v in np.asarray(Ps, F).reshape(12)]
    Rr = [[Pr[4 * i + j] for j in range(3)] for i in range(3)]
    Rs = [[Ps[4 * i + j] for j in range(3)] for i in range(3)]
    tr = [Pr[4 * i + 3] for i in range(3)]
    ts = [Ps[4 * i + 3] for i in range(3)]
    Rsr = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            s = 0.0
            for l in range(3):
                s += Rs[i][l] * Rr[j][l]
            Rsr[i][j] = s
    tsr = [0.0] * 3
    for i in range(3):
        s = 0.0
        for l in range(3):
            s += Rsr[i][l] * tr[l]
        tsr[i] = ts[i] - s
    M = [row[:] for row in Rsr]
    for i in range(3):
        M[i][2] += tsr[i] * invd
    fx, cx, fy, cy = (float(v) for v in np.asarray(Kr, F))
    Ki = [[1 / fx, 0.0, -cx / fx], [0.0, 1 / fy, -cy / fy], [0.0, 0.0, 1.0]]
    ks = [float(v) for v in np.asarray(Ks, F)]
    Kt = [[ks[0], 0.0, ks[1]], [0.0, ks[2], ks[3]], [0.0, 0.0, 1.0]]
    A = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            s = 0.0
            for l in range(3):
                s += M[i][l] * Ki[l][j]
            A[i][j] = s
    H = np.zeros(9, F)
    for i in range(3):
        for j in range(3):
            s = 0.0
            for l in range(3):
                s += Kt[i][l] * A[l][j]
            H[3 * i + j] = F(s)
    return H


def warp(src, H):
    """Warped value of every reference pixel (f32) and its validity."""
    rows, cols = src.shape
    ys, xs = np.mgrid[0:rows, 0:cols]
    x, y = xs.astype(F), ys.astype(F)
    h = [F(v) for v in H]
    with np.errstate(all="ignore"):
        w = (h[6] * x + h[7] * y) + h[8]
        nu = (h[0] * x + h[1] * y) + h[2]
        nv = (h[3] * x + h[4] * y) + h[5]
        u, v = nu / w, nv / w
        x0, y0 = np.floor(u), np.floor(v)
        valid = (w > 0) & (x0 >= 0) & (x0 + F(1) < F(cols)) & (y0 >= 0) & (y0 + F(1) < F(rows))
        fx, fy = u - x0, v - y0
    ix = np.where(valid, x0, 0).astype(np.int64)
    iy = np.where(valid, y0, 0).astype(np.int64)
    i00, i01, i10, i11 = src[iy, ix], src[iy, ix + valid], src[iy + valid, ix], src[iy + valid, ix + valid]
    one = F(1)
    with np.errstate(all="ignore"):
        val = (one - fy) * ((one - fx) * i00 + fx * i01) + fy * ((one - fx) * i10 + fx * i11)
    return val.astype(F), valid


# ---- plane sweep ----------------------------------------------------------------------------------------------------------
def depth_maps(images, K4, poses, neighbours, depth_range, opt):
    g = grey(images)
    n, rows, cols = g.shape
    K4 = np.asarray(K4, F).reshape(n, 4)
    P = np.asarray(poses, F).reshape(n, 12)
    nbr = np.asarray(neighbours, np.int32).reshape(n, -1)
    D, r, best_k = opt["num_planes"], opt["window_radius"], opt["best_k"]
    nt = (2 * r + 1) ** 2
    N = F(nt)
    nmv = F(nt) * F(opt["min_var"])
    max_cost = F(opt["max_cost"])
    depth = np.zeros((n, rows, cols), F)
    cost = np.full((n, rows, cols), INF, F)
    ir, ic = rows - 2 * r, cols - 2 * r                  # pixels whose window stays inside: [r, rows - r) x [r, cols - r)

    def taps(img):
        for dy in range(2 * r + 1):
            for dx in range(2 * r + 1):
                yield img[dy:dy + ir, dx:dx + ic]

    for v in range(n):
        lo, hi = depth_range[v]
        if not lo > 0:
            continue
        srcs = [int(s) for s in nbr[v] if s >= 0]
        step, invd = planes(lo, hi, D)
        ref = g[v]
        s = np.zeros((ir, ic), F)
        for t in taps(ref):
            s = s + t
        mr = s / N
        vr = np.zeros((ir, ic), F)
        for t in taps(ref):
            d = t - mr
            vr = vr + d * d
        ref_ok = ~(vr < nmv)
        best = np.full((ir, ic), INF, F)
        best_i = np.full((ir, ic), -1, np.int64)
        c_prev = np.full((ir, ic), INF, F)
        c_lo = np.full((ir, ic), INF, F)
        c_hi = np.full((ir, ic), INF, F)
        for k in range(D):
            costs = []
            for sv in srcs:
                val, ok = warp(g[sv], homography(K4[v], P[v], K4[sv], P[sv], invd[k]))
                ss = np.zeros((ir, ic), F)
                bad = np.zeros((ir, ic), bool)
                for t, tok in zip(taps(val), taps(ok)):
                    ss = ss + t
                    bad |= ~tok
                ms = ss / N
                cov = np.zeros((ir, ic), F)
                vs = np.zeros((ir, ic), F)
                for tr_, ts_ in zip(taps(ref), taps(val)):
                    dr, ds = tr_ - mr, ts_ - ms
                    cov = cov + dr * ds
                    vs = vs + ds * ds
                with np.errstate(all="ignore"):
                    c = F(1) - cov / np.sqrt(vr * vs)
                good = ref_ok & ~bad & ~(vs < nmv)
                costs.append(np.where(good, c, INF).astype(F))
            if costs:
                cs = np.sort(np.stack(costs), axis=0)
                nvalid = np.sum(cs != INF, axis=0)
                m = np.minimum(nvalid, best_k)
                acc = cs[0]
                for j in range(1, len(srcs)):
                    acc = np.where(j < m, acc + cs[j], acc)
                with np.errstate(all="ignore"):
                    ck = np.where(nvalid > 0, acc / np.maximum(m, 1).astype(F), INF).astype(F)
            else:
                ck = np.full((ir, ic), INF, F)
            c_hi = np.where((best_i >= 0) & (best_i == k - 1), ck, c_hi)
            upd = ck < best
            best = np.where(upd, ck, best)
            best_i = np.where(upd, k, best_i)
            c_lo = np.where(upd, c_prev, c_lo)
            c_hi = np.where(upd, INF, c_hi)
            c_prev = ck
        ok = (best_i > 0) & (best_i < D - 1) & ~(best > max_cost)
        with np.errstate(all="ignore"):
            den = (c_lo - F(2) * best) + c_hi
            off = np.where(den > 0, F(0.5) * (c_lo - c_hi) / den, F(0))
            off = np.minimum(np.maximum(off, F(-0.5)), F(0.5))
        off = np.where((c_lo == INF) | (c_hi == INF), F(0), off).astype(F)
        invd_f = np.array(invd, np.float64).astype(F)
        with np.errstate(all="ignore"):
            dep = F(1) / (invd_f[np.clip(best_i, 0, D - 1)] + off * F(step))
        depth[v, r:r + ir, r:r + ic] = np.where(ok, dep, F(0))
        cost[v, r:r + ir, r:r + ic] = best
    return depth, cost


# ---- fusion ---------------------------------------------------------------------------------------------------------------
def backproject(K, P, x, y, d):
    e0 = ((x - K[1]) / K[0]) * d - P[3]
    e1 = ((y - K[3]) / K[2]) * d - P[7]
    e2 = d - P[11]
    return [(P[j] * e0 + P[4 + j] * e1) + P[8 + j] * e2 for j in range(3)]


def to_camera(P, X):
    return [((P[4 * i] * X[0] + P[4 * i + 1] * X[1]) + P[4 * i + 2] * X[2]) + P[4 * i + 3] for i in range(3)]


def fuse(images, K4, poses, neighbours, depth, opt):
    im = np.asarray(images, np.uint8)
    if im.ndim == 3:
        im = im[..., None]
    n, rows, cols, ch = im.shape
    K4 = np.asarray(K4, F).reshape(n, 4)
    P = np.asarray(poses, F).reshape(n, 12)
    nbr = np.asarray(neighbours, np.int32).reshape(n, -1)
    dep = np.asarray(depth, F).reshape(n, rows, cols)
    rp2 = F(opt["fuse_reproj_px"]) * F(opt["fuse_reproj_px"])
    rel = F(opt["fuse_rel_depth"])
    out_xyz, out_rgb = [], []
    for v in range(n):
        ys, xs = np.nonzero(dep[v] > 0)                  # row-major order
        d = dep[v][ys, xs]
        x, y = xs.astype(F), ys.astype(F)
        K, Pv = K4[v], P[v]
        X = backproject(K, Pv, x, y, d)
        acc = [c.copy() for c in X]
        count = np.zeros(len(d), np.int32)
        with np.errstate(all="ignore"):
            for s in nbr[v]:
                if s < 0:
                    continue
                Ks, Ps = K4[s], P[s]
                p = to_camera(Ps, X)
                ok = p[2] > 0
                u = Ks[0] * (p[0] / p[2]) + Ks[1]
                w = Ks[2] * (p[1] / p[2]) + Ks[3]
                px, py = np.floor(u + F(0.5)), np.floor(w + F(0.5))
                ok &= (px >= 0) & (px < F(cols)) & (py >= 0) & (py < F(rows))
                ix = np.where(ok, px, 0).astype(np.int64)
                iy = np.where(ok, py, 0).astype(np.int64)
                ds = dep[s][iy, ix]
                ok &= ds > 0
                Y = backproject(Ks, Ps, px, py, ds)
                q = to_camera(Pv, Y)
                du = (K[0] * (q[0] / q[2]) + K[1]) - x
                dv = (K[2] * (q[1] / q[2]) + K[3]) - y
                cons = ok & (du * du + dv * dv < rp2) & (np.abs(q[2] - d) < rel * d)
                acc = [np.where(cons, a + b, a) for a, b in zip(acc, Y)]
                count += cons
        keep = count >= opt["fuse_min_views"]
        cnt = (1 + count[keep]).astype(F)
        out_xyz.append(np.stack([a[keep] / cnt for a in acc], axis=1).astype(F))
        px = im[v][ys[keep], xs[keep]]
        out_rgb.append(px[:, ::-1] if ch == 3 else np.repeat(px, 3, axis=1))
    return np.concatenate(out_xyz).reshape(-1, 3), np.concatenate(out_rgb).reshape(-1, 3).astype(np.uint8)
