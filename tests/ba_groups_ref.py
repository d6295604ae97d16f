"""Numpy reference for bundle adjustment with G free intrinsics blocks (multiple-camera mode), for the tests only.

A restatement of Ceres' bounded Levenberg-Marquardt loop as the reference project configures it (DENSE_SCHUR, Jacobi scaling,
CauchyLoss(0.5), box bounds on the intrinsics and on the reference camera), in the form tests/golden/make_golden.py states it for
one block -- projection at iteration 0, Plus() projects, projected gradient norm, Armijo search with the cubic step rule, Jacobi
scaling, the radius rule -- generalised to one block fx, cx, fy, cy per camera group.  It shares no code with the library.

Unknown vector: cameras (6 each) | points (3 each) | intrinsics blocks (4 each).  The Jacobian is analytic (both angle-axis
branches) and kept in blocks per observation; the step comes either from the dense normal equations (small cases) or from the
point-eliminated reduced system of 6 n_cam + 4 G unknowns, built with one matrix product per distinct camera tuple of the tracks.
"""
import numpy as np

EPS = np.finfo(np.float64).eps
TINY = np.finfo(np.float64).tiny


def _skew(v):
    z = np.zeros(len(v))
    return np.stack([np.stack([z, -v[:, 2], v[:, 1]], 1), np.stack([v[:, 2], z, -v[:, 0]], 1), np.stack([-v[:, 1], v[:, 0], z], 1)], 1)


def residual_jac(cams, pts, calib, grp, cam_idx, pt_idx, uv, jac=True):
    """ReprojectErrorTerm_updatecalib with the block of the observation's camera's group.
    Returns r [n, 2] and, with jac, Jc [n, 2, 6], Jp [n, 2, 3], Jk [n, 2, 4] (all before the loss)."""
    a = cams[cam_idx, :3]; t = cams[cam_idx, 3:]; X = pts[pt_idx]
    k = calib[grp[cam_idx]]
    th2 = (a * a).sum(1)
    big = th2 > EPS
    th = np.sqrt(np.where(big, th2, 1.0))
    s, c = np.sin(th), np.cos(th)
    alpha = np.where(big, s / th, 1.0)
    beta = np.where(big, (1.0 - c) / (th * th), 0.0)
    cs = np.where(big, c, 1.0)
    axX = np.cross(a, X)
    aX = (a * X).sum(1)
    p = cs[:, None] * X + alpha[:, None] * axX + (beta * aX)[:, None] * a + t
    iz = 1.0 / p[:, 2]
    x, y = p[:, 0] * iz, p[:, 1] * iz
    fx, cx, fy, cy = k[:, 0], k[:, 1], k[:, 2], k[:, 3]
    uvd = np.asarray(uv, np.float32).astype(np.float64)
    r = np.stack([uvd[:, 0] - (x * fx + cx), uvd[:, 1] - (y * fy + cy)], 1)
    if not jac:
        return r
    n = len(cam_idx)
    I = np.broadcast_to(np.eye(3), (n, 3, 3))
    aa = a[:, :, None] * a[:, None, :]
    R = cs[:, None, None] * I + alpha[:, None, None] * _skew(a) + beta[:, None, None] * aa
    # d p / d a: derivative of cos, of sin / theta and of (1 - cos) / theta^2 through theta, then of a x X and a (a.X)
    gamma = np.where(big, (c - alpha) / (th * th), 0.0)
    delta = np.where(big, (alpha - 2.0 * beta) / (th * th), 0.0)
    dcos = np.where(big, -alpha, 0.0)
    Ja = (dcos[:, None, None] * X[:, :, None] * a[:, None, :] + gamma[:, None, None] * axX[:, :, None] * a[:, None, :]
          - alpha[:, None, None] * _skew(X) + (delta * aX)[:, None, None] * aa
          + beta[:, None, None] * (aX[:, None, None] * I + a[:, :, None] * X[:, None, :]))
    z = np.zeros(n)
    drdp = np.stack([np.stack([-fx * iz, z, fx * x * iz], 1), np.stack([z, -fy * iz, fy * y * iz], 1)], 1)
    Jc = np.concatenate([drdp @ Ja, drdp], 2)
    Jp = drdp @ R
    o = np.ones(n)
    Jk = np.stack([np.stack([-x, -o, z, z], 1), np.stack([z, z, -y, -o], 1)], 1)
    return r, Jc, Jp, Jk


def _loss(r, cauchy_a):
    s = (r * r).sum(1)
    if cauchy_a > 0:
        b = cauchy_a * cauchy_a
        return b * np.log1p(s / b), np.maximum(1.0 / (1.0 + s / b), TINY)
    return s, np.ones_like(s)


def armijo_next_step(f0, g0, prev, cur, lo, hi):
    """Ceres' CUBIC interpolation: the minimiser over [lo, hi] of the polynomial through the value and slope at 0 and at the last
    one or two trial points (x, f, g)."""
    samples = [(0.0, f0, g0), cur] + ([prev] if prev is not None else [])
    deg = 2 * len(samples)
    A, b = [], []
    for (x, f, g) in samples:
        A.append([x ** j for j in range(deg)]); b.append(f)
        A.append([0.0] + [j * x ** (j - 1) for j in range(1, deg)]); b.append(g)
    coef = np.linalg.solve(np.array(A), np.array(b))
    poly = np.polynomial.Polynomial(coef)
    cands = [(lo + hi) / 2.0, lo, hi] + [float(np.real(zr)) for zr in np.roots(poly.deriv().coef[::-1]) if lo <= np.real(zr) <= hi]
    best = cands[0]
    for cnd in cands[1:]:
        if poly(cnd) < poly(best):
            best = cnd
    return best


class Problem:
    def __init__(self, cam_idx, pt_idx, uv, grp, cams0, pts0, calib0, tol, ref_cam=-1, ref_thr=1e-10, cauchy_a=0.5):
        self.cam_idx = np.asarray(cam_idx, np.int64); self.pt_idx = np.asarray(pt_idx, np.int64)
        self.uv = np.asarray(uv, np.float32)
        self.grp = np.asarray(grp, np.int64)
        self.n_cam, self.n_pt = len(cams0), len(pts0)
        calib0 = np.asarray(calib0, np.float64).reshape(-1, 4)
        self.G = len(calib0)
        self.n_obs = len(self.cam_idx)
        self.gidx = self.grp[self.cam_idx]
        self.cauchy_a = cauchy_a
        self.ko = 6 * self.n_cam + 3 * self.n_pt
        self.npar = self.ko + 4 * self.G
        self.x0 = np.concatenate([np.asarray(cams0, np.float64).ravel(), np.asarray(pts0, np.float64).ravel(), calib0.ravel()])
        # blocks that take part in the problem (Ceres drops the others with their bounds)
        act = np.zeros(self.npar, bool)
        act[:6 * self.n_cam] = np.repeat(np.bincount(self.cam_idx, minlength=self.n_cam) > 0, 6)
        act[6 * self.n_cam:self.ko] = np.repeat(np.bincount(self.pt_idx, minlength=self.n_pt) > 0, 3)
        act[self.ko:] = np.repeat(np.bincount(self.gidx, minlength=self.G) > 0, 4)
        self.active = act
        self.lo = np.full(self.npar, -np.inf); self.up = np.full(self.npar, np.inf)
        tol = np.broadcast_to(np.asarray(tol, np.float64), (self.G,))
        self.lo[self.ko:] = (calib0 - tol[:, None]).ravel(); self.up[self.ko:] = (calib0 + tol[:, None]).ravel()
        if ref_cam >= 0:
            self.lo[6 * ref_cam:6 * ref_cam + 6] = -ref_thr; self.up[6 * ref_cam:6 * ref_cam + 6] = ref_thr
        self.lo[~act] = -np.inf; self.up[~act] = np.inf
        # column index of the ten camera-side unknowns of every observation in the reduced system
        self.idx10 = np.concatenate([6 * self.cam_idx[:, None] + np.arange(6)[None, :],
                                     6 * self.n_cam + 4 * self.gidx[:, None] + np.arange(4)[None, :]], 1)
        self._tuples = None

    # ---- parameter vector ----
    def split(self, x):
        return x[:6 * self.n_cam].reshape(-1, 6), x[6 * self.n_cam:self.ko].reshape(-1, 3), x[self.ko:].reshape(-1, 4)

    def plus(self, x, d):
        return np.minimum(np.maximum(x + d, self.lo), self.up)

    def cost(self, x):
        cams, pts, cal = self.split(x)
        rho0, _ = _loss(residual_jac(cams, pts, cal, self.grp, self.cam_idx, self.pt_idx, self.uv, jac=False), self.cauchy_a)
        return 0.5 * rho0.sum()

    def evaluate(self, x):
        """cost, loss-corrected residual [n, 2] and Jacobian blocks F [n, 2, 6], E [n, 2, 3], K [n, 2, 4]"""
        cams, pts, cal = self.split(x)
        r, Jc, Jp, Jk = residual_jac(cams, pts, cal, self.grp, self.cam_idx, self.pt_idx, self.uv)
        rho0, rho1 = _loss(r, self.cauchy_a)
        sq = np.sqrt(rho1)
        return 0.5 * rho0.sum(), r * sq[:, None], Jc * sq[:, None, None], Jp * sq[:, None, None], Jk * sq[:, None, None]

    # ---- block operations: vectors in the layout of x ----
    def _scatter(self, wc, wp, wk):
        out = np.zeros(self.npar)
        for j in range(6):
            out[j:6 * self.n_cam:6] = np.bincount(self.cam_idx, weights=wc[:, j], minlength=self.n_cam)
        for j in range(3):
            out[6 * self.n_cam + j:self.ko:3] = np.bincount(self.pt_idx, weights=wp[:, j], minlength=self.n_pt)
        for j in range(4):
            out[self.ko + j::4] = np.bincount(self.gidx, weights=wk[:, j], minlength=self.G)
        return out

    def Jt(self, F, E, K, v):
        return self._scatter(np.einsum("nra,nr->na", F, v), np.einsum("nra,nr->na", E, v), np.einsum("nra,nr->na", K, v))

    def colsq(self, F, E, K):
        return self._scatter((F * F).sum(1), (E * E).sum(1), (K * K).sum(1))

    def Jv(self, F, E, K, d):
        dc, dp, dk = self.split(d)
        return (np.einsum("nra,na->nr", F, dc[self.cam_idx]) + np.einsum("nra,na->nr", E, dp[self.pt_idx])
                + np.einsum("nra,na->nr", K, dk[self.gidx]))

    def scaled(self, F, E, K, scale):
        sc, sp, sk = self.split(scale)
        return F * sc[self.cam_idx][:, None, :], E * sp[self.pt_idx][:, None, :], K * sk[self.gidx][:, None, :]

    def dense_jacobian(self, F, E, K):
        J = np.zeros((2 * self.n_obs, self.npar))
        rows = np.arange(self.n_obs)
        for i in range(2):
            for j in range(6):
                J[2 * rows + i, 6 * self.cam_idx + j] = F[:, i, j]
            for j in range(3):
                J[2 * rows + i, 6 * self.n_cam + 3 * self.pt_idx + j] = E[:, i, j]
            for j in range(4):
                J[2 * rows + i, self.ko + 4 * self.gidx + j] = K[:, i, j]
        return J

    # ---- the LM step: (J'J + D) step = -J'r ----
    def step_dense(self, F, E, K, r, D):
        J = self.dense_jacobian(F, E, K)
        return -np.linalg.solve(J.T @ J + np.diag(D), J.T @ r.ravel())

    def _track_tuples(self):
        """observations grouped by track, the tracks grouped by their tuple of cameras: [(points [P], observations [P, T])]"""
        if self._tuples is None:
            order = np.argsort(self.pt_idx, kind="stable")
            cnt = np.bincount(self.pt_idx, minlength=self.n_pt)
            start = np.concatenate([[0], np.cumsum(cnt)])
            out = []
            for T in np.unique(cnt[cnt > 0]):
                pts_T = np.nonzero(cnt == T)[0]
                obs = order[start[pts_T][:, None] + np.arange(T)[None, :]]
                _, inv = np.unique(self.cam_idx[obs], axis=0, return_inverse=True)
                inv = inv.reshape(-1)
                for u in range(inv.max() + 1):
                    sel = inv == u
                    out.append((pts_T[sel], obs[sel]))
            self._tuples = out
        return self._tuples

    def step_schur(self, F, E, K, r, D):
        nc6 = 6 * self.n_cam
        nred = nc6 + 4 * self.G
        Dc = np.concatenate([D[:nc6], D[self.ko:]]); Dp = D[nc6:self.ko].reshape(-1, 3)
        F10 = np.concatenate([F, K], 2)
        EtE = np.zeros((self.n_pt, 3, 3)); Etr = np.zeros((self.n_pt, 3))
        for i in range(3):
            Etr[:, i] = np.bincount(self.pt_idx, weights=(E[:, :, i] * r).sum(1), minlength=self.n_pt)
            for j in range(3):
                EtE[:, i, j] = np.bincount(self.pt_idx, weights=(E[:, :, i] * E[:, :, j]).sum(1), minlength=self.n_pt)
        Minv = np.linalg.inv(EtE + Dp[:, :, None] * np.eye(3)[None])
        S = np.diag(Dc).copy()
        rhs = np.zeros(nred)
        for pts_u, obs in self._track_tuples():
            T = obs.shape[1]
            Fu, Eu, ru = F10[obs], E[obs], r[obs]
            cols = self.idx10[obs[0]]                                             # [T, 10]
            Ft = Fu.transpose(1, 0, 2, 3).reshape(T, -1, 10)                      # slot t of the tuple: [2 P, 10]
            FtF = Ft.transpose(0, 2, 1) @ Ft
            Ftr = (Ft.transpose(0, 2, 1) @ ru.transpose(1, 0, 2).reshape(T, -1, 1))[:, :, 0]
            for t in range(T):
                np.add.at(S, (cols[t][:, None], cols[t][None, :]), FtF[t])
                np.add.at(rhs, cols[t], Ftr[t])
            U = (Fu.transpose(0, 1, 3, 2) @ Eu).reshape(len(pts_u), 10 * T, 3)    # W of every point: rows = its 10 T camera-side columns
            V = U @ Minv[pts_u]
            flat = cols.reshape(-1)
            Vf = V.transpose(1, 0, 2).reshape(10 * T, -1); Uf = U.transpose(1, 0, 2).reshape(10 * T, -1)    # [10 T, 3 P]: one product per tuple
            np.subtract.at(S, (flat[:, None], flat[None, :]), Vf @ Uf.T)
            np.subtract.at(rhs, flat, Vf @ Etr[pts_u].reshape(-1))
        yc = -np.linalg.solve(S, rhs)
        f = np.einsum("nra,na->nr", F10, yc[self.idx10])
        Wt = np.zeros((self.n_pt, 3))
        for i in range(3):
            Wt[:, i] = np.bincount(self.pt_idx, weights=(E[:, :, i] * f).sum(1), minlength=self.n_pt)
        yp = -np.einsum("pij,pj->pi", Minv, Etr + Wt)
        return np.concatenate([yc[:nc6], yp.ravel(), yc[nc6:]])


def solve(prob, max_iter, method="schur"):
    """The bounded LM loop.  Returns (x, log); log entries: cost, radius, step_norm, ok, gmax, ls, and for the stability checks rho
    (None where no ratio was formed) and armijo (the relative margin of every Armijo test of the iteration)."""
    P = prob
    stepper = P.step_schur if method == "schur" else P.step_dense

    def pgrad_norm(x, g):
        return np.abs(x - P.plus(x, -g)).max()

    def xnorm(x):
        return np.linalg.norm(x[P.active])

    x = P.plus(P.x0, 0.0)
    cost, r, F, E, K = P.evaluate(x)
    grad = P.Jt(F, E, K, r)
    scale = 1.0 / (1.0 + np.sqrt(P.colsq(F, E, K)))
    F, E, K = P.scaled(F, E, K, scale)
    radius, nu = 1e4, 2.0
    x_norm = xnorm(x)
    log = [dict(cost=cost, radius=radius, step_norm=0.0, ok=1, gmax=pgrad_norm(x, grad), ls=0, rho=None, armijo=[])]
    for it in range(1, max_iter + 1):
        D = np.clip(P.colsq(F, E, K), 1e-6, 1e32) / radius
        step = stepper(F, E, K, r, D)
        m = P.Jv(F, E, K, step)
        mcc = -(m * (r + m / 2.0)).sum()
        delta = step * scale
        g0 = grad @ delta
        dmax = np.abs(delta).max()

        trial = {}                    # the last trial point and its evaluation: the candidate is usually that very point

        def phi(t):
            xt = P.plus(x, t * delta)
            f, rr, FF, EE, KK = trial["ev"] = P.evaluate(xt)
            trial["x"] = xt
            return f, P.Jt(FF, EE, KK, rr) @ delta

        margins = []
        prev, n_ls, ls_ok = None, 0, True
        f, g = phi(1.0); cur = (1.0, f, g)
        while True:
            bound = cost + 1e-4 * g0 * cur[0]
            margins.append(abs(cur[1] - bound) / max(abs(cost), TINY))
            if not cur[1] > bound:
                break
            n_ls += 1
            if n_ls >= 20:
                ls_ok = False; break
            t = armijo_next_step(cost, g0, prev, cur, 1e-3 * cur[0], 0.6 * cur[0])
            if t * dmax < 1e-9:
                ls_ok = False; break
            prev = cur
            f, g = phi(t); cur = (t, f, g)
        if ls_ok:
            delta = delta * cur[0]
        cand = P.plus(x, delta)
        at_trial = np.array_equal(cand, trial["x"])
        ccost = trial["ev"][0] if at_trial else P.cost(cand)
        step_norm = np.linalg.norm(x - cand)
        if step_norm <= 1e-8 * (x_norm + 1e-8) or abs(cost - ccost) <= 1e-6 * cost:
            log.append(dict(cost=cost, radius=radius, step_norm=step_norm, ok=0, gmax=log[-1]["gmax"], ls=n_ls, rho=None, armijo=margins, stop=1))
            break
        rho = (cost - ccost) / mcc
        if rho > 1e-3:
            x = cand; x_norm = xnorm(x)
            cost, r, F, E, K = trial["ev"] if at_trial else P.evaluate(x)
            grad = P.Jt(F, E, K, r)
            F, E, K = P.scaled(F, E, K, scale)
            radius = min(1e16, radius / max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3)); nu = 2.0
            log.append(dict(cost=cost, radius=radius, step_norm=step_norm, ok=1, gmax=pgrad_norm(x, grad), ls=n_ls, rho=rho, armijo=margins))
        else:
            radius /= nu; nu *= 2.0
            log.append(dict(cost=ccost, radius=radius, step_norm=step_norm, ok=0, gmax=log[-1]["gmax"], ls=n_ls, rho=rho, armijo=margins))
    return x, log


def stability(log):
    """(smallest |rho - 1e-3|, smallest relative Armijo margin) over the trace: how far every accept / contract decision is from a tie"""
    rhos = [abs(e["rho"] - 1e-3) for e in log if e["rho"] is not None]
    arm = [mg for e in log for mg in e["armijo"]]
    return (min(rhos) if rhos else np.inf), (min(arm) if arm else np.inf)
