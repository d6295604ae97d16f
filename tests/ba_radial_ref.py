"""Numpy reference for bundle adjustment with free radial distortion per camera group, for the tests only.

The bounded Levenberg-Marquardt loop of tests/ba_groups_ref.py (its `solve`, loss, Armijo rule and pinhole Jacobian are imported)
over blocks fx, cx, fy, cy, k1, k2 -- 6 wide -- with the model of DESIGN.md section 5.6:

    x = p0/p2, y = p1/p2, r2 = x^2 + y^2, L = 1 + k1 r2 + k2 r2^2,    r = uv - (fx x L + cx, fy y L + cy).

The radial Jacobian is the pinhole one behind the chain rule through (x, y) -> (x L, y L): with D = 2 k1 + 4 k2 r2,
a00 = L + x^2 D, a01 = x y D, a11 = L + y^2 D, and the pinhole rows row0 = -fx dx/d., row1 = -fy dy/d.,

    radial row 0 = a00 row0 + a01 (fx / fy) row1,      radial row 1 = a01 (fy / fx) row0 + a11 row1.

`radial=False` takes k1, k2 out of the unknowns (the block is 4 wide, the coefficients stay where they start): with k = 0 that is
ba_groups_ref's problem, and tests/test_ba_radial_cpu.py holds its trace to that module's, bit for bit.

Unknown vector: cameras (6 each) | points (3 each) | blocks (W each, W = 6 or 4).
"""
import numpy as np

import ba_groups_ref as ref
from ba_groups_ref import _loss, solve, stability  # noqa: F401  (the loop and its helpers, re-exported for the tests)


def residual_jac(cams, pts, calib6, grp, cam_idx, pt_idx, uv, jac=True):
    """r [n, 2] and, with jac, Jc [n, 2, 6], Jp [n, 2, 3], Jk [n, 2, 6] (before the loss); calib6 [G, 6] = fx, cx, fy, cy, k1, k2"""
    k = calib6[grp[cam_idx]]
    r_pin, Jc, Jp, Jk4 = ref.residual_jac(cams, pts, calib6[:, :4], grp, cam_idx, pt_idx, uv)
    x, y = -Jk4[:, 0, 0], -Jk4[:, 1, 2]
    fx, cx, fy, cy, k1, k2 = (k[:, i] for i in range(6))
    r2 = x * x + y * y
    r4 = r2 * r2
    L = 1.0 + k1 * r2 + k2 * r4
    uvd = np.asarray(uv, np.float32).astype(np.float64)
    r = np.stack([uvd[:, 0] - (x * L * fx + cx), uvd[:, 1] - (y * L * fy + cy)], 1)
    if not jac:
        return r
    D = 2.0 * k1 + 4.0 * k2 * r2
    a00, a01, a11 = L + x * x * D, x * y * D, L + y * y * D

    def chain(J):
        return np.stack([a00[:, None] * J[:, 0] + (a01 * (fx / fy))[:, None] * J[:, 1],
                         (a01 * (fy / fx))[:, None] * J[:, 0] + a11[:, None] * J[:, 1]], 1)

    z, o = np.zeros(len(x)), np.ones(len(x))
    Jk = np.stack([np.stack([-(x * L), -o, z, z, -fx * x * r2, -fx * x * r4], 1),
                   np.stack([z, z, -(y * L), -o, -fy * y * r2, -fy * y * r4], 1)], 1)
    return r, chain(Jc), chain(Jp), Jk


class Problem:
    """calib0 [G, 4] +- tol [G], radial0 [G, 2] +- radial_tol [G]; radial=False holds k1, k2 at radial0 and out of the unknowns"""

    def __init__(self, cam_idx, pt_idx, uv, grp, cams0, pts0, calib0, tol, radial0, radial_tol, ref_cam=-1, ref_thr=1e-10, cauchy_a=0.5,
                 radial=True):
        self.cam_idx = np.asarray(cam_idx, np.int64); self.pt_idx = np.asarray(pt_idx, np.int64)
        self.uv = np.asarray(uv, np.float32)
        self.grp = np.asarray(grp, np.int64)
        self.n_cam, self.n_pt = len(cams0), len(pts0)
        calib0 = np.asarray(calib0, np.float64).reshape(-1, 4)
        self.G = len(calib0)
        self.radial0 = np.asarray(radial0, np.float64).reshape(self.G, 2)
        self.W = W = 6 if radial else 4
        block0 = np.concatenate([calib0, self.radial0], 1)[:, :W]
        self.n_obs = len(self.cam_idx)
        self.gidx = self.grp[self.cam_idx]
        self.cauchy_a = cauchy_a
        self.ko = 6 * self.n_cam + 3 * self.n_pt
        self.npar = self.ko + W * self.G
        self.x0 = np.concatenate([np.asarray(cams0, np.float64).ravel(), np.asarray(pts0, np.float64).ravel(), block0.ravel()])
        # blocks that take part in the problem (Ceres drops the others with their bounds)
        act = np.zeros(self.npar, bool)
        act[:6 * self.n_cam] = np.repeat(np.bincount(self.cam_idx, minlength=self.n_cam) > 0, 6)
        act[6 * self.n_cam:self.ko] = np.repeat(np.bincount(self.pt_idx, minlength=self.n_pt) > 0, 3)
        act[self.ko:] = np.repeat(np.bincount(self.gidx, minlength=self.G) > 0, W)
        self.active = act
        self.lo = np.full(self.npar, -np.inf); self.up = np.full(self.npar, np.inf)
        tol = np.broadcast_to(np.asarray(tol, np.float64), (self.G,))
        rtol = np.broadcast_to(np.asarray(radial_tol, np.float64), (self.G,))
        half = np.concatenate([np.repeat(tol[:, None], 4, 1), np.repeat(rtol[:, None], 2, 1)], 1)[:, :W]
        self.lo[self.ko:] = (block0 - half).ravel(); self.up[self.ko:] = (block0 + half).ravel()
        if ref_cam >= 0:
            self.lo[6 * ref_cam:6 * ref_cam + 6] = -ref_thr; self.up[6 * ref_cam:6 * ref_cam + 6] = ref_thr
        self.lo[~act] = -np.inf; self.up[~act] = np.inf
        # column index of the 6 + W camera-side unknowns of every observation in the reduced system
        self.idxc = np.concatenate([6 * self.cam_idx[:, None] + np.arange(6)[None, :],
                                    6 * self.n_cam + W * self.gidx[:, None] + np.arange(W)[None, :]], 1)
        self._tuples = None

    # ---- parameter vector ----
    def split(self, x):
        return x[:6 * self.n_cam].reshape(-1, 6), x[6 * self.n_cam:self.ko].reshape(-1, 3), x[self.ko:].reshape(-1, self.W)

    def calib6(self, x):
        blk = self.split(x)[2]
        return blk if self.W == 6 else np.concatenate([blk, self.radial0], 1)

    def plus(self, x, d):
        return np.minimum(np.maximum(x + d, self.lo), self.up)

    def cost(self, x):
        cams, pts, _ = self.split(x)
        rho0, _ = _loss(residual_jac(cams, pts, self.calib6(x), self.grp, self.cam_idx, self.pt_idx, self.uv, jac=False), self.cauchy_a)
        return 0.5 * rho0.sum()

    def evaluate(self, x):
        """cost, loss-corrected residual [n, 2] and Jacobian blocks F [n, 2, 6], E [n, 2, 3], K [n, 2, W]"""
        cams, pts, _ = self.split(x)
        r, Jc, Jp, Jk = residual_jac(cams, pts, self.calib6(x), self.grp, self.cam_idx, self.pt_idx, self.uv)
        Jk = Jk[:, :, :self.W]
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
        for j in range(self.W):
            out[self.ko + j::self.W] = np.bincount(self.gidx, weights=wk[:, j], minlength=self.G)
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
            for j in range(self.W):
                J[2 * rows + i, self.ko + self.W * self.gidx + j] = K[:, i, j]
        return J

    # ---- the LM step: (J'J + D) step = -J'r ----
    def step_dense(self, F, E, K, r, D):
        J = self.dense_jacobian(F, E, K)
        return -np.linalg.solve(J.T @ J + np.diag(D), J.T @ r.ravel())

    _track_tuples = ref.Problem._track_tuples      # (reads cam_idx, pt_idx, n_pt and the cache only)

    def step_schur(self, F, E, K, r, D):
        nc6 = 6 * self.n_cam
        W = self.W
        Wc = 6 + W
        nred = nc6 + W * self.G
        Dc = np.concatenate([D[:nc6], D[self.ko:]]); Dp = D[nc6:self.ko].reshape(-1, 3)
        Fc = np.concatenate([F, K], 2)
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
            Fu, Eu, ru = Fc[obs], E[obs], r[obs]
            cols = self.idxc[obs[0]]                                              # [T, Wc]
            Ft = Fu.transpose(1, 0, 2, 3).reshape(T, -1, Wc)                      # slot t of the tuple: [2 P, Wc]
            FtF = Ft.transpose(0, 2, 1) @ Ft
            Ftr = (Ft.transpose(0, 2, 1) @ ru.transpose(1, 0, 2).reshape(T, -1, 1))[:, :, 0]
            for t in range(T):
                np.add.at(S, (cols[t][:, None], cols[t][None, :]), FtF[t])
                np.add.at(rhs, cols[t], Ftr[t])
            U = (Fu.transpose(0, 1, 3, 2) @ Eu).reshape(len(pts_u), Wc * T, 3)    # W of every point: rows = its Wc T camera-side columns
            V = U @ Minv[pts_u]
            flat = cols.reshape(-1)
            Vf = V.transpose(1, 0, 2).reshape(Wc * T, -1); Uf = U.transpose(1, 0, 2).reshape(Wc * T, -1)
            np.subtract.at(S, (flat[:, None], flat[None, :]), Vf @ Uf.T)
            np.subtract.at(rhs, flat, Vf @ Etr[pts_u].reshape(-1))
        yc = -np.linalg.solve(S, rhs)
        f = np.einsum("nra,na->nr", Fc, yc[self.idxc])
        Wt = np.zeros((self.n_pt, 3))
        for i in range(3):
            Wt[:, i] = np.bincount(self.pt_idx, weights=(E[:, :, i] * f).sum(1), minlength=self.n_pt)
        yp = -np.einsum("pij,pj->pi", Minv, Etr + Wt)
        return np.concatenate([yc[:nc6], yp.ravel(), yc[nc6:]])


def distort_observations(uv, K4_of_obs, k_of_obs):
    """The observations of a pinhole scene as the radial model sees them: (u, v) -> normalised (x, y) -> (fx x L + cx, fy y L + cy),
    in f64, rounded to f32 like every observation.  K4_of_obs [n, 4], k_of_obs [n, 2]."""
    K = np.asarray(K4_of_obs, np.float64); k = np.asarray(k_of_obs, np.float64)
    uvd = np.asarray(uv, np.float64)
    x = (uvd[:, 0] - K[:, 1]) / K[:, 0]; y = (uvd[:, 1] - K[:, 3]) / K[:, 2]
    r2 = x * x + y * y
    L = 1.0 + k[:, 0] * r2 + k[:, 1] * r2 * r2
    return np.ascontiguousarray(np.stack([K[:, 0] * x * L + K[:, 1], K[:, 2] * y * L + K[:, 3]], 1), np.float32)
