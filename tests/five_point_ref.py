"""An OUTSIDE reference for the 5-point essential-matrix solver (numpy only; a helper, not a test module).

The product (easysfm_amd/csrc/five_point_core.hpp) and the CPU oracle (oracle/ransac_ref.c) evaluate ONE arithmetic: Householder null
space, Gauss-Jordan to the hidden-variable matrix B(z), det B(z), Durand-Kerner.  This file takes the other published route (Stewenius,
Engels, Nister: "Recent developments on direct relative orientation", 2006) and shares no step with them:
  1  null space of the 5 x 9 epipolar system from numpy's SVD (or a basis handed in);
  2  the ten cubic constraints 2 E E'E - tr(E E')E = 0, det E = 0 with E = x N0 + y N1 + z N2 + N3, expanded as polynomials in (x, y, z)
     by coefficient-tensor arithmetic (c[i, j, k] = coefficient of x^i y^j z^k) -> a 10 x 20 matrix in a degree-graded monomial order;
  3  its cubic 10 x 10 block is solved against the rest (numpy.linalg.solve): every cubic monomial as a combination of the ten
     monomials of degree <= 2 on the solution set;
  4  the 10 x 10 multiplication matrix of x on those ten monomials; its eigenvalues are the x of the ten solutions and its
     eigenvectors hold (x, y, z, 1) of each (numpy.linalg.eig).
The real solutions become unit-norm models with the largest-magnitude entry positive, as the product writes them.  Nothing is polished:
what this route returns is as good as its own conditioning, and the census measures that (residual) before it judges the product."""
import numpy as np

REAL_GATE = 1e-8          # |Im| / max(1, |Re|) of an eigenvalue up to this: a real solution (the product's gate on its roots)
GREY_GATE = 1e-4          # between the two: neither clearly real nor clearly complex -- the sample is left out of a census
DEGENERATE_SIGMA = 1e-9   # sigma5 / sigma1 of the 5 x 9 system below this, or
DEGENERATE_COND = 1e10    # condition number of the cubic block above this: a degenerate sample

# monomials as exponent triples: the ten cubic ones, then the basis of the quotient ring x2 xy xz y2 yz z2 x y z 1
CUBIC = [(3, 0, 0), (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 1, 1), (1, 0, 2), (0, 3, 0), (0, 2, 1), (0, 1, 2), (0, 0, 3)]
BASIS = [(2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
_UP_TO_2 = [m for m in BASIS]                                   # support of a polynomial of degree <= 2
_UP_TO_1 = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]         # ... of degree <= 1
# the copies of (x, y, z, 1) inside (x2 xy xz y2 yz z2 x y z 1): scaled by x, y, z and 1
_COPIES = np.array([(0, 1, 2, 6), (1, 3, 4, 7), (2, 4, 5, 8), (6, 7, 8, 9)])


def epipolar_system(q1, q2):
    """[..., 5, 9]: row i = (x2 x1, x2 y1, x2, y2 x1, y2 y1, y2, x1, y1, 1), that is x2' E x1 with E row-major"""
    q1 = np.asarray(q1, np.float64); q2 = np.asarray(q2, np.float64)
    one = np.ones(q1.shape[:-1] + (1,))
    h1 = np.concatenate([q1, one], -1); h2 = np.concatenate([q2, one], -1)
    return (h2[..., :, None] * h1[..., None, :]).reshape(q1.shape[:-1] + (9,))


def _mul(p, q, support):
    """product of coefficient tensors [n, 4, 4, 4]; q is non-zero on `support` only; total degree <= 3, so nothing is cut off"""
    r = np.zeros_like(p)
    for i, j, k in support:
        r[:, i:, j:, k:] += q[:, i, j, k, None, None, None] * p[:, :4 - i, :4 - j, :4 - k]
    return r


def constraint_matrices(N):
    """N [n, 4, 9] -> [n, 10, 20]: the ten constraints on E = x N0 + y N1 + z N2 + N3 over the monomials CUBIC + BASIS"""
    n = len(N)
    E = [[None] * 3 for _ in range(3)]
    for r in range(3):
        for c in range(3):
            p = np.zeros((n, 4, 4, 4))
            for k, m in enumerate(_UP_TO_1): p[(slice(None),) + m] = N[:, k, 3 * r + c]
            E[r][c] = p
    G = [[sum(_mul(E[r][k], E[c][k], _UP_TO_1) for k in range(3)) for c in range(3)] for r in range(3)]       # E E'
    tr = G[0][0] + G[1][1] + G[2][2]
    rows = [2.0 * sum(_mul(E[k][c], G[r][k], _UP_TO_2) for k in range(3)) - _mul(E[r][c], tr, _UP_TO_2) for r in range(3) for c in range(3)]
    minor = lambda a, b: _mul(E[1][a], E[2][b], _UP_TO_1) - _mul(E[1][b], E[2][a], _UP_TO_1)
    rows.append(_mul(E[0][0], minor(1, 2), _UP_TO_2) - _mul(E[0][1], minor(0, 2), _UP_TO_2) + _mul(E[0][2], minor(0, 1), _UP_TO_2))
    return np.stack([np.stack([p[(slice(None),) + m] for m in CUBIC + BASIS], -1) for p in rows], 1)


def canonical(E):
    """unit Frobenius norm, largest-magnitude entry positive"""
    E = np.asarray(E, np.float64).reshape(3, 3)
    E = E / np.linalg.norm(E)
    return -E if E.ravel()[np.argmax(np.abs(E))] < 0 else E


def solve_many(q1, q2, basis=None):
    """q1, q2 [n, 5, 2] (normalised coordinates) -> a list of n dicts:
         models [k, 3, 3] (ascending E[0][0]), eigenvalues [10] complex, sigma_ratio (sigma5 / sigma1 of the 5 x 9 system),
         cond (of the cubic 10 x 10 block), degenerate (one of the two measures past its bound), grey (some eigenvalue neither clearly
         real nor clearly complex).
    basis [n, 4, 9]: orthonormal null-space bases to use in place of the SVD's (sigma_ratio still comes from the SVD)."""
    q1 = np.asarray(q1, np.float64).reshape(-1, 5, 2); q2 = np.asarray(q2, np.float64).reshape(-1, 5, 2)
    n = len(q1)
    _, sv, Vt = np.linalg.svd(epipolar_system(q1, q2))
    N = Vt[:, 5:9] if basis is None else np.asarray(basis, np.float64).reshape(n, 4, 9)
    M = constraint_matrices(N)
    sigma_ratio = np.where(sv[:, 0] > 0, sv[:, 4] / np.where(sv[:, 0] > 0, sv[:, 0], 1.0), 0.0)
    finite = np.isfinite(M).all(axis=(1, 2))
    cond = np.full(n, np.inf)
    cond[finite] = np.linalg.cond(M[finite][:, :, :10])
    out = []
    for s in range(n):
        o = {"models": np.zeros((0, 3, 3)), "eigenvalues": np.full(10, np.nan, complex), "sigma_ratio": float(sigma_ratio[s]),
             "cond": float(cond[s]), "degenerate": bool(sigma_ratio[s] < DEGENERATE_SIGMA or not cond[s] <= DEGENERATE_COND), "grey": False}
        out.append(o)
        if not np.isfinite(cond[s]):
            continue
        try:
            red = -np.linalg.solve(M[s, :, :10], M[s, :, 10:])  # cubic monomial i = red[i] . BASIS on the solution set
        except np.linalg.LinAlgError:                           # (an exact zero pivot: cond above says degenerate already)
            o["degenerate"] = True
            continue
        Mx = np.zeros((10, 10))
        for r, (i, j, k) in enumerate(BASIS):                   # x * BASIS[r] in terms of BASIS
            m = (i + 1, j, k)
            if m in CUBIC: Mx[r] = red[CUBIC.index(m)]
            else: Mx[r, BASIS.index(m)] = 1.0
        if not np.isfinite(Mx).all():
            continue
        lam, vec = np.linalg.eig(Mx)
        o["eigenvalues"] = lam
        rel = np.abs(lam.imag) / np.maximum(1.0, np.abs(lam.real))
        o["grey"] = bool(np.any((rel > REAL_GATE) & (rel < GREY_GATE)))
        models = []
        for a in np.nonzero(rel <= REAL_GATE)[0]:
            v = vec[:, a]
            v = (v * np.conj(v[np.argmax(np.abs(v))])).real     # real up to a complex scale: rotate it onto the real axis
            # v = (x2 xy xz y2 yz z2 x y z 1) up to scale holds (x, y, z, 1) four times: take the largest copy (no division, and no
            # reading of x, y, z out of entries that are small against the quadratic ones)
            c = v[_COPIES[np.argmax(np.abs(v[_COPIES]).max(axis=1))]]
            e = c @ N[s]
            if np.linalg.norm(e) > 0:
                models.append(canonical(e))
        if models:
            models.sort(key=lambda e: e[0, 0])
            o["models"] = np.array(models)
    return out


def solve(q1, q2, basis=None):
    """one sample (q1, q2 [5, 2]); see solve_many"""
    return solve_many(np.asarray(q1)[None], np.asarray(q2)[None], None if basis is None else np.asarray(basis)[None])[0]


def residual(E, q1, q2):
    """r(E) = max(|x2' E x1| over the sample, |det E|, max |2 E E'E - tr(E E')E|) of the unit-norm E"""
    E = np.asarray(E, np.float64).reshape(3, 3)
    E = E / np.linalg.norm(E)
    epi = np.abs(epipolar_system(np.asarray(q1).reshape(5, 2), np.asarray(q2).reshape(5, 2)) @ E.ravel()).max()
    return max(epi, abs(np.linalg.det(E)), np.abs(2.0 * E @ E.T @ E - np.trace(E @ E.T) * E).max())


def worst_residual(models, q1, q2):
    """the largest r over a sample's models (0 when it has none)"""
    return max([residual(E, q1, q2) for E in models], default=0.0)


def model_distance(A, B):
    """the largest distance (max-abs entry) from a model of one set to the nearest of the other; inf if exactly one set is empty"""
    A = np.asarray(A, np.float64).reshape(-1, 9); B = np.asarray(B, np.float64).reshape(-1, 9)
    if len(A) == 0 and len(B) == 0:
        return 0.0
    if len(A) == 0 or len(B) == 0:
        return np.inf
    d = np.abs(A[:, None, :] - B[None, :, :]).max(axis=2)
    return max(d.min(axis=1).max(), d.min(axis=0).max())
