"""Independent numpy statement of the SIFT detector + 128-value descriptor, written from the rules of Lowe 2004 as OpenCV's
SIFT_create(nfeatures) states them with its defaults (3 layers, contrast 0.04, edge 10, sigma 1.6, first octave -1): float64
throughout, whole-array formulations, its own Gaussian taps, pyramid and math (np.exp, np.sin).  It imports neither `oracle`
nor `easysfm_amd` nor tests/sift_ref.py and uses no ctypes; the one shared approximation is cv::fastAtan2, part of the
specification, taken from surf_ref.fast_atan2_deg (as are the 14-bit gray weights).

It does not reproduce a detector's output; `verify` checks the claims in one.  The reference enumerates its own extrema, walks
every candidate through the sub-pixel rounds and sorts it into kept / rejected / undecided, where undecided means that a
float32 evaluation of the stated expressions could fall on either side of one of its decisions.  A candidate whose walk may
branch is followed along every branch (`refine`): it is rejected if every branch ends rejected, undecided otherwise.

Bounds come from the float32 unit round-off u = 2^-24, not from any implementation's output.  The pyramid is the one place
where a worst-case bound is useless: a pixel of layer 3 of octave 4 has passed through some 2000 roundings, their worst case
(every one of them u, all of one sign) is 230 u x 255 = 3.5e-3, and under it a third of the fountain picture's keypoints have
an offset not known to 0.025 px.  `blur_error` therefore uses the standard model of round-off as independent zero-mean errors
of at most u each (variance u^2 / 3; Higham, Accuracy and Stability of Numerical Algorithms, section 2.8; Higham and Mary
2019) and takes six standard deviations; errors a layer inherits are averaged by the next blur like any other noise (variance
times the squared sum of squared taps).  tests/test_sift_ref_cpu.py::test_pyramid_bound_holds checks every pixel of every layer
of every case of the float32 restatement against it.  Everything after the pyramid is worst case: `derivatives` and `refine`
carry the pixel bound through the central differences and the 3 x 3 solve (the form of surf_ref._refine), `orientation`
through the gradient of every sample into the bins it may reach.  Orientation and descriptor are recomputed from the REPORTED
x, y, size, angle and octave field, so a disagreement in one stage does not leak into the next.

What is listed as undecided is a claim, not a candidate: a reported keypoint that rests on a decision within its bound (or
whose own bound exceeds a limit below), or a keypoint of the float64 reference that is not reported and was kept without
margin.  A candidate that float64 rejects and nobody reports makes no claim.

Limits (half the smallest tamper tests/test_sift_ref_cpu.py requires `verify` to catch; a keypoint whose own derived bound
exceeds its limit is listed as undecided):
  POS_LIMIT    0.025 px in the octave's own pixels (tamper: 0.05 px)
  SIZE_LIMIT   1 % of the size (tamper: x 1.02)
  RESP_LIMIT   0.5 % of the response (tamper: x 1.01)
  ANGLE_LIMIT  5 degrees (tamper: one bin, 10 degrees)

Descriptor check.  The descriptor before its final rounding is continuous in everything float32 can perturb (the trilinear
weights vanish at every floor boundary, the 0.2 clip is a min), so one L2 distance decides: `descriptor` runs once in float64
and once with pyramid, gradients, weights and histogram sums in float32, on the sampled keypoints of every case of
feature_cases.SIFT_CASES, gray and BGR (tests/test_sift_ref_cpu.py::test_descriptor_tolerance_measured asserts all of it):
  DESC_F32_DISTANCE  largest L2 distance of the float32 run from the float64 run, in descriptor units (0..255 per element)
                     ......... 3.06e-4 measured (fountain256x320), recorded as 3.2e-4
  DESC_TOL           4 x that (covers summation orders the float32 run does not try) .. 1.28e-3
  A reported descriptor holds integers: element i may differ from the float64 value by the 0.5 of its rounding; what exceeds
  0.5 is the element's excess, and the L2 norm of the excesses (`descriptor_distance`) must stay within DESC_TOL.
  Smallest tamper distances over the same keypoints, same measure:
    one element moved by 1 away from the float64 value ... 0.5 at the least (0.5 + its rounding residue)
    orientation bins reversed inside each cell ........... 335 at the least
    cells transposed ..................................... 127 at the least (fountain256x320)
  DESC_TAMPER_MIN = 0.5;  DESC_TOL < DESC_TAMPER_MIN / 2 holds by two orders of magnitude.

Undecided share per case (gray = BGR form), CPU restatement's output, cap 0.02: fountain256x320 4 / 299 = 0.013,
blobs240x320 3 / 197 = 0.015, blobs33x40 0, border150x203 0, checker168 0, blob11 0, blob24 0.

A finding about cv::fastAtan2, part of the specification: it is not continuous across |dx| = |dy| (44.990 degrees on one side,
45.010 on the other), which straddles the edge between orientation bins 4 and 5 (and 13 | 14, 22 | 23, 31 | 32).  `orientation`
accounts for it.  A picture that equals its own transpose puts whole diagonals of samples there; feature_cases.blob11_symmetric
is one, and which of its peaks exist turns on float32 round-off alone (the verifier lists it as undecided, it does not fail it).

Stage by stage, what this statement was compared with (tests/sift_ref/sift_ref.c line, kernel of
easysfm_amd/csrc/sift_kernels.hip) and the outcome -- all through `verify` on the seven cases in gray and BGR form:
  gray, x2 base ............ sift_ref.c:204, 249-263 / sift_upsample_kernel ............ agree (known answer: 3 x 3 ramp)
  taps, blur, octaves ...... sift_ref.c:173-225, 265-280 / sift_blur_rows/cols_kernel .. agree within blur_error
  26-neighbour extremum .... sift_ref.c:529-543 / sift_extrema_kernel .................. agree; ties (>=) kept by both
  sub-pixel rounds ......... sift_ref.c:337-364 / sift_extrema_kernel .................. agree (known answer: quadratic field)
  contrast, edge ........... sift_ref.c:365-378 / sift_extrema_kernel .................. agree (known answer: tr^2/det = 12.1)
  fields, octave packing ... sift_ref.c:379-386, 582-583 / sift_extrema_kernel, sift_api.cpp:185-190 .. agree
  orientation .............. sift_ref.c:392-434 / sift_orient_kernel ................... agree (known answers: constant gradient, parabola);
                             blob11_symmetric: 1 peak there, 3 here, all four within the histogram's error radius
  descriptor ............... sift_ref.c:436-500 / sift_describe_kernel ................. agree within DESC_TOL (known answer: direct double sum)
  order, duplicates, cuts .. sift_ref.c:554-578 / sift_api.cpp:141-171 ................. agree
Not reached by any picture tried: de-duplication (two scan positions that end on the same sample give bit-equal keypoints; none
of the seven cases, white noise 296 x 390 or blobs centred on and between pixels has such a pair, so `Stages.n_duplicates` is 0
throughout and only the tamper test exercises the rule), and a tie between neighbouring DoG samples (>= against >).
Deliberate deviation kept: `nfeatures` keeps every response >= the n-th largest in scan order (OpenCV's retainBest also
keeps the ties but orders by nth_element); stated the same way here, in sift_ref.c and in sift_api.cpp.
"""
import math

import numpy as np
from scipy.ndimage import correlate1d

from surf_ref import bgr2gray, fast_atan2_deg, sample_indices

N_LAYERS, SIGMA, CONTRAST, EDGE, BORDER, MAX_ROUNDS, ORI_BINS = 3, 1.6, 0.04, 10.0, 5, 5, 36
U = 2.0 ** -24
POS_LIMIT, SIZE_LIMIT, RESP_LIMIT, ANGLE_LIMIT = 0.025, 0.01, 0.005, 5.0
DESC_F32_DISTANCE = 3.2e-4
DESC_TOL = 4 * DESC_F32_DISTANCE
DESC_TAMPER_MIN = 0.5
EPS32 = 2.0 ** -23


def as_gray(image):
    image = np.asarray(image)
    return bgr2gray(image) if image.ndim == 3 else image.astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------ pyramid
def _linear_x2(a, axis):
    """INTER_LINEAR x2 along one axis: output sample k reads the source at (k + 0.5) / 2 - 0.5, edge pixels replicated."""
    n = a.shape[axis]
    src = (np.arange(2 * n) + 0.5) / 2 - 0.5
    i0 = np.floor(src).astype(np.int64)
    f = src - i0
    lo, hi = np.take(a, np.clip(i0, 0, n - 1), axis=axis), np.take(a, np.clip(i0 + 1, 0, n - 1), axis=axis)
    shape = [1, 1]; shape[axis] = 2 * n
    f = f.reshape(shape)
    return lo * (1 - f) + hi * f


def upsample2(gray):
    return _linear_x2(_linear_x2(np.asarray(gray, np.float64), 1), 0)


def gaussian_taps(sigma):
    n = int(round(8 * sigma + 1)) | 1
    x = np.arange(n) - (n - 1) / 2
    w = np.exp(-x * x / (2 * sigma * sigma))
    return w / w.sum()


def layer_sigmas():
    """sigma of the blur that makes layer i from layer i - 1 (entry 0: the base image, which carries 0.5 px x 2 already)."""
    k = 2.0 ** (1.0 / N_LAYERS)
    return [math.sqrt(SIGMA ** 2 - 1.0)] + [SIGMA * math.sqrt(k ** (2 * i) - k ** (2 * i - 2)) for i in range(1, N_LAYERS + 3)]


def n_octaves(rows, cols):
    return int(round(math.log2(min(2 * rows, 2 * cols)) - 2)) + 1


def blur(img, sigma):
    """Separable Gaussian, BORDER_REFLECT_101 (scipy's 'mirror', which reflects again when the kernel is wider than the image)."""
    w = gaussian_taps(sigma).astype(img.dtype)
    return correlate1d(correlate1d(img, w, axis=1, mode="mirror"), w, axis=0, mode="mirror")


def blur_error(n_taps, top):
    """Float32 round-off one blur adds to a pixel, for data of magnitude <= top, at six standard deviations of the model in the
    header.  Row pass: n products and a running sum of n partial sums, none above the result; column pass: the pairs are
    added, multiplied and summed outward from the centre, r + 1 partial sums, r = n / 2; the taps are rounded to float once.  That
    is n + 5 roundings of at most u top each when counted by magnitude (the partial sums of symmetric taps that sum to 1 add up to
    (n + 1) / 2 of the result), each of variance (u top)^2 / 3: 6 u top sqrt((n + 5) / 3)."""
    return U * top * (6 / math.sqrt(3)) * math.sqrt(n_taps + 5)


def build_pyramid(gray, dtype=np.float64):
    """([octave] -> [6, rows, cols] Gaussian layers, [octave] -> [5, rows, cols] DoG layers, [octave][6] error bound of a
    Gaussian pixel, [octave][5] error bound of a DoG pixel before its own |value| u).  A layer's error is its own blur's round-off
    and what it inherits: the inherited error e is averaged, variance x att = (sum of squared taps)^2; the DoG sees blur(e) - e,
    whose variance is at most (1 + att) var e."""
    sig = layer_sigmas()
    taps = [len(gaussian_taps(s)) for s in sig]
    att = [float(np.sum(gaussian_taps(s) ** 2)) ** 2 for s in sig]
    base = upsample2(gray).astype(dtype)                        # multiples of 1/16 below 256: exact in float32
    G, D, EG, ED = [], [], [], []
    for o in range(n_octaves(*np.shape(gray))):
        if o == 0:
            first, e = blur(base, sig[0]), blur_error(taps[0], float(base.max()))
        else:
            first, e = G[o - 1][N_LAYERS][0::2, 0::2][:G[o - 1].shape[1] // 2, :G[o - 1].shape[2] // 2], EG[o - 1][N_LAYERS]
        layers, eg, ed = [first], [e], []
        for i in range(1, N_LAYERS + 3):
            layers.append(blur(layers[-1], sig[i]))
            rho = blur_error(taps[i], float(np.abs(layers[-2]).max()))
            ed.append(math.sqrt((1 + att[i]) * eg[-1] ** 2 + rho ** 2))
            eg.append(math.sqrt(att[i] * eg[-1] ** 2 + rho ** 2))
        g = np.stack(layers)
        G.append(g); D.append(g[1:] - g[:-1]); EG.append(eg); ED.append(ed)
    return G, D, EG, ED


# --------------------------------------------------------------------------------------------------------------- candidates
def _neighbours():
    return [(dl, dy, dx) for dl in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dl, dy, dx) != (0, 0, 0)]


def extrema(D, layer, err=None):
    """Candidates of DoG layer `layer` (1..3) of one octave, border 5: |v| > 1 and v >= all 26 neighbours (v > 0) or <= (v < 0).
    Returns (rows, cols, margin, exact) in scan order.  Without `err` these are the candidates.  With `err` ([5] bounds of a DoG
    value) they are the loose set -- every sample a float32 evaluation could take for a candidate: `exact` says whether the float64
    comparisons all hold, and margin <= 0 marks the samples at which one of the 27 comparisons lies within the pair's bounds."""
    _, rows, cols = D.shape
    if rows <= 2 * BORDER or cols <= 2 * BORDER:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0), np.zeros(0, bool)
    v = D[layer][BORDER:rows - BORDER, BORDER:cols - BORDER]
    e = [0.0] * 5 if err is None else [x + 4 * U * float(np.abs(D).max()) for x in err]
    sgn = np.sign(v)
    margin = np.abs(v) - 1.0 - e[layer]
    exact = np.abs(v) > 1.0
    loose = np.abs(v) + e[layer] > 1.0
    for dl, dy, dx in _neighbours():
        gap = sgn * (v - D[layer + dl][BORDER + dy:rows - BORDER + dy, BORDER + dx:cols - BORDER + dx])
        pair = e[layer] + e[layer + dl]
        exact &= gap >= 0
        loose &= gap + pair >= 0
        margin = np.minimum(margin, gap - pair)
    r, c = np.nonzero(loose if err is not None else exact)
    return r + BORDER, c + BORDER, margin[r, c], exact[r, c]


def derivatives(D, layer, r, c, err=None):
    """Gradient (x, y, s) and Hessian of the DoG at a sample by central differences, in image units (values / 255): first
    differences x 0.5, second x 1, cross x 0.25.  With `err`, also the bounds of both (a DoG value carries err[layer] + 3 u |value|
    through a difference, as in surf_ref._refine)."""
    s = 1.0 / 255
    N = D[layer - 1:layer + 2, r - 1:r + 2, c - 1:c + 2]
    v = N[1, 1, 1]
    g = 0.5 * s * np.array([N[1, 1, 2] - N[1, 1, 0], N[1, 2, 1] - N[1, 0, 1], N[2, 1, 1] - N[0, 1, 1]])
    cross = lambda p, q, rr, t: 0.25 * s * (p - q - rr + t)
    dxy = cross(N[1, 2, 2], N[1, 2, 0], N[1, 0, 2], N[1, 0, 0])
    dxs = cross(N[2, 1, 2], N[2, 1, 0], N[0, 1, 2], N[0, 1, 0])
    dys = cross(N[2, 2, 1], N[2, 0, 1], N[0, 2, 1], N[0, 0, 1])
    H = np.array([[s * (N[1, 1, 2] + N[1, 1, 0] - 2 * v), dxy, dxs], [dxy, s * (N[1, 2, 1] + N[1, 0, 1] - 2 * v), dys], [dxs, dys, s * (N[2, 1, 1] + N[0, 1, 1] - 2 * v)]])
    if err is None:
        return g, H, None, None, 0.0
    M = np.abs(N) * 3 * U + np.array(err[layer - 1:layer + 2])[:, None, None]
    dg = 0.5 * s * np.array([M[1, 1, 2] + M[1, 1, 0], M[1, 2, 1] + M[1, 0, 1], M[2, 1, 1] + M[0, 1, 1]])
    cm = lambda p, q, rr, t: 0.25 * s * (p + q + rr + t)
    mxy, mxs, mys = cm(M[1, 2, 2], M[1, 2, 0], M[1, 0, 2], M[1, 0, 0]), cm(M[2, 1, 2], M[2, 1, 0], M[0, 1, 2], M[0, 1, 0]), cm(M[2, 2, 1], M[2, 0, 1], M[0, 2, 1], M[0, 0, 1])
    mc = M[1, 1, 1]
    dH = np.array([[s * (M[1, 1, 2] + M[1, 1, 0] + 2 * mc), mxy, mxs], [mxy, s * (M[1, 2, 1] + M[1, 0, 1] + 2 * mc), mys], [mxs, mys, s * (M[2, 1, 1] + M[0, 1, 1] + 2 * mc)]])
    return g, H, dg, dH, mc * s


def edge_ok(dxx, dyy, dxy):
    """Kept iff det > 0 and 10 tr^2 < 121 det, i.e. tr^2 / det < (EDGE + 1)^2 / EDGE."""
    tr, det = dxx + dyy, dxx * dyy - dxy * dxy
    return bool(det > 0 and EDGE * tr * tr < (EDGE + 1) ** 2 * det)


class Refined:
    """Outcome of `refine`.  status: 'kept', 'rejected' (reason in `why`), or 'undecided' (`why` lists the decisions a float32
    evaluation may take the other way; `kept64` is the float64 outcome).  offset = (xc, xr, xi) about (layer, r, c).
    `others`: where the walks end that a float32 evaluation may take instead, those that end rejected left out."""
    __slots__ = ("status", "why", "kept64", "layer", "r", "c", "offset", "ex", "contrast", "e_contrast", "rounds", "others")


def _offset(D, layer, r, c, err):
    """(offset, its bound) of one round, or (None, None) where the Hessian is singular."""
    g, H, dg, dH, _ = derivatives(D, layer, r, c, err)
    if abs(np.linalg.det(H)) < 1e-300 or np.linalg.cond(H) > 1e7:
        return None, None
    x = -np.linalg.solve(H, g)
    if err is None:
        return x, np.zeros(3)
    Hi = np.abs(np.linalg.inv(H))
    return x, Hi @ (dg + dH @ np.abs(x)) + 16 * U * (Hi @ (np.abs(H) @ np.abs(x)))


def _leaf(layer, r, c, x, ex, rounds, status, why, contrast=0.0, e_contrast=0.0, kept64=False):
    out = Refined()
    out.layer, out.r, out.c, out.offset, out.ex, out.rounds, out.status, out.why = layer, r, c, x, ex, rounds, status, list(why)
    out.contrast, out.e_contrast, out.kept64, out.others = contrast, e_contrast, kept64, []
    return out


def _accept(D, layer, r, c, x, ex, rounds, err):
    """The contrast and edge tests at a converged position."""
    g, H, dg, dH, e_v = derivatives(D, layer, r, c, err)
    contr = D[layer, r, c] / 255 + 0.5 * float(g @ x)
    e_contr = 0.0 if err is None else e_v + 0.5 * float(dg @ np.abs(x) + np.abs(g) @ ex) + 4 * U * abs(contr)
    gate = []
    if err is not None and abs(abs(contr) * N_LAYERS - CONTRAST) <= N_LAYERS * e_contr + 2 * U * CONTRAST:
        gate.append("contrast threshold")
    keep = abs(contr) * N_LAYERS >= CONTRAST
    if not keep and not gate:
        return _leaf(layer, r, c, x, ex, rounds, "rejected", ["contrast"], contr, e_contr)
    dxx, dyy, dxy = H[0, 0], H[1, 1], H[0, 1]
    tr, det = dxx + dyy, dxx * dyy - dxy * dxy
    f = (EDGE + 1) ** 2 * det - EDGE * tr * tr
    close = False
    if err is not None:
        e_det = abs(dyy) * dH[0, 0] + abs(dxx) * dH[1, 1] + 2 * abs(dxy) * dH[0, 1] + 3 * U * (abs(dxx * dyy) + dxy * dxy)
        e_f = (EDGE + 1) ** 2 * e_det + 2 * EDGE * abs(tr) * (dH[0, 0] + dH[1, 1] + U * abs(tr)) + 4 * U * ((EDGE + 1) ** 2 * abs(det) + EDGE * tr * tr)
        close = abs(det) <= e_det or abs(f) <= e_f
    if not edge_ok(dxx, dyy, dxy):
        if not close:
            return _leaf(layer, r, c, x, ex, rounds, "rejected", ["edge"], contr, e_contr)
        keep = False
    if close:
        gate.append("edge threshold")
    return _leaf(layer, r, c, x, ex, rounds, "undecided" if gate else "kept", gate, contr, e_contr, keep)


def _walk(D, layer, r, c, it, err, leaves, nominal):
    """Every way a float32 evaluation may take from round `it` on: where an |offset| lies within its bound of 0.5, or a move
    within its bound of a rounding tie, both ways are walked.  Leaves are (follows the float64 decisions, Refined)."""
    _, rows, cols = D.shape
    if len(leaves) > 64:
        return
    if it >= MAX_ROUNDS:
        leaves.append((nominal, _leaf(layer, r, c, np.zeros(3), np.zeros(3), it, "rejected", ["no round converged"]))); return
    x, ex = _offset(D, layer, r, c, err)
    if x is None or not np.all(ex < 1.0):
        # the float32 elimination gives up on a pivot below 10 eps and calls the offset zero; an offset known to less than a
        # pixel decides nothing: neither is a walk float64 can follow
        leaves.append((nominal, _leaf(layer, r, c, np.zeros(3) if x is None else x, np.full(3, np.inf), it + 1, "undecided", ["offset not determined"]))); return
    may_converge, may_move = np.all(np.abs(x) - ex < 0.5), np.any(np.abs(x) + ex >= 0.5)
    converges = bool(np.all(np.abs(x) < 0.5))
    if may_converge:
        # whatever the offset, a converged one has |x_i| < 0.5: |contrast| <= |v| / 255 + sum |g_i| / 4
        g, _, dg, _, e_v = derivatives(D, layer, r, c, err)
        if err is not None and (abs(D[layer, r, c]) / 255 + e_v + 0.25 * float(np.sum(np.abs(g) + dg))) * N_LAYERS < CONTRAST * (1 - 4 * U):
            leaves.append((nominal and converges, _leaf(layer, r, c, x, ex, it + 1, "rejected", ["contrast"])))
        else:
            leaves.append((nominal and converges, _accept(D, layer, r, c, x, ex, it + 1, err)))
    if not may_move:
        return
    if np.any(np.abs(x) > 2.0 ** 31 / 3):
        leaves.append((nominal, _leaf(layer, r, c, x, ex, it + 1, "rejected", ["offset beyond the integers"]))); return
    steps = [range(int(np.rint(x[t] - ex[t])), int(np.rint(x[t] + ex[t])) + 1) for t in range(3)]
    for sc in steps[0]:
        for sr in steps[1]:
            for sl in steps[2]:
                if (sc, sr, sl) == (0, 0, 0) and may_converge:
                    continue                                    # that is the converged walk
                same = nominal and not converges and (sc, sr, sl) == tuple(int(v) for v in np.rint(x))
                c2, r2, l2 = c + sc, r + sr, layer + sl
                if l2 < 1 or l2 > N_LAYERS or c2 < BORDER or c2 >= cols - BORDER or r2 < BORDER or r2 >= rows - BORDER:
                    leaves.append((same, _leaf(layer, r, c, x, ex, it + 1, "rejected", ["left the layers or the border"])))
                else:
                    _walk(D, l2, r2, c2, it + 1, err, leaves, same)


def refine(D, layer, r, c, err=None):
    """Up to 5 rounds about a candidate of one octave's DoG stack D [5, rows, cols] (pixel units): offset = -H^-1 g; done when
    all three |offsets| < 0.5, else move by the rounded offset; rejected when it leaves layers 1..3 or the border of 5 or when no
    round converged; then contrast D / 255 + g . offset / 2 (rejected if |contrast| * 3 < 0.04) and the edge test.
    Offset bound: |dx| <= |H^-1| (dg + dH |x|) + 16 u |H^-1| |H| |x| (inputs, then a float32 3 x 3 elimination).
    A candidate all of whose possible walks end rejected is rejected; one with several walks of which any survives is undecided."""
    leaves = []
    _walk(D, layer, r, c, 0, err, leaves, True)
    main = next((leaf for nom, leaf in leaves if nom), leaves[0][1])
    rest = [leaf for nom, leaf in leaves if leaf is not main]
    if len(leaves) > 64:
        main.status, main.why = "undecided", main.why + ["too many possible walks"]
    elif rest and not all(leaf.status == "rejected" for leaf in [main] + rest):
        main.status, main.why = "undecided", main.why + ["a decision of the walk within its bound"]
        main.others = [leaf for leaf in rest if leaf.status != "rejected"]
        for leaf in main.others:
            leaf.status, leaf.kept64, leaf.why = "undecided", False, leaf.why + ["reached only if float32 walks another way"]
    return main


def keypoint_fields(o, layer, offset, r, c, contrast):
    """(x, y, size, response, packed octave) as reported: position and size in the x2 base's pixels, then the first-octave
    adjustment (x, y, size halved, the octave byte one lower)."""
    xc, xr, xi = offset
    x, y = (c + xc) * 2.0 ** o, (r + xr) * 2.0 ** o
    size = SIGMA * 2.0 ** ((layer + xi) / N_LAYERS) * 2.0 ** o * 2
    packed = o + (layer << 8) + (int(np.rint((xi + 0.5) * 255)) << 16)
    packed = (packed & ~255) | ((packed - 1) & 255)
    return x / 2, y / 2, size / 2, abs(contrast), packed


def unpack_octave(field):
    """(pyramid octave index, layer, quantised xi) of a reported octave field."""
    v = int(field)
    o = v & 255
    return (o if o < 128 else o - 256) + 1, (v >> 8) & 255, (v >> 16) & 255


# -------------------------------------------------------------------------------------------------------------- orientation
class Peak:
    __slots__ = ("bin", "angle", "bound", "decided", "exists64")


class Orientation:
    __slots__ = ("raw", "hist", "radius", "n_samples", "n_skipped", "peaks", "rad")


def smooth(raw):
    """Circular [1 4 6 4 1] / 16."""
    return (np.roll(raw, 2) + np.roll(raw, -2)) / 16 + (np.roll(raw, 1) + np.roll(raw, -1)) * 4 / 16 + raw * 6 / 16


def peaks_of(hist, rad=None):
    """Bins strictly above both neighbours and >= 0.8 max, refined by a parabola; angle = 360 - 10 bin, 360 folded to 0.  `rad`:
    error radius of every bin; a peak whose three comparisons do not all clear the radii is listed with decided = False, one that
    fails a comparison by less than the radii is listed with exists64 = False."""
    n = len(hist)
    rad = np.zeros(n) if rad is None else rad
    top, e_top = hist.max(), rad.max()
    out = []
    for j in range(n):
        l, r = (j - 1) % n, (j + 1) % n
        m = min(hist[j] - hist[l] - rad[j] - rad[l], hist[j] - hist[r] - rad[j] - rad[r], hist[j] - 0.8 * top - rad[j] - 0.8 * e_top - 2 * U * top)
        exists = hist[j] > hist[l] and hist[j] > hist[r] and hist[j] >= 0.8 * top
        loose = min(hist[j] - hist[l] + rad[j] + rad[l], hist[j] - hist[r] + rad[j] + rad[r], hist[j] - 0.8 * top + rad[j] + 0.8 * e_top + 2 * U * top) >= 0
        if not (exists or (loose and rad.any())):
            continue
        p = Peak()
        p.bin, p.exists64, p.decided = j, bool(exists), bool(exists and m > 0)
        num, den = hist[l] - hist[r], hist[l] - 2 * hist[j] + hist[r]
        if den == 0:
            p.angle, p.bound, p.decided = (360.0 - 10.0 * j) % 360.0, 360.0, False
            out.append(p); continue
        b = j + 0.5 * num / den
        b = b + n if b < 0 else b - n if b >= n else b
        a = 360.0 - (360.0 / n) * b
        p.angle = 0.0 if abs(a - 360.0) < EPS32 else a
        e_num, e_den = rad[l] + rad[r], rad[l] + 2 * rad[j] + rad[r]
        p.bound = (360.0 / n) * 0.5 * (e_num / abs(den) + abs(num) * e_den / (den * den)) * (1 + 1e-3) + 16 * U * 360.0
        if abs(den) <= e_den:
            p.bound = 360.0
        if p.bound > ANGLE_LIMIT:
            p.decided = False
        out.append(p)
    return out


def orientation(img, r, c, scl, e_pix=None):
    """Histogram and peaks at sample (r, c) of the keypoint's Gaussian layer, scl the scale in the octave's pixels: radius
    round(4.5 scl), weights exp(-(i^2 + j^2) / (2 (1.5 scl)^2)), dx = I(y, x + 1) - I(y, x - 1), dy = I(y - 1, x) - I(y + 1, x),
    samples strictly inside the image, weight x magnitude into bin round(fastAtan2(dy, dx) / 10) mod 36.

    With e_pix (bound of a pixel of the layer) every bin gets an error radius: a gradient component errs by 2 e_pix + u |d|, the
    angle of a sample by that over its magnitude (plus 2e-4 degrees for the float32 polynomial); a sample within that of a bin
    edge may land in the neighbouring bin, so its whole mass goes into the radius of both; one whose angle is not known to 5
    degrees into the radius of every bin.  Sure samples contribute the error of their mass, and a bin its float32 summation."""
    rows, cols = img.shape
    out = Orientation()
    radius = int(np.rint(4.5 * scl))
    sg = 1.5 * scl
    i, j = np.mgrid[-radius:radius + 1, -radius:radius + 1]
    y, x = r + i, c + j
    ok = (y > 0) & (y < rows - 1) & (x > 0) & (x < cols - 1)
    out.radius, out.n_samples, out.n_skipped = radius, int(ok.sum()), int((~ok).sum())
    y, x, i, j = y[ok], x[ok], i[ok], j[ok]
    dx, dy = img[y, x + 1] - img[y, x - 1], img[y - 1, x] - img[y + 1, x]
    w = np.exp(-(i * i + j * j) / (2 * sg * sg))
    mag = np.hypot(dx, dy)
    t = fast_atan2_deg(dy, dx) / (360.0 / ORI_BINS)
    b = np.rint(t).astype(np.int64) % ORI_BINS
    mass = w * mag
    out.raw = np.bincount(b, mass, ORI_BINS)
    out.hist = smooth(out.raw)
    out.rad = np.zeros(ORI_BINS)
    if e_pix is not None:
        e_d = 2 * e_pix + U * np.maximum(np.abs(dx), np.abs(dy))
        e_ang = np.where(mag > 2 * e_d, np.degrees(2 * e_d / np.where(mag > 2 * e_d, mag, 1.0)) * 1.05, 360.0) + 2e-4
        # fastAtan2 is not continuous across |dx| = |dy|: one side ends at p(1) = 44.990 degrees, the other starts at 90 - p(1)
        e_ang = e_ang + np.where(np.abs(np.abs(dx) - np.abs(dy)) <= 2 * e_d, 0.0206, 0.0)
        e_mass = w * 2 * e_d + 6 * U * mass
        lost = e_ang > 5.0
        edge = ~lost & (np.abs(np.abs(t - np.floor(t)) - 0.5) <= e_ang / 10.0)
        up = np.rint(t) <= t                                  # the other bin is the next one up
        sure = np.bincount(b, e_mass, ORI_BINS) + (np.bincount(b, None, ORI_BINS) + 2) * U * out.raw
        out.rad = smooth(sure) + 6 * U * out.hist + float((mass + e_mass)[lost].sum())
        # a sample that changes bins moves its mass under the smoothing kernel by one place: bin j of the smoothed histogram
        # changes by mass |k(j - b') - k(j - b)|
        kernel = np.zeros(ORI_BINS); kernel[[0, 1, 2, -1, -2]] = [6 / 16, 4 / 16, 1 / 16, 4 / 16, 1 / 16]
        shift = np.abs(np.roll(kernel, 1) - kernel)           # from bin 0 to bin 1
        moved_up = np.bincount(b[edge & up], (mass + e_mass)[edge & up], ORI_BINS)
        moved_dn = np.bincount(b[edge & ~up], (mass + e_mass)[edge & ~up], ORI_BINS)
        for q in np.nonzero(moved_up)[0]:
            out.rad += moved_up[q] * np.roll(shift, q)
        for q in np.nonzero(moved_dn)[0]:
            out.rad += moved_dn[q] * np.roll(shift, q - 1)
    out.peaks = peaks_of(out.hist, out.rad if e_pix is not None else None)
    return out


# --------------------------------------------------------------------------------------------------------------- descriptor
def descriptor_geometry(shape, scl):
    """(sampling radius, whether the octave's diagonal clipped it)."""
    radius = int(np.rint(3 * scl * math.sqrt(2) * 2.5))
    diag = int(math.sqrt(shape[0] ** 2 + shape[1] ** 2))
    return min(radius, diag), radius > diag


def descriptor_histogram(img, xo, yo, scl, angle, dtype=np.float64):
    """The 4 x 4 x 8 histogram before normalisation at octave position (xo, yo), octave scale scl, keypoint angle `angle`:
    ori = 360 - angle, hist_width = 3 scl, window radius round(hist_width sqrt2 2.5) clipped to the octave's diagonal, offsets
    (j, i) about the rounded position rotated by ori and divided by hist_width, bins rbin = r_rot + 1.5, cbin = c_rot + 1.5; a
    sample counts iff -1 < rbin, cbin < 4 and its pixel lies strictly inside the image; weight exp(-(c_rot^2 + r_rot^2) / 8);
    obin = (Ori - ori) 8 / 360; trilinear spread over 6 x 6 x 10 bins with orientation bins 8, 9 folded onto 0, 1 (stated here as
    orientation indices modulo 8, which is the same sum)."""
    f = dtype
    img = np.asarray(img, f)
    rows, cols = img.shape
    ori = 360.0 - float(angle)
    if abs(ori - 360.0) < EPS32:
        ori = 0.0
    px, py = int(np.rint(xo)), int(np.rint(yo))
    hw = f(3.0) * f(scl)
    radius, _ = descriptor_geometry(img.shape, scl)
    ct, st = f(math.cos(math.radians(ori))) / hw, f(math.sin(math.radians(ori))) / hw
    i, j = np.mgrid[-radius:radius + 1, -radius:radius + 1]
    fi, fj = i.astype(f), j.astype(f)
    c_rot, r_rot = fj * ct - fi * st, fj * st + fi * ct
    rbin, cbin = r_rot + f(1.5), c_rot + f(1.5)
    r, c = py + i, px + j
    ok = (rbin > -1) & (rbin < 4) & (cbin > -1) & (cbin < 4) & (r > 0) & (r < rows - 1) & (c > 0) & (c < cols - 1)
    r, c, rbin, cbin, c_rot, r_rot = r[ok], c[ok], rbin[ok], cbin[ok], c_rot[ok], r_rot[ok]
    dx, dy = img[r, c + 1] - img[r, c - 1], img[r - 1, c] - img[r + 1, c]
    W = np.exp(-(c_rot * c_rot + r_rot * r_rot) / f(8)).astype(f)
    Ori = fast_atan2_deg(dy, dx).astype(f)
    obin = ((Ori - f(ori)) * f(8.0 / 360.0)).astype(f)
    mag = (np.sqrt(dx * dx + dy * dy) * W).astype(f)
    r0, c0, o0 = np.floor(rbin), np.floor(cbin), np.floor(obin)
    fr, fc, fo = (rbin - r0).astype(f), (cbin - c0).astype(f), (obin - o0).astype(f)
    r0, c0, o0 = r0.astype(np.int64) + 1, c0.astype(np.int64) + 1, o0.astype(np.int64)
    hist = np.zeros((6, 6, 8), f)
    for a, wr in ((0, f(1) - fr), (1, fr)):
        for b, wc in ((0, f(1) - fc), (1, fc)):
            for q, wo in ((0, f(1) - fo), (1, fo)):
                np.add.at(hist, (r0 + a, c0 + b, (o0 + q) % 8), (mag * wr * wc * wo).astype(f))
    return hist[1:5, 1:5, :]


def descriptor_finish(hist):
    """128 values before the final rounding: clipped at 0.2 of the norm, rescaled to 512 / norm of the clipped, saturated at 255."""
    v = np.asarray(hist, np.float64).reshape(128)
    v = np.minimum(v, 0.2 * np.sqrt(np.sum(v * v)))
    return np.clip(v * (512.0 / max(np.sqrt(np.sum(v * v)), EPS32)), 0.0, 255.0)


def descriptor(img, xo, yo, scl, angle, dtype=np.float64):
    return descriptor_finish(descriptor_histogram(img, xo, yo, scl, angle, dtype))


def descriptor_distance(pre, reported):
    """L2 norm of what each reported (integer) element differs from the unrounded value by beyond the 0.5 of its rounding."""
    return float(np.linalg.norm(np.maximum(np.abs(np.asarray(reported, np.float64) - pre) - 0.5, 0.0)))


# ------------------------------------------------------------------------------------------------------------------- stages
class Final:
    """One refined position of an octave, with every scan position that led to it."""
    __slots__ = ("o", "ref", "starts", "x", "y", "size", "response", "packed", "scl", "ori", "why")

    @property
    def layer(self): return self.ref.layer


class Stages:
    """Gray image, pyramid with its error bounds, every candidate walked through `refine`, grouped by where it ended."""

    def __init__(self, image, dtype=np.float64):
        self.gray = as_gray(image)
        self.G, self.D, self.EG, self.ED = build_pyramid(self.gray, dtype)
        self.finals = {}                                      # (o, layer, r, c) -> Final
        self.n_candidates = self.n_starts_kept = 0
        if dtype != np.float64:
            return
        for o, D in enumerate(self.D):
            for i in range(1, N_LAYERS + 1):
                rr, cc, margin, exact = extrema(D, i, self.ED[o])
                for r, c, m, ex64 in zip(rr.tolist(), cc.tolist(), margin.tolist(), exact.tolist()):
                    self.n_candidates += 1
                    main = refine(D, i, r, c, self.ED[o])
                    for ref in [main] + main.others:
                        if ref.status == "rejected":
                            continue
                        sure = m > 0 and ref.status == "kept"
                        if m <= 0:
                            ref.status = "undecided"
                            ref.why = ["extremum or |v| > 1 within the bound"] + ref.why
                            ref.kept64 = ref.kept64 and ex64
                        key = (o, ref.layer, ref.r, ref.c)
                        fin = self.finals.get(key)
                        if fin is None:
                            fin = self.finals[key] = Final()
                            fin.o, fin.ref, fin.starts, fin.ori, fin.why = o, ref, [], None, []
                        fin.starts.append(((o, i, r, c), sure, ref))
        for fin in self.finals.values():
            self._fields(fin)

    def _fields(self, fin):
        # the final is as sure as its surest start; its scan key is that of its first start
        best = next((s for s in fin.starts if s[1]), None) or next((s for s in fin.starts if s[2].kept64), None)
        fin.ref = best[2] if best else fin.starts[0][2]
        if not (best and best[1]):
            fin.why = list(fin.ref.why)
        elif not fin.starts[0][1]:
            fin.why = ["an earlier scan position may or may not lead here"]
        ref = fin.ref
        fin.x, fin.y, fin.size, fin.response, fin.packed = keypoint_fields(fin.o, ref.layer, ref.offset, ref.r, ref.c, ref.contrast)
        fin.scl = fin.size / 2.0 ** fin.o
        if not np.all(np.isfinite(ref.ex)) or ref.ex[0] > POS_LIMIT or ref.ex[1] > POS_LIMIT:
            fin.why.append("position bound above the limit")
        if math.log(2) / N_LAYERS * ref.ex[2] > SIZE_LIMIT:
            fin.why.append("size bound above the limit")
        if ref.e_contrast > RESP_LIMIT * abs(ref.contrast):
            fin.why.append("response bound above the limit")

    def kept64(self, fin):
        return any(s[2].kept64 for s in fin.starts)

    def orientation_of(self, fin):
        if fin.ori is None:
            fin.ori = orientation(self.G[fin.o][fin.ref.layer], fin.ref.r, fin.ref.c, fin.scl, self.EG[fin.o][fin.ref.layer])
        return fin.ori

    def n_duplicates(self):
        """Scan positions kept by the float64 decisions beyond the first of their final position: what de-duplication removes."""
        return sum(max(sum(1 for s in f.starts if s[2].kept64) - 1, 0) for f in self.finals.values())

    def reference(self):
        """The float64 reference's own keypoint list in scan order: [(scan key + (bin,), Final, Peak)]."""
        out = []
        for fin in self.finals.values():
            if not self.kept64(fin):
                continue
            first = min(s[0] for s in fin.starts if s[2].kept64)
            out += [(first + (p.bin,), fin, p) for p in self.orientation_of(fin).peaks if p.exists64]
        return sorted(out, key=lambda t: t[0])


# ------------------------------------------------------------------------------------------------------------------- verify
class Report:
    def __init__(self):
        self.errors, self.undecided = [], []
        self.n_reference = self.n_reported = self.n_described = self.n_clipped_radius = self.n_partial_disc = self.n_duplicates = 0
        self.max_desc_distance = 0.0

    @property
    def ok(self):
        return not self.errors

    def undecided_share(self):
        return len(self.undecided) / max(self.n_reference, 1)

    def __repr__(self):
        return (f"<sift report: {self.n_reported} reported, {self.n_reference} reference, {len(self.undecided)} undecided, {self.n_duplicates} duplicates removed, "
                f"{self.n_described} described (max distance {self.max_desc_distance:.3g}), {self.n_clipped_radius} with a clipped radius, "
                f"{self.n_partial_disc} with a partial disc, {len(self.errors)} errors: {self.errors[:4]}>")


def octave_position(kp_row):
    """(pyramid octave, layer, xo, yo, scl) of a reported keypoint: its position and scale in its octave's own pixels."""
    o, layer, _ = unpack_octave(kp_row[5])
    return o, layer, float(kp_row[0]) * 2 / 2.0 ** o, float(kp_row[1]) * 2 / 2.0 ** o, float(kp_row[2]) / 2.0 ** o


def verify(image, params, keypoints, descriptors, stages=None):
    """params: {'nfeatures': n (0 = all), optional 'max_keypoints': m, 'describe': indices or None for the seeded sample,
    'desc_tol'}.  keypoints [n, 7] float32 (x, y, size, angle, response, octave, class_id), descriptors [n, 128] float32."""
    st = stages or Stages(image)
    rep = Report()
    err = rep.errors.append
    kp = np.asarray(keypoints, np.float64).reshape(-1, 7)
    desc = np.asarray(descriptors, np.float64).reshape(-1, 128)
    rep.n_reported = len(kp)
    if len(kp) != len(desc):
        err("keypoint and descriptor counts differ")
        return rep
    nfeatures, max_kp = int(params.get("nfeatures", 0)), params.get("max_keypoints")
    reference = st.reference()
    rep.n_reference, rep.n_duplicates = len(reference), st.n_duplicates()
    n_listed = set()

    def undecided(kind, who, why):
        """One entry per claim: a reported keypoint (by index) or a keypoint of the reference (by scan key)."""
        if who not in n_listed:
            n_listed.add(who); rep.undecided.append((kind, who, why))
    by_octave = {}
    for fin in st.finals.values():
        by_octave.setdefault(fin.o, []).append(fin)
    # ---- every reported keypoint sits on a candidate, and its fields follow from the float64 DoG
    taken, keys = {}, []
    for k, row in enumerate(kp):
        x, y, size, angle, resp, octave, cid = row
        keys.append(None)
        if octave != int(octave) or cid != -1 or not (0 <= angle < 360):
            err(f"kp {k}: malformed fields {row.tolist()}"); continue
        o, layer, xiq = unpack_octave(octave)
        half = 2.0 ** o / 2
        bound = lambda f, t: (f.ref.ex[t] if np.isfinite(f.ref.ex[t]) else 1.0) * half + 8 * U * (abs(x) + abs(y) + half)
        pool = sorted(by_octave.get(o, []), key=lambda f: (f.x - x) ** 2 + (f.y - y) ** 2)
        near = [f for f in pool if abs(f.x - x) <= bound(f, 0) and abs(f.y - y) <= bound(f, 1)]
        if not near:
            fin = pool[0] if pool else None
            err(f"kp {k}: ({x:.4f}, {y:.4f}) octave {o} matches no extremum of the reference"
                + (f" (nearest ({fin.x:.4f}, {fin.y:.4f}), bounds {bound(fin, 0):.2g}, {bound(fin, 1):.2g})" if fin else ""))
            continue
        # two scan positions may end a pixel apart on the same extremum: the keypoint belongs to the one that has its peak free
        circ = lambda a, b: abs((a - b + 180.0) % 360.0 - 180.0)
        fin = pk = None
        problems = []
        for f in near:
            if layer != f.ref.layer:
                problems.append(f"layer {layer} vs {f.ref.layer}"); continue
            peaks = st.orientation_of(f).peaks
            q = min(peaks, key=lambda p: circ(360.0 - 10.0 * p.bin, angle), default=None)
            # a peak's parabola moves it by less than half a bin; where its own bound is within the limit, that bound holds
            if q is None or circ(360.0 - 10.0 * q.bin, angle) > 5.0 + 1e-3 or (q.bound <= ANGLE_LIMIT and circ(q.angle, angle) > q.bound):
                problems.append(f"angle {angle} is no peak of the reference's histogram" + (f" (nearest bin {q.bin}, {q.angle:.4f}, bound {q.bound:.3g})" if q else "")); continue
            if (id(f), q.bin) in taken:
                problems.append(f"angle {angle:.3f} is reported twice (also kp {taken[(id(f), q.bin)]})"); continue
            fin, pk = f, q
            break
        if fin is None:
            err(f"kp {k}: ({x:.3f}, {y:.3f}): " + "; ".join(problems)); continue
        ref = fin.ref
        loose = bool(fin.why)
        if loose:
            undecided("reported", k, tuple(fin.why))
        e_xi = ref.ex[2] if np.isfinite(ref.ex[2]) else 1.0
        if abs(size - fin.size) > fin.size * (math.log(2) / N_LAYERS * e_xi * 1.01 + 16 * U):
            err(f"kp {k}: size {size!r} vs {fin.size!r} (bound on xi {e_xi:.3g})")
        if abs(resp - fin.response) > ref.e_contrast + 4 * U * fin.response:
            err(f"kp {k}: response {resp!r} vs {fin.response!r} (bound {ref.e_contrast:.3g})")
        q = (ref.offset[2] + 0.5) * 255
        if not (np.rint(q - 255 * e_xi - 1e-6) <= xiq <= np.rint(q + 255 * e_xi + 1e-6)):
            err(f"kp {k}: octave field's offset byte {xiq} vs {q:.4f}")
        rep.n_partial_disc += fin.ori.n_skipped > 0
        taken[(id(fin), pk.bin)] = k
        if not pk.exists64 or pk.bound > ANGLE_LIMIT:
            undecided("reported", k, ("a peak within the histogram's error radius",))
        if not loose and not st.kept64(fin):
            err(f"kp {k}: ({x:.3f}, {y:.3f}) is a candidate the reference rejects")
        sure = [s[0] for s in fin.starts if s[2].kept64] or [s[0] for s in fin.starts]
        keys[k] = None if min(s[0] for s in fin.starts) < min(sure) else min(sure) + (pk.bin,)
    # ---- the cuts
    cut, e_cut, cut_fin = None, 0.0, None
    if nfeatures > 0 and nfeatures < len(reference):
        by_resp = sorted(reference, key=lambda t: -t[1].response)
        cut_fin = by_resp[nfeatures - 1][1]
        cut, e_cut = cut_fin.response, cut_fin.ref.e_contrast
        r_min = kp[:, 4].min() if len(kp) else 0.0
        if len(kp) < nfeatures and max_kp is None:
            err(f"nfeatures {nfeatures}: only {len(kp)} reported")
        if int((kp[:, 4] > r_min).sum()) >= nfeatures:
            err(f"nfeatures {nfeatures}: {int((kp[:, 4] > r_min).sum())} responses above the weakest reported")
    if max_kp is not None and len(kp) > max_kp:
        err(f"max_keypoints {max_kp}: {len(kp)} reported")
    last_key = None
    if max_kp is not None and len(kp) == max_kp:
        known = [t for t in keys if t is not None]
        last_key = max(known) if known else ()
    # ---- completeness: what the reference keeps with margin is reported
    for key, fin, pk in reference:
        here = (id(fin), pk.bin) in taken
        if last_key is not None and key > last_key:
            continue
        if cut is not None and fin is not cut_fin:
            tol = e_cut + fin.ref.e_contrast + 4 * U * cut
            if abs(fin.response - cut) <= tol:
                if not here:
                    undecided("tie at the nfeatures cut", key, ())
                continue
            if fin.response < cut:
                if here and not fin.why:
                    err(f"kp {taken[(id(fin), pk.bin)]}: response {fin.response!r} lies below the nfeatures cut {cut!r}")
                continue
        if here:
            continue
        if fin.why or not pk.decided:
            undecided("missing, kept by the reference without margin", key, tuple(fin.why) or ("peak",))
        else:
            err(f"missing keypoint ({fin.x:.3f}, {fin.y:.3f}) size {fin.size:.3f} angle {pk.angle:.3f} octave {fin.o - 1} layer {fin.layer}")
    # ---- order: octave, detection layer, row, column, peak bin
    prev = None
    for k, key in enumerate(keys):
        if key is None:
            continue
        if prev is not None and not prev[1] < key:
            err(f"order: kp {prev[0]} {prev[1]} before kp {k} {key}")
        prev = (k, key)
    # ---- descriptors, from the reported fields
    which = params.get("describe")
    if which is None:
        which = sample_indices(np.asarray(keypoints).reshape(-1, 7)) if len(kp) else np.zeros(0, np.int64)
    which = set(np.asarray(which, np.int64).tolist())
    tolerance = params.get("desc_tol", DESC_TOL)
    for k, row in enumerate(kp):
        if row[5] != int(row[5]) or row[2] <= 0:
            continue
        o, layer, xo, yo, scl = octave_position(row)
        if not (0 <= o < len(st.G) and 1 <= layer <= N_LAYERS):
            continue
        clipped = descriptor_geometry(st.G[o][layer].shape, scl)[1]
        rep.n_clipped_radius += clipped
        if k not in which and not clipped:
            continue
        tie = lambda v: abs(abs(v - math.floor(v)) - 0.5) <= 8 * U * (abs(v) + 1)
        if tie(xo) or tie(yo) or tie(3 * scl * math.sqrt(2) * 2.5):
            undecided("descriptor rounding", k, ()); continue
        dist = descriptor_distance(descriptor(st.G[o][layer], xo, yo, scl, row[3]), desc[k])
        rep.n_described += 1
        rep.max_desc_distance = max(rep.max_desc_distance, dist)
        if not dist <= tolerance:
            err(f"kp {k}: descriptor at distance {dist:.3g} (tolerance {tolerance:.3g})")
    return rep
