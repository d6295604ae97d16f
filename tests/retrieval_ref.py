"""Restatement of include/esfm.h "Image retrieval" in numpy, line by line of the rule list.  Imports nothing from the product or
from oracle/.  Float arithmetic is per element in the stated order (f32 for distances, f64 for the quantisation and the scores);
every sum across descriptors is an integer sum."""
from dataclasses import dataclass

import numpy as np

L2, HAMMING = 0, 1
MAX_DIM, MAX_SETS = 32768, 8192


@dataclass
class Options:
    n_centres: int = 64
    kmeans_iterations: int = 10
    max_train: int = 65536
    top_k: int = 10
    window: int = 0

    @property
    def kw(self):
        return dict(n_centres=self.n_centres, kmeans_iterations=self.kmeans_iterations, max_train=self.max_train, top_k=self.top_k,
                    window=self.window)


def working(rows, metric):
    """the rows as working f32 components: [n, d]"""
    if metric == L2:
        return np.ascontiguousarray(rows, np.float32)
    rows = np.ascontiguousarray(rows, np.uint8)
    return np.unpackbits(rows, axis=1, bitorder="little").astype(np.float32)


def dist(x, m):
    """[rows, centres] f32: acc = 0; for t ascending: df = x_t - m_t; acc = acc + df df (multiply and add rounded separately)"""
    acc = np.zeros((x.shape[0], m.shape[0]), np.float32)
    for t in range(x.shape[1]):
        df = x[:, t, None] - m[None, :, t]
        acc = acc + df * df
    return acc


def assign(x, m):
    """the lowest centre index with the smallest distance"""
    if x.shape[0] == 0:
        return np.zeros(0, np.int32)
    return np.argmin(dist(x, m), axis=1).astype(np.int32)      # argmin returns the first minimum


def q(x):
    return np.rint(np.asarray(x, np.float32).astype(np.float64) * 65536.0).astype(np.int64)


def sample_rows(total, max_train):
    stride = -(-total // max_train)
    return np.arange(0, total, stride, dtype=np.int64)


def train(sets, metric, o):
    x_all = working(np.concatenate(sets, axis=0), metric)
    total = x_all.shape[0]
    assert total > 0
    x = x_all[sample_rows(total, o.max_train)]
    nt = x.shape[0]
    m = np.stack([x[(c * nt) // o.n_centres] for c in range(o.n_centres)]).astype(np.float32)
    qx = q(x)
    for _ in range(o.kmeans_iterations):
        a = assign(x, m)
        for c in range(o.n_centres):
            sel = a == c
            count = int(sel.sum())
            if count > 0:
                s = qx[sel].sum(axis=0, dtype=np.int64)
                m[c] = ((s.astype(np.float64) / np.float64(count)) / 65536.0).astype(np.float32)
    return m


def vlad(sets, metric, m):
    """(vlad int8 [n, D], norm2 int32 [n], assign int32 [rows], S int64 [n, D])"""
    n_centres, d = m.shape
    D = n_centres * d
    qm = q(m)
    V = np.zeros((len(sets), D), np.int8); norm2 = np.zeros(len(sets), np.int32); S_all = np.zeros((len(sets), D), np.int64)
    assigns = []
    for i, rows in enumerate(sets):
        x = working(rows, metric) if len(rows) else np.zeros((0, d), np.float32)
        a = assign(x, m)
        assigns.append(a)
        qx = q(x)
        S = np.zeros((n_centres, d), np.int64)
        for c in range(n_centres):
            sel = a == c
            S[c] = qx[sel].sum(axis=0, dtype=np.int64) - np.int64(sel.sum()) * qm[c]
        S = S.reshape(-1)
        S_all[i] = S
        max_s = int(np.abs(S).max()) if D else 0
        if max_s:
            mag = np.rint((127.0 * np.sqrt(np.abs(S).astype(np.float64))) / np.sqrt(np.float64(max_s)))
            V[i] = (np.sign(S) * mag.astype(np.int64)).astype(np.int8)
        norm2[i] = int((V[i].astype(np.int64) ** 2).sum())
    return V, norm2, (np.concatenate(assigns) if assigns else np.zeros(0, np.int32)), S_all


def rank(V, top_k):
    """(nearest int32 [n, top_k], dots int32 [n, n], scores float64 [n, n])"""
    V = np.asarray(V, np.int8)
    n = V.shape[0]
    dots = (V.astype(np.int64) @ V.astype(np.int64).T).astype(np.int32)
    norm2 = np.diagonal(dots).astype(np.int64) if n else np.zeros(0, np.int64)
    root = np.sqrt(norm2.astype(np.float64))
    scores = np.zeros((n, n), np.float64)
    ok = norm2 > 0
    for i in range(n):
        for j in range(n):
            if ok[i] and ok[j]:
                scores[i, j] = np.float64(dots[i, j]) / (root[i] * root[j])
    nearest = np.full((n, top_k), -1, np.int32)
    for i in range(n):
        if not ok[i]:
            continue
        cand = [j for j in range(n) if j != i and ok[j]]
        cand.sort(key=lambda j: (-scores[i, j], j))
        for k, j in enumerate(cand[:top_k]):
            nearest[i, k] = j
    return nearest, dots, scores


def pair_list(nearest, n_sets, window):
    """int32 [P, 2], ascending by (first, second), no duplicates"""
    chosen = set()
    if nearest is not None:
        for i in range(n_sets):
            for j in np.asarray(nearest).reshape(n_sets, -1)[i]:
                if j >= 0:
                    chosen.add((max(i, int(j)), min(i, int(j))))
    for i in range(n_sets):
        for w in range(1, window + 1):
            if i - w >= 0:
                chosen.add((i, i - w))
    return np.array(sorted(chosen), np.int32).reshape(-1, 2)


def chain(sets, metric, o):
    """every stage's output of the whole chain, as a dict"""
    m = train(sets, metric, o)
    V, norm2, a, S = vlad(sets, metric, m)
    nearest, dots, scores = rank(V, o.top_k)
    return dict(centres=m, vlad=V, norm2=norm2, assign=a, sums=S, nearest=nearest, dots=dots, scores=scores,
                pairs=pair_list(nearest, len(sets), o.window))
