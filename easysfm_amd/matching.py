"""Host-side mirror of the reference's matching interface over the C ABI.

``FeatureMatching.matchFeaturesSURF / matchFeaturesORB`` keep the names, argument meaning and
append-to-``matches`` behaviour of cpp_code/include/feature_matching.h:17-21 (bodies:
cpp_code/src/feature_matching.cpp:71-97, :115-142).  ``match_all_pairs`` is the batched pair loop of
cpp_code/test/sfm.cpp:140-161 with descriptors resident in HBM.  All compute happens in
libesfm_hip.so; nothing here falls back to the CPU.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._lib import ESFM_HAMMING, ESFM_L2_F32, Context, check, default_context, lib
from .types import DMatch, Frame


def _ptr(a: np.ndarray) -> C.c_void_p:
    return C.c_void_p(a.ctypes.data)


def _as_desc(a, dtype) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype)
    if a.ndim != 2:
        raise ValueError("descriptors must be a 2-D array [rows, width]")
    return a


def _one_pair(q, t, dtype, ctx, same_width=True):
    ctx = ctx or default_context()
    q = _as_desc(q, dtype); t = _as_desc(t, dtype)
    if same_width and q.shape[1] != t.shape[1]:
        raise ValueError("descriptor widths differ")
    return q, t, ctx


def _knn2(fn, q, t, dtype, ctx):
    q, t, ctx = _one_pair(q, t, dtype, ctx)
    nq = q.shape[0]
    idx = np.full((nq, 2), -1, np.int32); dist = np.zeros((nq, 2), np.float32)
    check(fn(ctx.handle, _ptr(q), nq, _ptr(t), t.shape[0], q.shape[1], _ptr(idx), _ptr(dist)))
    return idx, dist


def knn_match_l2(q, t, ctx: Optional[Context] = None) -> Tuple[np.ndarray, np.ndarray]:
    """knnMatch(q, t, out, 2) under NORM_L2 (exact brute force).  Returns (idx[nq,2], dist[nq,2])."""
    return _knn2(lib().esfm_knn2_l2_f32, q, t, np.float32, ctx)


def knn_match_hamming(q, t, ctx: Optional[Context] = None) -> Tuple[np.ndarray, np.ndarray]:
    """knnMatch(q, t, out, 2) for "BruteForce-Hamming".  Returns (idx[nq,2], dist[nq,2])."""
    return _knn2(lib().esfm_knn2_hamming, q, t, np.uint8, ctx)


def _match(fn, q, t, dtype, ctx, filt, same_width=False):
    """One pair through a single-pair entry point fn(ctx, q, nq, t, nt, width, *filt, queryIdx, trainIdx, distance, &n)."""
    q, t, ctx = _one_pair(q, t, dtype, ctx, same_width)
    nq = q.shape[0]
    qi = np.empty(max(nq, 1), np.int32); ti = np.empty(max(nq, 1), np.int32); d = np.empty(max(nq, 1), np.float32)
    n = C.c_int32(0)
    check(fn(ctx.handle, _ptr(q), nq, _ptr(t), t.shape[0], q.shape[1], *filt, _ptr(qi), _ptr(ti), _ptr(d), C.byref(n)))
    return qi[:n.value].copy(), ti[:n.value].copy(), d[:n.value].copy()


def match_l2(q, t, ratio: float = 0.5, ctx: Optional[Context] = None):
    """2-NN + Lowe ratio for float descriptors; returns (queryIdx, trainIdx, distance) arrays."""
    return _match(lib().esfm_match_l2_f32, q, t, np.float32, ctx, (float(ratio),))


def match_hamming(q, t, ratio: float = 0.8, ctx: Optional[Context] = None):
    return _match(lib().esfm_match_hamming, q, t, np.uint8, ctx, (float(ratio),))


def _match_pairs_host(fn, sets, pairs, metric, ctx, *filt):
    """The batched pair loop through HOST pointers, fn(ctx, metric, bank, ..., pairs, n_pairs, *filt, outputs...)."""
    ctx = ctx or default_context()
    dt = np.float32 if metric == ESFM_L2_F32 else np.uint8
    sets = [_as_desc(s_, dt) for s_ in sets]
    width = sets[0].shape[1]
    off = np.zeros(len(sets) + 1, np.int32)
    np.cumsum([s_.shape[0] for s_ in sets], out=off[1:])
    bank = np.ascontiguousarray(np.concatenate(sets, axis=0)) if off[-1] else np.zeros((1, width), dt)
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    total = int(sum(sets[i].shape[0] for i, _ in pairs))
    qi = np.zeros(max(total, 1), np.int32); ti = np.zeros(max(total, 1), np.int32); d = np.zeros(max(total, 1), np.float32)
    n_out = np.zeros(max(len(pairs), 1), np.int32); out_off = np.zeros(len(pairs) + 1, np.int64)
    check(fn(ctx.handle, metric, _ptr(bank), _ptr(off), len(sets), width, _ptr(pairs), len(pairs), *filt,
             _ptr(qi), _ptr(ti), _ptr(d), _ptr(n_out), _ptr(out_off)))
    return [(qi[o:o + k].copy(), ti[o:o + k].copy(), d[o:o + k].copy()) for o, k in zip(out_off[:-1], n_out[:len(pairs)])]


def match_pairs_host(sets: Sequence[np.ndarray], pairs, ratio: float, metric: int = ESFM_L2_F32, ctx: Optional[Context] = None):
    """esfm_match_pairs: the batched pair loop through HOST pointers (upload once, one launch sequence, one read-back) -- what the
    C++ driver calls.  Returns [(queryIdx, trainIdx, distance)] per pair."""
    return _match_pairs_host(lib().esfm_match_pairs, sets, pairs, metric, ctx, float(ratio))


# ---- cross-check (mutual nearest neighbour), include/esfm.h "Cross-check matching": ratio=None is cross alone, a number is
# ratio+cross (the ratio test in both directions as well)
def _cross_args(ratio):
    return (0, 0.0) if ratio is None else (1, float(ratio))


def match_cross_l2(q, t, ratio: Optional[float] = None, ctx: Optional[Context] = None):
    """Mutual nearest neighbours of float descriptors (cv2.BFMatcher(NORM_L2, crossCheck=True) as feature_match.py:24-27 uses it, under
    the strict rule of esfm.h); with `ratio`, also Lowe's test in both directions.  Returns (queryIdx, trainIdx, distance) arrays."""
    return _match(lib().esfm_match_cross_l2_f32, q, t, np.float32, ctx, _cross_args(ratio), same_width=True)


def match_cross_hamming(q, t, ratio: Optional[float] = None, ctx: Optional[Context] = None):
    """match_cross_l2 for binary descriptors (Hamming distance)."""
    return _match(lib().esfm_match_cross_hamming, q, t, np.uint8, ctx, _cross_args(ratio), same_width=True)


def match_cross_pairs_host(sets: Sequence[np.ndarray], pairs, ratio: Optional[float] = None, metric: int = ESFM_L2_F32,
                           ctx: Optional[Context] = None):
    """esfm_match_cross_pairs: match_pairs_host with the cross-check filter.  Returns [(queryIdx, trainIdx, distance)] per pair."""
    return _match_pairs_host(lib().esfm_match_cross_pairs, sets, pairs, metric, ctx, *_cross_args(ratio))


# ---- epipolar-guided matching, include/esfm.h "Epipolar-guided matching": the search of a query row restricted to the train rows the
# pair's essential matrix admits.  ratio=None switches the ratio test off (then cross_check must be on)
def _guided_args(ratio, cross_check):
    return (0, 0.0, int(bool(cross_check))) if ratio is None else (1, float(ratio), int(bool(cross_check)))


def _as_kp(kp, rows) -> np.ndarray:
    kp = np.ascontiguousarray(kp, np.float32).reshape(-1, 2)
    if kp.shape[0] != rows:
        raise ValueError("one keypoint (u, v) per descriptor row")
    return kp


def _geometry(E, K4, n_pairs):
    E = np.ascontiguousarray(E, np.float64).reshape(-1, 9); K4 = np.ascontiguousarray(K4, np.float32).reshape(-1, 4)
    if E.shape[0] != n_pairs or K4.shape[0] != n_pairs:
        raise ValueError("one essential matrix and one K4 (fx, cx, fy, cy) per pair")
    return E, K4


def _match_guided(fn, q, kp_q, t, kp_t, dtype, E, K4, max_epipolar_px, ratio, cross_check, ctx):
    q, t, ctx = _one_pair(q, t, dtype, ctx)
    kp_q = _as_kp(kp_q, q.shape[0]); kp_t = _as_kp(kp_t, t.shape[0])
    E, K4 = _geometry(E, K4, 1)
    nq = q.shape[0]
    qi = np.empty(max(nq, 1), np.int32); ti = np.empty(max(nq, 1), np.int32); d = np.empty(max(nq, 1), np.float32)
    n = C.c_int32(0)
    check(fn(ctx.handle, _ptr(q), _ptr(kp_q), nq, _ptr(t), _ptr(kp_t), t.shape[0], q.shape[1], _ptr(E), _ptr(K4), float(max_epipolar_px),
             *_guided_args(ratio, cross_check), _ptr(qi), _ptr(ti), _ptr(d), C.byref(n)))
    return qi[:n.value].copy(), ti[:n.value].copy(), d[:n.value].copy()


def match_guided_l2(q, kp_q, t, kp_t, E, K4, max_epipolar_px: float = 1.0, ratio: Optional[float] = 0.5, cross_check: bool = False,
                    ctx: Optional[Context] = None):
    """esfm_match_guided_l2_f32: one pair's guided match list.  kp_q / kp_t: [rows, 2] pixels, E [3,3], K4 = fx, cx, fy, cy (the query
    frame's).  Returns (queryIdx, trainIdx, distance) arrays."""
    return _match_guided(lib().esfm_match_guided_l2_f32, q, kp_q, t, kp_t, np.float32, E, K4, max_epipolar_px, ratio, cross_check, ctx)


def match_guided_hamming(q, kp_q, t, kp_t, E, K4, max_epipolar_px: float = 1.0, ratio: Optional[float] = 0.8, cross_check: bool = False,
                         ctx: Optional[Context] = None):
    """match_guided_l2 for binary descriptors (Hamming distance)."""
    return _match_guided(lib().esfm_match_guided_hamming, q, kp_q, t, kp_t, np.uint8, E, K4, max_epipolar_px, ratio, cross_check, ctx)


def match_guided_pairs_host(sets: Sequence[np.ndarray], keypoints: Sequence[np.ndarray], pairs, E, K4, max_epipolar_px: float,
                            ratio: Optional[float], cross_check: bool = False, metric: int = ESFM_L2_F32, ctx: Optional[Context] = None):
    """esfm_match_guided_pairs: the guided pass of a pair list through HOST pointers.  Returns [(queryIdx, trainIdx, distance)] per pair."""
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    E, K4 = _geometry(E, K4, len(pairs))
    rows = sum(np.asarray(s_).shape[0] for s_ in sets)
    kp = np.concatenate([_as_kp(k, np.asarray(s_).shape[0]) for k, s_ in zip(keypoints, sets)], axis=0) if rows else np.zeros((1, 2), np.float32)

    def fn(h, metric_, bank, *rest):
        return lib().esfm_match_guided_pairs(h, metric_, bank, _ptr(kp), *rest)
    return _match_pairs_host(fn, sets, pairs, metric, ctx, _ptr(E), _ptr(K4), float(max_epipolar_px), *_guided_args(ratio, cross_check))


class FeatureMatching:
    """Mirror of p3dv::FeatureMatching's matching members (feature_matching.h:17-21)."""

    def __init__(self, ctx: Optional[Context] = None):
        self._ctx = ctx

    @property
    def ctx(self) -> Context:
        return self._ctx or default_context()

    def matchFeaturesORB(self, cur_frame_1: Frame, cur_frame_2: Frame, matches: List[DMatch],
                         ratio_thre: float = 0.8, show: bool = False, cross_check: bool = False) -> bool:
        """feature_matching.cpp:71-97.  Query = cur_frame_1, train = cur_frame_2; survivors are
        APPENDED to `matches` (the reference never clears it, :90).  cross_check: keep mutual nearest neighbours
        that also pass the ratio test in both directions (match_cross_hamming)."""
        if cross_check:
            qi, ti, d = match_cross_hamming(cur_frame_1.descriptors, cur_frame_2.descriptors, ratio_thre, self.ctx)
        else:
            qi, ti, d = match_hamming(cur_frame_1.descriptors, cur_frame_2.descriptors, ratio_thre, self.ctx)
        matches.extend(DMatch(int(a), int(b), float(c)) for a, b, c in zip(qi, ti, d))
        return True

    def matchFeaturesSURF(self, cur_frame_1: Frame, cur_frame_2: Frame, matches: List[DMatch],
                          ratio_thre: float = 0.5, show: bool = False, cross_check: bool = False) -> bool:
        """feature_matching.cpp:115-142 with the exact brute-force matcher the Python prototype
        uses (feature_match.py:33-34) instead of the approximate FlannBasedMatcher (:120).  cross_check: keep mutual
        nearest neighbours that also pass the ratio test in both directions (match_cross_l2)."""
        if cross_check:
            qi, ti, d = match_cross_l2(cur_frame_1.descriptors, cur_frame_2.descriptors, ratio_thre, self.ctx)
        else:
            qi, ti, d = match_l2(cur_frame_1.descriptors, cur_frame_2.descriptors, ratio_thre, self.ctx)
        matches.extend(DMatch(int(a), int(b), float(c)) for a, b, c in zip(qi, ti, d))
        return True

    def detectFeaturesSURF(self, cur_frame: Frame, minHessian: int = 400, show: bool = False) -> bool:
        """feature_matching.cpp:43-69 (features.detectFeaturesSURF)."""
        from .features import detectFeaturesSURF
        return detectFeaturesSURF(cur_frame, minHessian, show, self._ctx)

    def detectFeaturesORB(self, cur_frame: Frame, max_num: int = 5000, show: bool = False) -> bool:
        """feature_matching.cpp:14-41 (features.detectFeaturesORB)."""
        from .features import detectFeaturesORB
        return detectFeaturesORB(cur_frame, max_num, show, self._ctx)

    def matchFeaturesSIFT(self, cur_frame_1: Frame, cur_frame_2: Frame, matches: List[DMatch],
                          ratio_thre: float = 0.7, show: bool = False, cross_check: bool = False) -> bool:
        """The prototype's SIFT matching (feature_match.py, nn_ratio 0.7): matchFeaturesSURF's L2 path on 128-float rows."""
        return self.matchFeaturesSURF(cur_frame_1, cur_frame_2, matches, ratio_thre, show, cross_check)

    def detectFeaturesSIFT(self, cur_frame: Frame, nfeatures: int = 0, show: bool = False) -> bool:
        """The prototype's SIFT branch (features.detectFeaturesSIFT)."""
        from .features import detectFeaturesSIFT
        return detectFeaturesSIFT(cur_frame, nfeatures, show, self._ctx)

    # ---- frame selection (feature_matching.cpp:160-268): integer logic on the track matrix, host side ----
    def findInitializeFramePair(self, feature_track_matrix, frames, img_match_graph, min_track_num_init: int = 100,
                                max_depth_baseline_ratio_init: float = 50.0, max_h_inlier_ratio: Optional[float] = None,
                                h_stats: Optional[dict] = None):
        """feature_matching.cpp:160-229 (defaults feature_matching.h:26).  feature_track_matrix: [n_frames, n_unique] bool (frame sees track);
        img_match_graph[i][j].appro_depth (or a 2-D array of depths): depth / baseline of pair (i, j < i).
        Returns (found, initialization_frame_1, initialization_frame_2, depth_init).  The pair maximising the sum, over
        the tracks both frames see, of the number of frames that see the track; ties go to the LATER pair in (i, j < i)
        order (`>=` at :203); pairs whose depth / baseline exceeds the limit are skipped (:193-194).
        max_h_inlier_ratio (not in the reference): when given, a pair that passed the depth guard and whose
        img_match_graph[i][j].h_inlier_ratio exceeds it is skipped at the same place -- a homography explains it nearly as well as
        the essential matrix, so it is planar or rotation-only (esfm.h "Homography RANSAC"); an entry without the field counts as 0.
        h_stats (a dict, or None) then receives "candidates", the pairs that reached this test, and "skipped", those it skipped."""
        T = np.asarray(feature_track_matrix, bool)
        n_frames = len(frames)
        T = T[:n_frames]
        weight = T.sum(axis=0).astype(np.int64)                    # point_track_frame_num (:172-180)
        score = (T.astype(np.int64) * weight[None, :]) @ T.T.astype(np.int64)

        def depth(i, j):
            e = img_match_graph[i][j]
            return float(getattr(e, "appro_depth", e))

        best, f1, f2, d_init = int(min_track_num_init), 0, 0, None
        candidates = skipped = 0
        for i in range(n_frames):
            for j in range(i):
                d = depth(i, j)
                if d > max_depth_baseline_ratio_init:
                    continue
                if max_h_inlier_ratio is not None:
                    candidates += 1
                    if float(getattr(img_match_graph[i][j], "h_inlier_ratio", 0.0)) > max_h_inlier_ratio:
                        skipped += 1
                        continue
                if score[i, j] >= best:
                    best, f1, f2, d_init = int(score[i, j]), i, j, d
        if h_stats is not None:
            h_stats["candidates"], h_stats["skipped"] = candidates, skipped
        if f1 == f2:
            print("Failed to find proper frame pair for initialization. Use default frame [1] and frame [0]")
            return False, 1, 0, None                                # depth_init is left unset by the reference (:217-223)
        return True, f1, f2, d_init

    def findNextFrame(self, feature_track_matrix, frames_to_process, unique_3d_point_ids, next_frame: int = -1) -> int:
        """feature_matching.cpp:231-268: among the frames still to process, the one seeing most of the already
        triangulated tracks; the FIRST such frame on ties (strict `>` at :252); `next_frame` is returned unchanged when
        no candidate sees any (the reference leaves its output argument untouched)."""
        T = np.asarray(feature_track_matrix, bool)
        ids = np.asarray(unique_3d_point_ids, np.int64)
        best = 0
        for i, todo in enumerate(frames_to_process):
            if not todo:
                continue
            c = int(T[i, ids].sum()) if len(ids) else 0
            if c > best:
                best, next_frame = c, i
        return next_frame


# ------------------------------------------------------------------------------------------------
@dataclass
class PairMatches:
    """Result of a batched call: pair p owns out slice [offset[p], offset[p] + n_out[p])."""
    pairs: np.ndarray        # int32 [n_pairs, 2] (query set, train set)
    offset: np.ndarray       # int64 [n_pairs + 1]
    n_out: "object"          # device int32 [n_pairs]   (torch tensor)
    query_idx: "object"      # device int32 [sum nq]
    train_idx: "object"      # device int32
    distance: "object"       # device float32
    ctx: "object" = None

    def to_host(self) -> List[Tuple[np.ndarray, np.ndarray, np.ndarray]]:
        if self.ctx is not None:
            self.ctx.synchronize()
        n = self.n_out.cpu().numpy()
        q = self.query_idx.cpu().numpy(); t = self.train_idx.cpu().numpy(); d = self.distance.cpu().numpy()
        out = []
        for p in range(len(self.pairs)):
            o = int(self.offset[p]); k = int(n[p])
            out.append((q[o:o + k].copy(), t[o:o + k].copy(), d[o:o + k].copy()))
        return out


class DescriptorBank:
    """All descriptor sets of a reconstruction, concatenated in one HBM buffer (torch owns the
    memory; the kernels see a raw device pointer)."""

    def __init__(self, sets: Sequence[np.ndarray], metric: int, device: str = "cuda:0", keypoints: Optional[Sequence[np.ndarray]] = None):
        """keypoints (optional): one [rows, 2] array of pixel positions per set, kept beside the rows for PairMatcher.match_guided."""
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("no MI355X visible: DescriptorBank needs a GPU (easysfm_amd has no CPU fallback)")
        self.metric = metric
        dt = np.float32 if metric == ESFM_L2_F32 else np.uint8
        sets = [_as_desc(s, dt) for s in sets]
        widths = {s.shape[1] for s in sets}
        if len(widths) != 1:
            raise ValueError("all descriptor sets must have the same width")
        self.width = widths.pop()
        self.rows = np.array([s.shape[0] for s in sets], np.int32)
        self.row_offset = np.zeros(len(sets) + 1, np.int32)
        np.cumsum(self.rows, out=self.row_offset[1:])
        host = np.concatenate(sets, axis=0) if sets else np.zeros((0, self.width), dt)
        self.device = torch.device(device)
        self.data = torch.from_numpy(host).to(self.device)
        self.keypoints = None
        if keypoints is not None:
            if len(keypoints) != len(sets):
                raise ValueError("one keypoint array per descriptor set")
            kp = [_as_kp(k, s.shape[0]) for k, s in zip(keypoints, sets)]
            self.keypoints = torch.from_numpy(np.concatenate(kp, axis=0) if kp else np.zeros((0, 2), np.float32)).to(self.device)
        self._matchers = []          # live PairMatchers (weak): update() re-prepares them

    @property
    def n_sets(self) -> int:
        return len(self.rows)

    def update(self, sets: Sequence[np.ndarray]) -> None:
        """Replace the rows IN PLACE (same set sizes: the buffer and every PairMatcher's output slices stay as they are).  The
        operand images a PairMatcher derived from the old rows are stale after this: every matcher of this bank is re-prepared
        (esfm.h: a prepared buffer must be prepared again before a match call relies on it)."""
        import torch
        dt = np.float32 if self.metric == ESFM_L2_F32 else np.uint8
        sets = [_as_desc(s, dt) for s in sets]
        if [s.shape[0] for s in sets] != list(self.rows) or any(s.shape[1] != self.width for s in sets):
            raise ValueError("update() keeps the bank's shape: same number of sets, rows per set and width")
        for m in list(self._matchers):
            m.release()
        if len(sets) and int(self.row_offset[-1]):
            self.data.copy_(torch.from_numpy(np.concatenate(sets, axis=0)))
            torch.cuda.synchronize(self.device)
        for m in list(self._matchers):
            m.prepare()


class _WeakCall:
    """A weak reference that forwards attribute access to its referent (DescriptorBank keeps its matchers without owning them)."""

    def __init__(self, ref):
        self._ref = ref

    def __call__(self):
        return self._ref()

    def __getattr__(self, name):
        obj = self._ref()
        if obj is None:
            return lambda *a, **k: None
        return getattr(obj, name)


class PairMatcher:
    """Batched pair loop (sfm.cpp:140-161): one call matches a whole pair list on one GPU.
    Output buffers are allocated once and reused across calls."""

    def __init__(self, bank: DescriptorBank, pairs: np.ndarray, ctx: Optional[Context] = None):
        import torch
        self.bank = bank
        self.pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        self.torch = torch
        dev_index = bank.device.index or 0
        if ctx is None:
            ctx = Context.on_torch_stream(dev_index)
        self.ctx = ctx
        total = int(bank.rows[self.pairs[:, 0]].sum()) if len(self.pairs) else 0
        self.total_queries = total
        dev = bank.device
        self.query_idx = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
        self.train_idx = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
        self.distance = torch.empty(max(total, 1), dtype=torch.float32, device=dev)
        self.n_out = torch.empty(max(len(self.pairs), 1), dtype=torch.int32, device=dev)
        self.offset = np.zeros(len(self.pairs) + 1, np.int64)
        self.knn_idx = None
        self.knn_dist = None
        torch.cuda.synchronize(dev)   # the bank upload ran on torch's stream; kernels run on ctx's
        import weakref
        bank._matchers = [m for m in bank._matchers if m() is not None]
        self._ref = weakref.ref(self)
        bank._matchers.append(_WeakCall(self._ref))
        self.prepare()

    def prepare(self) -> None:
        """Part of the upload: the per-row operands the matcher derives from the resident descriptors (esfm_match_prepare_dev) --
        computed once here instead of at the head of every match() / knn2() call.  ONE prepared buffer per context (esfm.h): a
        second PairMatcher on the same Context takes the prepared state over, and the first one's calls re-derive the operands
        every time (correct, slower) until its prepare() is called again.  The bank's rows must not change while prepared:
        DescriptorBank.update() is the way to rewrite them."""
        b = self.bank
        check(lib().esfm_match_prepare_dev(self.ctx.handle, b.metric, C.c_void_p(b.data.data_ptr()), int(b.row_offset[-1]), b.width))

    def release(self) -> None:
        """esfm_match_release_prepared_buffer: to be called before the bank's buffer is freed or rewritten (close() / garbage collection /
        DescriptorBank.update() do) -- a later allocation at the same address must not inherit this one's operand images.  Releases
        only if THIS bank's buffer is the one prepared on the context: an older matcher that is garbage-collected must not take the
        prepared operands from the live one on the same Context (its calls would silently re-derive them every time)."""
        try:
            h = self.ctx.handle
        except RuntimeError:
            return
        check(lib().esfm_match_release_prepared_buffer(h, C.c_void_p(self.bank.data.data_ptr())))

    def close(self) -> None:
        self.release()
        self.bank._matchers = [m for m in self.bank._matchers if m() is not None and m() is not self]

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    def set_prepared_check(self, enable: bool) -> None:
        """esfm_ctx_set_prepared_check: fingerprint the prepared buffer and verify it on every call (a debugging aid)."""
        check(lib().esfm_ctx_set_prepared_check(self.ctx.handle, 1 if enable else 0))

    def _call(self, fn, *args) -> None:
        """fn(ctx, metric, bank, row_offset, n_sets, width, pairs, n_pairs, *args, offset): one pair-list entry point."""
        b = self.bank
        check(fn(self.ctx.handle, b.metric, C.c_void_p(b.data.data_ptr()), _ptr(b.row_offset), b.n_sets, b.width,
                 _ptr(self.pairs), len(self.pairs), *args, _ptr(self.offset)))

    def _lists(self, fn, *filt) -> PairMatches:
        self._call(fn, *filt, C.c_void_p(self.query_idx.data_ptr()), C.c_void_p(self.train_idx.data_ptr()),
                   C.c_void_p(self.distance.data_ptr()), C.c_void_p(self.n_out.data_ptr()))
        return PairMatches(self.pairs, self.offset, self.n_out, self.query_idx, self.train_idx, self.distance, self.ctx)

    def match(self, ratio: float) -> PairMatches:
        """Enqueue the whole pair list; does not synchronise."""
        return self._lists(lib().esfm_match_pairs_dev, float(ratio))

    def match_cross(self, ratio: Optional[float] = None) -> PairMatches:
        """esfm_match_cross_pairs_dev: mutual nearest neighbours of every pair (ratio=None), or ratio+cross (Lowe's test in both
        directions as well).  Enqueues; does not synchronise."""
        return self._lists(lib().esfm_match_cross_pairs_dev, *_cross_args(ratio))

    def _guided_call(self, fn, pair_indices, E, K4, max_epipolar_px, filt, alloc):
        """fn(ctx, metric, bank, keypoints, row_offset, n_sets, width, sub-list, n, E, K4, max_epipolar_px, *filt, *outputs, offset) on
        self.pairs[pair_indices]; alloc(total queries, pairs) makes the output tensors.  Returns (sub-list, offset, outputs)."""
        b = self.bank
        if b.keypoints is None:
            raise ValueError("guided matching needs a DescriptorBank built with keypoints")
        sub = np.ascontiguousarray(self.pairs[np.asarray(pair_indices, np.int64)], np.int32).reshape(-1, 2)
        E, K4 = _geometry(E, K4, len(sub))
        offset = np.zeros(len(sub) + 1, np.int64)
        outs = alloc(max(int(b.rows[sub[:, 0]].sum()) if len(sub) else 0, 1), max(len(sub), 1))
        check(fn(self.ctx.handle, b.metric, C.c_void_p(b.data.data_ptr()), C.c_void_p(b.keypoints.data_ptr()), _ptr(b.row_offset), b.n_sets, b.width,
                 _ptr(sub), len(sub), _ptr(E), _ptr(K4), float(max_epipolar_px), *filt, *(C.c_void_p(o.data_ptr()) for o in outs), _ptr(offset)))
        return sub, offset, outs

    def match_guided(self, pair_indices, E, K4, max_epipolar_px: float, ratio: Optional[float], cross_check: bool = False) -> PairMatches:
        """esfm_match_guided_pairs_dev on self.pairs[pair_indices]: E [n, 3, 3] and K4 [n, 4] (fx, cx, fy, cy) per listed pair.  The
        result has buffers of its own (this matcher's match() outputs stay as they are).  Enqueues; does not synchronise."""
        torch, dev = self.torch, self.bank.device

        def alloc(total, n_pairs):
            return (torch.empty(total, dtype=torch.int32, device=dev), torch.empty(total, dtype=torch.int32, device=dev),
                    torch.empty(total, dtype=torch.float32, device=dev), torch.empty(n_pairs, dtype=torch.int32, device=dev))
        sub, offset, (qi, ti, d, n_out) = self._guided_call(lib().esfm_match_guided_pairs_dev, pair_indices, E, K4, max_epipolar_px,
                                                            _guided_args(ratio, cross_check), alloc)
        return PairMatches(sub, offset, n_out, qi, ti, d, self.ctx)

    def knn2_guided(self, pair_indices, E, K4, max_epipolar_px: float):
        """esfm_knn2_guided_pairs_dev: (idx [sum nq, 2], dist [sum nq, 2], n_adm [sum nq]) device tensors and the host offsets."""
        torch, dev = self.torch, self.bank.device

        def alloc(total, n_pairs):
            return (torch.empty((total, 2), dtype=torch.int32, device=dev), torch.empty((total, 2), dtype=torch.float32, device=dev),
                    torch.empty(total, dtype=torch.int32, device=dev))
        _, offset, (idx, dist, n_adm) = self._guided_call(lib().esfm_knn2_guided_pairs_dev, pair_indices, E, K4, max_epipolar_px, (), alloc)
        return idx, dist, n_adm, offset

    def _tables(self):
        torch = self.torch
        shape = (max(self.total_queries, 1), 2)
        return (torch.empty(shape, dtype=torch.int32, device=self.bank.device), torch.empty(shape, dtype=torch.float32, device=self.bank.device))

    def knn2(self):
        """Raw 2-NN table of every pair: (idx[sum nq, 2], dist[sum nq, 2]) device tensors."""
        if self.knn_idx is None:
            self.knn_idx, self.knn_dist = self._tables()
        self._call(lib().esfm_knn2_pairs_dev, C.c_void_p(self.knn_idx.data_ptr()), C.c_void_p(self.knn_dist.data_ptr()))
        return self.knn_idx, self.knn_dist

    def knn2_screened(self, ratio: float):
        """Hamming only (esfm_knn2_pairs_screened_dev): the raw table of a pass that screens with `ratio` -- train index -2 marks
        the queries it dropped as unable to pass d0 < ratio d1."""
        idx, dist = self._tables()
        self._call(lib().esfm_knn2_pairs_screened_dev, float(ratio), C.c_void_p(idx.data_ptr()), C.c_void_p(dist.data_ptr()))
        return idx, dist

    def set_l2_audit(self, mode: int) -> None:
        """Certificate audit (tests): 0 product path, 1 skip the exact re-scan, 2 brute-force every query, 3 the one-product pass alone (esfm.h)."""
        check(lib().esfm_ctx_set_l2_audit(self.ctx.handle, int(mode)))

    def set_l2_two_launch(self, enable: bool) -> None:
        """esfm_ctx_set_l2_two_launch: run the 64-float match-list path's distance pass and finish stages as two launches instead of one (same results; A/B measurements, tests)."""
        check(lib().esfm_ctx_set_l2_two_launch(self.ctx.handle, 1 if enable else 0))

    def flagged(self) -> np.ndarray:
        """(pair index, query row) of the queries the last L2 call could not certify; synchronises."""
        n = C.c_int64(0)
        check(lib().esfm_match_last_flagged(self.ctx.handle, None, 0, C.byref(n)))
        out = np.zeros((max(n.value, 1), 2), np.int32)
        check(lib().esfm_match_last_flagged(self.ctx.handle, _ptr(out), n.value, C.byref(n)))
        return out[:n.value].copy()

    def stats(self) -> Tuple[int, int]:
        """(queries, queries re-scanned exactly) of the last L2 call; synchronises."""
        a = C.c_int64(0); b = C.c_int64(0)
        check(lib().esfm_match_last_stats(self.ctx.handle, C.byref(a), C.byref(b)))
        return a.value, b.value


    def second_pass(self) -> int:
        """Queries of the last L2 call the one-product bf16 pass could not certify and handed to the threshold-filter stage of l2_finish_kernel (64-float descriptors); synchronises."""
        a = C.c_int64(0)
        check(lib().esfm_match_last_second_pass(self.ctx.handle, C.byref(a)))
        return a.value

def shard_pair_list(n_frames: int, rows_per_frame: Optional[np.ndarray], rank: int, world: int) -> np.ndarray:
    """This rank's share of the (i, j<i) pair list (host-only, no GPU)."""
    cap = n_frames * (n_frames - 1) // 2
    out = np.zeros((max(cap, 1), 2), np.int32)
    rows = None if rows_per_frame is None else np.ascontiguousarray(rows_per_frame, np.int32)
    n = lib().esfm_shard_pair_list(int(n_frames), _ptr(rows) if rows is not None else None, int(rank), int(world), _ptr(out))
    if n < 0:
        check(n)
    return out[:n].copy()
