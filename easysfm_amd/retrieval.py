"""Image retrieval for pair selection (include/esfm.h "Image retrieval"): one int8 VLAD descriptor per image over a k-means
codebook trained on the run's own local descriptors, an all-images similarity table, the ``top_k`` nearest images of each image,
and from that table (plus an optional window of preceding images) the pair list the match entry points take.

``select_pairs`` runs the whole chain on the GPU; ``retrieval_train`` / ``retrieval_vlad`` / ``retrieval_rank`` are its stages, each
callable on its own; ``retrieval_pair_list`` is host code.  The defaults -- 64 centres, 10 nearest images -- are conventions of
VLAD retrieval and have not been tuned on this project's data."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np

from ._lib import ESFM_L2_F32, Context, RetrievalOptionsStruct, check, default_context, lib


class RetrievalOptions:
    """esfm_retrieval_options."""

    def __init__(self, n_centres: int = 64, kmeans_iterations: int = 10, max_train: int = 65536, top_k: int = 10, window: int = 0):
        self.n_centres = int(n_centres)
        self.kmeans_iterations = int(kmeans_iterations)
        self.max_train = int(max_train)
        self.top_k = int(top_k)
        self.window = int(window)

    def struct(self) -> RetrievalOptionsStruct:
        return RetrievalOptionsStruct(self.n_centres, self.kmeans_iterations, self.max_train, self.top_k, self.window, 0)


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else C.c_void_p(a.ctypes.data)


def working_dim(metric: int, width: int) -> int:
    """d of the rule list: the width of float rows, eight times that of binary rows."""
    return int(width) if metric == ESFM_L2_F32 else 8 * int(width)


def _rows(sets: Sequence[np.ndarray], metric: int):
    """(rows back to back, set_row_offset, width) of a list of descriptor arrays."""
    dt = np.float32 if metric == ESFM_L2_F32 else np.uint8
    sets = [np.ascontiguousarray(s, dt) for s in sets]
    if any(s.ndim != 2 for s in sets):
        raise ValueError("descriptors must be 2-D arrays [rows, width]")
    widths = {s.shape[1] for s in sets}
    if len(widths) != 1:
        raise ValueError("all descriptor sets must have the same width")
    width = widths.pop()
    off = np.zeros(len(sets) + 1, np.int32)
    np.cumsum([s.shape[0] for s in sets], out=off[1:])
    bank = np.ascontiguousarray(np.concatenate(sets, axis=0)) if off[-1] else np.zeros((1, width), dt)
    return bank, off, width


def _pair_capacity(n_sets: int, top_k: int, window: int) -> int:
    return max(n_sets * (max(top_k, 0) + min(max(window, 0), max(n_sets - 1, 0))), 1)


def retrieval_train(sets: Sequence[np.ndarray], metric: int = ESFM_L2_F32, options: Optional[RetrievalOptions] = None,
                    ctx: Optional[Context] = None) -> np.ndarray:
    """esfm_retrieval_train: the codebook, float32 [n_centres, d]."""
    ctx = ctx or default_context()
    o = options or RetrievalOptions()
    bank, off, width = _rows(sets, metric)
    centres = np.zeros((max(o.n_centres, 1), working_dim(metric, width)), np.float32)
    check(lib().esfm_retrieval_train(ctx.handle, metric, _ptr(bank), _ptr(off), len(sets), width, C.byref(o.struct()), _ptr(centres)))
    return centres


def retrieval_vlad(sets: Sequence[np.ndarray], centres: np.ndarray, metric: int = ESFM_L2_F32, ctx: Optional[Context] = None,
                   debug: bool = False):
    """esfm_retrieval_vlad: (vlad int8 [n_sets, D], norm2 int32 [n_sets]); with debug also (assign int32 [rows], S int64 [n_sets, D])."""
    ctx = ctx or default_context()
    bank, off, width = _rows(sets, metric)
    centres = np.ascontiguousarray(centres, np.float32)
    d = working_dim(metric, width)
    if centres.ndim != 2 or centres.shape[1] != d:
        raise ValueError(f"centres must be [n_centres, {d}]")
    n, D = len(sets), centres.shape[0] * d
    vlad = np.zeros((n, D), np.int8); norm2 = np.zeros(n, np.int32)
    assign = np.zeros(int(off[-1]), np.int32) if debug else None
    sums = np.zeros((n, D), np.int64) if debug else None
    check(lib().esfm_retrieval_vlad(ctx.handle, metric, _ptr(bank), _ptr(off), n, width, centres.shape[0], _ptr(centres), _ptr(vlad), _ptr(norm2),
                                    _ptr(assign), _ptr(sums)))
    return (vlad, norm2, assign, sums) if debug else (vlad, norm2)


def retrieval_rank(vlad: np.ndarray, top_k: int, ctx: Optional[Context] = None, debug: bool = False):
    """esfm_retrieval_rank: nearest int32 [n_sets, top_k] (-1 padded); with debug also (dots int32 [n, n], scores float64 [n, n])."""
    ctx = ctx or default_context()
    vlad = np.ascontiguousarray(vlad, np.int8)
    if vlad.ndim != 2:
        raise ValueError("vlad must be [n_sets, D]")
    n, D = vlad.shape
    nearest = np.full((n, max(int(top_k), 0)), -1, np.int32)
    dots = np.zeros((n, n), np.int32) if debug else None
    scores = np.zeros((n, n), np.float64) if debug else None
    check(lib().esfm_retrieval_rank(ctx.handle, n, D, _ptr(vlad), int(top_k), _ptr(nearest), _ptr(dots), _ptr(scores)))
    return (nearest, dots, scores) if debug else nearest


def retrieval_pair_list(nearest: Optional[np.ndarray], n_sets: int, window: int = 0) -> np.ndarray:
    """esfm_retrieval_pair_list (host only): the int32 [P, 2] list of (i, j < i) pairs the table and the window select."""
    top_k = 0
    if nearest is not None:
        nearest = np.ascontiguousarray(nearest, np.int32).reshape(int(n_sets), -1) if int(n_sets) else np.zeros((0, 0), np.int32)
        top_k = nearest.shape[1]
    pairs = np.zeros((_pair_capacity(int(n_sets), top_k, int(window)), 2), np.int32)
    n = C.c_int32(0)
    check(lib().esfm_retrieval_pair_list(int(n_sets), top_k, _ptr(nearest) if top_k else None, int(window), _ptr(pairs), C.byref(n)))
    return pairs[:n.value].copy()


def select_pairs(sets_or_bank, metric: int = ESFM_L2_F32, options: Optional[RetrievalOptions] = None, ctx: Optional[Context] = None) -> np.ndarray:
    """The whole chain: int32 [P, 2] pairs (i, j < i), ascending.  `sets_or_bank`: a list of descriptor arrays
    (esfm_retrieval_pairs: uploaded once) or a matching.DescriptorBank, whose resident rows are used as they are
    (esfm_retrieval_pairs_dev; `metric` is then the bank's)."""
    ctx = ctx or default_context()
    o = options or RetrievalOptions()
    n = C.c_int32(0)
    if hasattr(sets_or_bank, "row_offset"):
        import torch
        bank = sets_or_bank
        pairs = np.zeros((_pair_capacity(bank.n_sets, o.top_k, o.window), 2), np.int32)
        torch.cuda.synchronize(bank.device)          # the bank's upload ran on torch's stream
        check(lib().esfm_retrieval_pairs_dev(ctx.handle, bank.metric, C.c_void_p(bank.data.data_ptr()), _ptr(bank.row_offset), bank.n_sets, bank.width,
                                             C.byref(o.struct()), _ptr(pairs), C.byref(n)))
    else:
        rows, off, width = _rows(sets_or_bank, metric)
        pairs = np.zeros((_pair_capacity(len(sets_or_bank), o.top_k, o.window), 2), np.int32)
        check(lib().esfm_retrieval_pairs(ctx.handle, metric, _ptr(rows), _ptr(off), len(sets_or_bank), width, C.byref(o.struct()), _ptr(pairs),
                                         C.byref(n)))
    return pairs[:n.value].copy()


def last_stage_ms(ctx: Optional[Context] = None) -> Tuple[float, float, float, float]:
    """esfm_retrieval_last_stage_ms: under Context.set_kernel_timing(True), the device time in ms of the last select_pairs call's
    stages (codebook training, assignment + accumulation, finalise, similarity + ranking)."""
    ctx = ctx or default_context()
    ms = (C.c_double * 4)()
    check(lib().esfm_retrieval_last_stage_ms(ctx.handle, ms))
    return tuple(ms)
