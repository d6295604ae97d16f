"""ctypes loader of tests/sift_ref/sift_ref.c, the CPU restatement of esfm_sift_detect_and_compute (test infrastructure).

The C file is compiled with the oracle's flags into a directory the caller names (a pytest temporary directory), in a child
process; nothing is written into the tree."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "sift_ref", "sift_ref.c")
CFLAGS = ["-O3", "-march=x86-64-v3", "-fPIC", "-std=c11", "-ffp-contract=off", "-fno-fast-math", "-Wall"]


class SiftRef:
    def __init__(self, out_dir: str):
        so = os.path.join(str(out_dir), "libsift_ref.so")
        r = subprocess.run([os.environ.get("CC", "gcc"), *CFLAGS, "-shared", "-o", so, SRC, "-lm"],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError("sift_ref.c failed to build:\n" + r.stdout)
        L = C.CDLL(so)
        vp, f32 = C.c_void_p, C.c_float
        L.sift_ref_taps.argtypes = [C.c_double, vp]
        L.sift_ref_sigmas.argtypes = [vp]
        L.sift_ref_n_octaves.argtypes = [C.c_int, C.c_int]
        L.sift_ref_bgr2gray.argtypes = [vp, C.c_int, vp]
        L.sift_ref_pyramid.argtypes = [vp, C.c_int, C.c_int, vp]
        L.sift_ref_detect.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.POINTER(f32)), C.POINTER(C.POINTER(f32))]
        L.sift_ref_free.argtypes = [vp]
        for name in ("sift_exp", "sift_exp2", "sift_sin", "sift_cos"):
            getattr(L, name).argtypes = [f32]
            getattr(L, name).restype = f32
        self.L = L

    def taps(self, sigma: float) -> np.ndarray:
        out = np.zeros(128, np.float32)
        n = self.L.sift_ref_taps(float(sigma), out.ctypes.data)
        return out[:n].copy()

    def sigmas(self) -> np.ndarray:
        out = np.zeros(6, np.float64)
        self.L.sift_ref_sigmas(out.ctypes.data)
        return out

    def octave_shapes(self, rows: int, cols: int):
        n = self.L.sift_ref_n_octaves(rows, cols)
        shapes, r, c = [], 2 * rows, 2 * cols
        for _ in range(n):
            shapes.append((r, c))
            r, c = r // 2, c // 2
        return shapes

    def gray(self, image) -> np.ndarray:
        img = np.ascontiguousarray(image, np.uint8)
        if img.ndim == 2:
            return img
        out = np.empty(img.shape[:2], np.uint8)
        self.L.sift_ref_bgr2gray(img.ctypes.data, img.shape[0] * img.shape[1], out.ctypes.data)
        return out

    def pyramid(self, gray):
        """[octave][layer] float32 Gaussian layers."""
        g = np.ascontiguousarray(gray, np.uint8)
        shapes = self.octave_shapes(*g.shape)
        flat = np.zeros(sum(6 * r * c for r, c in shapes), np.float32)
        self.L.sift_ref_pyramid(g.ctypes.data, g.shape[0], g.shape[1], flat.ctypes.data)
        out, off = [], 0
        for r, c in shapes:
            layers = []
            for _ in range(6):
                layers.append(flat[off:off + r * c].reshape(r, c)); off += r * c
            out.append(layers)
        return out

    def detect(self, image, nfeatures: int = 0, max_keypoints=None):
        """(keypoints [n, 7], descriptors [n, 128]) float32, as esfm_sift_detect_and_compute returns them."""
        g = self.gray(image)
        kp, de = C.POINTER(C.c_float)(), C.POINTER(C.c_float)()
        n = self.L.sift_ref_detect(g.ctypes.data, g.shape[0], g.shape[1], int(nfeatures), -1 if max_keypoints is None else int(max_keypoints),
                                   C.byref(kp), C.byref(de))
        k = np.ctypeslib.as_array(kp, shape=(max(n, 1) * 7,))[:n * 7].reshape(n, 7).copy()
        d = np.ctypeslib.as_array(de, shape=(max(n, 1) * 128,))[:n * 128].reshape(n, 128).copy()
        self.L.sift_ref_free(C.cast(kp, C.c_void_p)); self.L.sift_ref_free(C.cast(de, C.c_void_p))
        return k, d

    def fn(self, name: str, x: np.ndarray) -> np.ndarray:
        f = getattr(self.L, name)
        return np.array([f(float(v)) for v in np.asarray(x, np.float32)], np.float32)
