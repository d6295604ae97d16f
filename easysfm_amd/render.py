"""Mesh rendering (include/esfm.h, "Mesh rendering"): esfm_mesh_render draws an indexed triangle mesh into views -- per pixel the
owning triangle, its depth and its colour from the texture atlas, the vertex colours or plain grey --, mesh_render_error compares
such pictures with the photographs the views took, and orbit_poses makes preview cameras around a mesh."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from ._lib import Context, MeshRenderOptions, check, default_context, lib
from .mesh import _cameras, _ptr, _triangle_array


def default_mesh_render_options() -> MeshRenderOptions:
    """esfm_mesh_render_options_default: background (0, 0, 0)."""
    opt = MeshRenderOptions()
    lib().esfm_mesh_render_options_default(C.byref(opt))
    return opt


def mesh_render(vertices, triangles, K4, poses, rows: int, cols: int, vertex_rgb=None, uv=None, atlas=None,
                options: Optional[MeshRenderOptions] = None, ctx: Optional[Context] = None, outputs=("rgb", "depth", "triangle_id")):
    """esfm_mesh_render on vertices [V, 3] float32 and triangles [T, 3] int32 under n views of rows x cols pixels (K4 [n, 4], poses
    [n, 12] or [n, 3 | 4, 4]).  Colour comes from uv [T, 3, 2] float32 with atlas [H, W, 3] uint8 RGB (mesh_texture_bake's), else
    from vertex_rgb [V, 3] uint8, else it is grey.  Returns (rgb [n, rows, cols, 3] uint8 RGB, depth [n, rows, cols] float32,
    triangle_id [n, rows, cols] int32); background pixels hold options.background, depth 0 and id -1.  An output not named in
    `outputs` is not computed and comes back as None."""
    opt = options or default_mesh_render_options()
    ctx = ctx or default_context()
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    t = _triangle_array(triangles)
    c = np.ascontiguousarray(vertex_rgb, np.uint8).reshape(-1, 3) if vertex_rgb is not None else None
    if c is not None and len(c) != len(v):
        raise ValueError("vertex_rgb must hold one colour per vertex")
    K, P = _cameras(K4, poses)
    g = at = None
    H = W = 0
    if uv is not None:
        g = np.ascontiguousarray(uv, np.float32).reshape(-1, 3, 2)
        if len(g) != len(t):
            raise ValueError("uv must hold three corners per triangle")
        if len(g) == 0:
            g = np.zeros((1, 3, 2), np.float32)                          # (a pointer that is not NULL: uv and atlas go together)
    if atlas is not None:
        at = np.ascontiguousarray(atlas, np.uint8)
        if at.ndim != 3 or at.shape[2] != 3:
            raise ValueError("atlas must be [H, W, 3]")
        H, W = at.shape[:2]
    n, r, co = len(K), max(int(rows), 0), max(int(cols), 0)
    rgb = np.zeros((n, r, co, 3), np.uint8) if "rgb" in outputs else None
    depth = np.zeros((n, r, co), np.float32) if "depth" in outputs else None
    tid = np.zeros((n, r, co), np.int32) if "triangle_id" in outputs else None
    check(lib().esfm_mesh_render(ctx.handle, len(v), len(t), _ptr(v), _ptr(t), _ptr(c), _ptr(g), H, W, _ptr(at), n, int(rows), int(cols), _ptr(K), _ptr(P),
                                 C.byref(opt), _ptr(rgb), _ptr(depth), _ptr(tid)))
    return rgb, depth, tid


def mesh_render_error(rgb, triangle_id, images):
    """The re-render error of pictures rgb [n, rows, cols, 3] uint8 RGB with triangle_id [n, rows, cols] against the photographs
    `images` [n, rows, cols(, 1 | 3)] uint8 (BGR or grey, as the rest of the package takes them): per view (sum_abs int64: the sum of
    |picture - photograph| over the covered pixels -- triangle_id >= 0 -- and the three channels, covered: their number), two arrays
    of n.  Integer arithmetic on the host."""
    pic = np.asarray(rgb, np.uint8)
    tid = np.asarray(triangle_id)
    img = np.asarray(images, np.uint8)
    if img.ndim == 3:
        img = img[..., None]
    if pic.ndim != 4 or pic.shape[3] != 3 or tid.shape != pic.shape[:3] or img.shape[:3] != pic.shape[:3] or img.shape[3] not in (1, 3):
        raise ValueError("rgb [n, rows, cols, 3], triangle_id [n, rows, cols] and images [n, rows, cols(, 1 | 3)] must agree")
    photo = img[..., ::-1] if img.shape[3] == 3 else np.repeat(img, 3, axis=3)
    diff = np.abs(pic.astype(np.int64) - photo.astype(np.int64)).sum(axis=3)
    covered = tid >= 0
    return np.where(covered, diff, 0).sum(axis=(1, 2)).astype(np.int64), covered.sum(axis=(1, 2)).astype(np.int64)


def orbit_poses(vertices, n: int, elevation_deg: float = 20.0, distance: float = 2.5, up=(0.0, -1.0, 0.0)):
    """n preview poses [n, 12] float32 on a circle about the midpoint of the mesh's bounding box: the radius is `distance` times the
    box's half diagonal, the circle is raised by elevation_deg towards `up`, and every camera looks at the midpoint with `up` upwards
    in its picture.  Python only."""
    v = np.asarray(vertices, np.float64).reshape(-1, 3)
    if len(v) == 0 or n < 1:
        raise ValueError("orbit_poses needs vertices and n >= 1")
    lo, hi = v.min(axis=0), v.max(axis=0)
    mid, radius = (lo + hi) / 2.0, float(distance) * max(np.linalg.norm(hi - lo) / 2.0, 1e-12)
    upv = np.asarray(up, np.float64) / np.linalg.norm(up)
    a = np.cross(upv, [0.0, 0.0, 1.0] if abs(upv[2]) < 0.9 else [1.0, 0.0, 0.0])
    a /= np.linalg.norm(a)
    b = np.cross(upv, a)
    el = np.deg2rad(elevation_deg)
    if abs(np.cos(el)) < 1e-6:
        raise ValueError("elevation_deg must stay away from +-90")
    poses = np.zeros((n, 12), np.float32)
    for i in range(n):
        phi = 2.0 * np.pi * i / n
        centre = mid + radius * (np.cos(el) * (np.cos(phi) * a + np.sin(phi) * b) + np.sin(el) * upv)
        z = (mid - centre) / np.linalg.norm(mid - centre)
        x = np.cross(-upv, z)
        x /= np.linalg.norm(x)
        R = np.stack([x, np.cross(z, x), z])
        poses[i] = np.concatenate([R, (-R @ centre)[:, None]], axis=1).reshape(12)
    return poses


__all__ = ["MeshRenderOptions", "default_mesh_render_options", "mesh_render", "mesh_render_error", "orbit_poses"]
