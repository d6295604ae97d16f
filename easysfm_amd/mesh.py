"""Surface reconstruction over the C ABI (include/esfm.h, "Surface reconstruction"): depth maps into a truncated signed
distance volume (``tsdf_integrate``), an indexed triangle mesh out of it by marching tetrahedra (``tsdf_extract``), and both
with the volume staying on the device (``mvs_mesh``).  ``dense_mesh`` takes what the pipeline holds after its final bundle
adjustment, as ``mvs.dense_merge`` does, and ends in a mesh instead of a point cloud.  ``mesh_components`` and ``mesh_clean``
(esfm.h, "Mesh clean-up") label a mesh's connected pieces, drop the small ones, smooth the rest and recompute its normals;
``mesh_simplify`` (esfm.h, "Mesh simplification") merges the vertices of each cell of a regular grid into one;
``mesh_texture`` (esfm.h, "Mesh texturing") lets every triangle choose the view that sees it best and bakes a texture atlas;
``mesh_texture_level`` solves for per-vertex colour offsets that take the steps out of the seams between views."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Tuple

import numpy as np

from ._lib import (Context, MeshCleanOptions, MeshSimplifyOptions, MeshTextureLevelOptions, MeshTextureLevelStats, MeshTextureOptions, MVSOptions,
                   TSDFGrid, TSDFOptions, check, default_context, lib)
from .mvs import MergeOptions, _views, default_mvs_options, frame_arrays, merge_voxel_size, mvs_depth_maps, mvs_fuse, mvs_plan
from .types import Frame, SparsePointCloud

MAX_VIEWS = 64
MAX_DIM = 1024
CAPACITY_GUESS = (1 << 18, 1 << 19)      # vertices, triangles of a first attempt


def default_tsdf_options() -> TSDFOptions:
    """esfm_tsdf_options_default: trunc 0 (= 4 voxels), min_weight 2."""
    opt = TSDFOptions()
    lib().esfm_tsdf_options_default(C.byref(opt))
    return opt


def _ptr(a) -> Optional[C.c_void_p]:
    return C.c_void_p(a.ctypes.data) if a is not None else None


def tsdf_grid(origin, voxel_size: float, dims) -> TSDFGrid:
    """esfm_tsdf_grid of dims = (nx, ny, nz) voxels of side voxel_size whose first corner is origin."""
    g = TSDFGrid()
    g.origin[:] = [float(v) for v in origin]
    g.voxel_size = float(voxel_size)
    g.dims[:] = [int(v) for v in dims]
    return g


def _view_arrays(images, K4, poses, depth):
    d = np.ascontiguousarray(depth, np.float32)
    if d.ndim != 3:
        raise ValueError("depth must be [n_views, rows, cols]")
    n, rows, cols = d.shape
    if images is None:
        K = np.ascontiguousarray(np.asarray(K4, np.float32).reshape(n, 4))
        P = np.ascontiguousarray(np.asarray(poses, np.float32).reshape(n, -1, 4)[:, :3, :].reshape(n, 12))
        return None, K, P, d, 1
    imgs, K, P = _views(images, K4, poses)
    if imgs.shape[:3] != d.shape:
        raise ValueError("images and depth must share [n_views, rows, cols]")
    return imgs, K, P, d, imgs.shape[3]


def tsdf_integrate(images, K4, poses, depth, grid: TSDFGrid, opt: Optional[TSDFOptions] = None, ctx: Optional[Context] = None):
    """esfm_tsdf_integrate.  images [n, rows, cols(, 1 | 3)] uint8 or None, K4 [n, 4], poses [n, 12] (or [n, 3 | 4, 4]), depth
    [n, rows, cols] float32 (0 = none).  Returns (tsdf [nz, ny, nx] float32, weight [nz, ny, nx] int32, rgb [nz, ny, nx, 3] uint8
    or None without images)."""
    opt = opt or default_tsdf_options()
    ctx = ctx or default_context()
    imgs, K, P, d, ch = _view_arrays(images, K4, poses, depth)
    n, rows, cols = d.shape
    shape = (int(grid.dims[2]), int(grid.dims[1]), int(grid.dims[0]))
    if min(shape) < 0 or shape[0] * shape[1] * shape[2] > 2 ** 27:
        shape = (0, 0, 0)                                         # (the call rejects the grid; nothing is written)
    tsdf = np.zeros(shape, np.float32)
    weight = np.zeros(shape, np.int32)
    rgb = np.zeros(shape + (3,), np.uint8) if imgs is not None else None
    check(lib().esfm_tsdf_integrate(ctx.handle, n, rows, cols, ch, _ptr(imgs), _ptr(K), _ptr(P), _ptr(d), C.byref(grid), C.byref(opt),
                                    _ptr(tsdf), _ptr(weight), _ptr(rgb)))
    return tsdf, weight, rgb


def _with_capacities(call, want_normals: bool, want_rgb: bool, capacity: Optional[Tuple[int, int]]):
    """Runs `call(max_v, max_t, vertices, normals, rgb, triangles, n_v, n_t)` with guessed capacities and, if the mesh does not
    fit, once more with the counts the first call reported."""
    cap_v, cap_t = capacity if capacity is not None else CAPACITY_GUESS
    for attempt in range(2):
        vertices = np.zeros((max(cap_v, 1), 3), np.float32)
        normals = np.zeros((max(cap_v, 1), 3), np.float32) if want_normals else None
        rgb = np.zeros((max(cap_v, 1), 3), np.uint8) if want_rgb else None
        triangles = np.zeros((max(cap_t, 1), 3), np.int32)
        nv, nt = C.c_int32(-1), C.c_int32(-1)
        status = call(cap_v, cap_t, vertices, normals, rgb, triangles, nv, nt)
        too_small = status == -1 and (nv.value > cap_v or nt.value > cap_t)
        if too_small and attempt == 0 and capacity is None:
            cap_v, cap_t = nv.value, nt.value
            continue
        check(status)
        cut = lambda a, m: None if a is None else a[:m].copy()
        return cut(vertices, nv.value), cut(normals, nv.value), cut(rgb, nv.value), cut(triangles, nt.value)
    raise AssertionError("unreachable")


def tsdf_extract(tsdf, weight, rgb, grid: TSDFGrid, opt: Optional[TSDFOptions] = None, ctx: Optional[Context] = None,
                 normals: bool = True, colours: bool = True, capacity: Optional[Tuple[int, int]] = None):
    """esfm_tsdf_extract on a volume as tsdf_integrate returns it (rgb may be None).  Returns (vertices [V, 3] float32, normals
    [V, 3] float32 or None, vertex_rgb [V, 3] uint8 or None, triangles [T, 3] int32).  capacity = (max_vertices, max_triangles)
    is passed as given (too small: EsfmError with both counts); None guesses and retries once with the reported counts."""
    opt = opt or default_tsdf_options()
    ctx = ctx or default_context()
    n_vox = int(grid.dims[0]) * int(grid.dims[1]) * int(grid.dims[2])
    f = np.ascontiguousarray(tsdf, np.float32)
    w = np.ascontiguousarray(weight, np.int32)
    c = np.ascontiguousarray(rgb, np.uint8) if rgb is not None else None
    if f.size != n_vox or w.size != n_vox or (c is not None and c.size != 3 * n_vox):
        raise ValueError("the volume arrays do not match the grid")

    def call(cap_v, cap_t, vertices, nrm, col, triangles, nv, nt):
        return lib().esfm_tsdf_extract(ctx.handle, C.byref(grid), _ptr(f), _ptr(w), _ptr(c), C.byref(opt), cap_v, cap_t, _ptr(vertices),
                                       _ptr(nrm), _ptr(col), _ptr(triangles), C.byref(nv), C.byref(nt))
    return _with_capacities(call, normals, colours and c is not None, capacity)


def mvs_mesh(images, K4, poses, depth, grid: TSDFGrid, opt: Optional[TSDFOptions] = None, ctx: Optional[Context] = None,
             normals: bool = True, colours: bool = True, capacity: Optional[Tuple[int, int]] = None):
    """esfm_mvs_mesh: tsdf_integrate and tsdf_extract in one call, the volume never leaves the device.  Arguments as
    tsdf_integrate takes them, results as tsdf_extract returns them."""
    opt = opt or default_tsdf_options()
    ctx = ctx or default_context()
    imgs, K, P, d, ch = _view_arrays(images, K4, poses, depth)
    n, rows, cols = d.shape

    def call(cap_v, cap_t, vertices, nrm, col, triangles, nv, nt):
        return lib().esfm_mvs_mesh(ctx.handle, n, rows, cols, ch, _ptr(imgs), _ptr(K), _ptr(P), _ptr(d), C.byref(grid), C.byref(opt), cap_v,
                                   cap_t, _ptr(vertices), _ptr(nrm), _ptr(col), _ptr(triangles), C.byref(nv), C.byref(nt))
    return _with_capacities(call, normals, colours and imgs is not None, capacity)


class MeshOptions:
    """Settings of dense_mesh's volume.  voxel_size > 0 is used as given; 0 derives it as voxel_scale times the merge's median
    pixel footprint (mvs.merge_voxel_size).  The voxels are enlarged just enough for the grid to hold at most max_voxels and at
    most 1024 per axis.  trunc_voxels: the truncation distance in voxels; min_weight: views a voxel needs to be valid."""

    def __init__(self, voxel_size: float = 0.0, voxel_scale: float = 2.0, max_voxels: int = 2 ** 24, trunc_voxels: float = 4.0,
                 min_weight: int = 2):
        self.voxel_size, self.voxel_scale, self.max_voxels, self.trunc_voxels, self.min_weight = \
            voxel_size, voxel_scale, max_voxels, trunc_voxels, min_weight


def masked_depth(depth, pixel_index) -> np.ndarray:
    """The depth maps with every pixel the fusion did not keep set to 0 (pixel_index as mvs_fuse(return_index=True) gives it)."""
    d = np.asarray(depth, np.float32)
    out = np.zeros(d.size, np.float32)
    idx = np.asarray(pixel_index, np.int64)
    out[idx] = d.reshape(-1)[idx]
    return out.reshape(d.shape)


def mesh_grid(xyz, voxel_size: float, mesh_opt: MeshOptions) -> TSDFGrid:
    """The grid dense_mesh uses: the 1st..99th percentile box of the points per axis (sorted[floor(0.01 (n - 1))] and
    sorted[ceil(0.99 (n - 1))]) padded by the truncation distance; the voxel size is enlarged just enough for max_voxels and 1024
    voxels per axis."""
    pts = np.asarray(xyz, np.float64).reshape(-1, 3)
    pts = pts[np.all(np.isfinite(pts), axis=1)]
    if len(pts) == 0:
        raise ValueError("no points to place a grid around")
    s = np.sort(pts, axis=0)
    n1 = len(s) - 1
    lo, hi = s[int(np.floor(0.01 * n1))], s[int(np.ceil(0.99 * n1))]
    h = float(voxel_size)
    max_voxels = min(int(mesh_opt.max_voxels), 2 ** 27)

    def dims_of(h):
        pad = mesh_opt.trunc_voxels * h
        return np.maximum(np.ceil((hi - lo + 2 * pad) / h).astype(np.int64) + 1, 2)
    while True:
        dims = dims_of(h)
        if dims.max() <= MAX_DIM and int(dims[0]) * int(dims[1]) * int(dims[2]) <= max_voxels:
            break
        grow = max(dims.max() / MAX_DIM, (float(dims[0]) * float(dims[1]) * float(dims[2]) / max_voxels) ** (1.0 / 3.0))
        h *= max(grow, 1.0) * 1.001
    h = float(np.float32(h))
    dims = np.minimum(dims_of(h), MAX_DIM)
    origin = (lo + hi) / 2 - dims * h / 2
    return tsdf_grid(origin, h, dims)


def mesh_arrays(imgs, K4, poses, nb, depth, opt: MVSOptions, mesh_opt: MeshOptions, ctx: Context):
    """dense_mesh behind the depth maps (plain arrays).  Returns (vertices, normals, rgb, triangles, grid)."""
    if len(depth) > MAX_VIEWS:
        raise ValueError("dense_mesh integrates at most 64 views")
    xyz, _, index = mvs_fuse(imgs, K4, poses, nb, depth, opt, ctx, return_index=True)
    if len(xyz) == 0:
        raise ValueError("the fusion kept no point: nothing to mesh")
    h = merge_voxel_size(depth, K4, index, MergeOptions(voxel_size=mesh_opt.voxel_size, voxel_scale=mesh_opt.voxel_scale))
    grid = mesh_grid(xyz, float(h), mesh_opt)
    t_opt = default_tsdf_options()
    t_opt.trunc = float(np.float32(mesh_opt.trunc_voxels) * np.float32(grid.voxel_size))
    t_opt.min_weight = int(mesh_opt.min_weight)
    vertices, normals, rgb, triangles = mvs_mesh(imgs, K4, poses, masked_depth(depth, index), grid, t_opt, ctx)
    return vertices, normals, rgb, triangles, grid


def dense_mesh(frames: Sequence[Frame], process_frame_id: Sequence[bool], cloud: SparsePointCloud,
               opt: Optional[MVSOptions] = None, mesh_opt: Optional[MeshOptions] = None, ctx: Optional[Context] = None):
    """Plan, depth maps, fusion, and the mesh of the depth maps masked to the pixels the fusion kept (a single view's blunder
    never reaches the volume).  Returns (vertices [V, 3] float32, normals [V, 3] float32, rgb [V, 3] uint8, triangles [T, 3]
    int32, the esfm_tsdf_grid used)."""
    if len(frames) > MAX_VIEWS:
        raise ValueError("dense_mesh integrates at most 64 views")
    opt = opt or default_mvs_options()
    mesh_opt = mesh_opt or MeshOptions()
    ctx = ctx or default_context()
    imgs, K4, poses = frame_arrays(frames, process_frame_id)
    nb, rng = mvs_plan(frames, process_frame_id, cloud, opt)
    depth, _ = mvs_depth_maps(imgs, K4, poses, nb, rng, opt, ctx)
    return mesh_arrays(imgs, K4, poses, nb, depth, opt, mesh_opt, ctx)


def default_mesh_clean_options() -> MeshCleanOptions:
    """esfm_mesh_clean_options_default: components of at least 64 triangles and 1 % of the largest, 5 Taubin iterations with
    lambda 0.5 and mu -0.53, border vertices pinned."""
    opt = MeshCleanOptions()
    lib().esfm_mesh_clean_options_default(C.byref(opt))
    return opt


def _triangle_array(triangles) -> np.ndarray:
    t = np.ascontiguousarray(triangles, np.int32)
    if t.size % 3:
        raise ValueError("triangles must hold 3 indices each")
    return t.reshape(-1, 3)


def mesh_components(triangles, n_vertices: int, ctx: Optional[Context] = None):
    """esfm_mesh_components.  Returns (labels [V] int32: the smallest vertex index of each vertex's component, tri_count [V]
    int32: a component's triangle count at its label vertex and 0 elsewhere, the number of components)."""
    ctx = ctx or default_context()
    t = _triangle_array(triangles)
    labels = np.zeros(max(int(n_vertices), 0), np.int32)
    count = np.zeros(max(int(n_vertices), 0), np.int32)
    n = C.c_int32(0)
    check(lib().esfm_mesh_components(ctx.handle, int(n_vertices), len(t), _ptr(t), _ptr(labels), _ptr(count), C.byref(n)))
    return labels, count, n.value


def mesh_clean(vertices, rgb, triangles, opt: Optional[MeshCleanOptions] = None, ctx: Optional[Context] = None, return_maps: bool = False):
    """esfm_mesh_clean on vertices [V, 3] float32, rgb [V, 3] uint8 or None and triangles [T, 3] int32.  Returns (vertices,
    normals, rgb or None, triangles) of the cleaned mesh, and with return_maps also (vertex_map, triangle_map): the old index of
    every new vertex and triangle."""
    opt = opt or default_mesh_clean_options()
    ctx = ctx or default_context()
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    c = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3) if rgb is not None else None
    if c is not None and len(c) != len(v):
        raise ValueError("rgb must hold one colour per vertex")
    t = _triangle_array(triangles)
    out_v, out_n = np.zeros_like(v), np.zeros_like(v)
    out_c = np.zeros_like(c) if c is not None else None
    out_t = np.zeros_like(t)
    vmap = np.zeros(len(v), np.int32) if return_maps else None
    tmap = np.zeros(len(t), np.int32) if return_maps else None
    nv, nt = C.c_int32(0), C.c_int32(0)
    check(lib().esfm_mesh_clean(ctx.handle, len(v), len(t), _ptr(v), _ptr(c), _ptr(t), C.byref(opt), _ptr(out_v), _ptr(out_n), _ptr(out_c),
                                _ptr(out_t), _ptr(vmap), _ptr(tmap), C.byref(nv), C.byref(nt)))
    cut = lambda a, m: None if a is None else a[:m].copy()
    out = (cut(out_v, nv.value), cut(out_n, nv.value), cut(out_c, nv.value), cut(out_t, nt.value))
    return out + (cut(vmap, nv.value), cut(tmap, nt.value)) if return_maps else out


def default_mesh_simplify_options() -> MeshSimplifyOptions:
    """esfm_mesh_simplify_options_default: regularisation 1e-3, quadric placement on."""
    opt = MeshSimplifyOptions()
    lib().esfm_mesh_simplify_options_default(C.byref(opt))
    return opt


def mesh_simplify(vertices, rgb, triangles, cell: float, origin=None, opt: Optional[MeshSimplifyOptions] = None,
                  ctx: Optional[Context] = None, return_maps: bool = False):
    """esfm_mesh_simplify on vertices [V, 3] float32, rgb [V, 3] uint8 or None and triangles [T, 3] int32: all vertices of one
    grid cell of side `cell` (the grid starts at `origin`; None = the per-axis minimum of the vertices) become one.  Returns
    (vertices, normals, rgb or None, triangles) of the simplified mesh, and with return_maps also (vertex_map [V]: the new vertex
    of every old vertex or -1, triangle_map: the old index of every new triangle)."""
    opt = opt or default_mesh_simplify_options()
    ctx = ctx or default_context()
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    c = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3) if rgb is not None else None
    if c is not None and len(c) != len(v):
        raise ValueError("rgb must hold one colour per vertex")
    t = _triangle_array(triangles)
    if origin is None:
        origin = v.min(axis=0) if len(v) else np.zeros(3, np.float32)
    o = np.ascontiguousarray(origin, np.float32).reshape(3)
    out_v, out_n = np.zeros_like(v), np.zeros_like(v)
    out_c = np.zeros_like(c) if c is not None else None
    out_t = np.zeros_like(t)
    vmap = np.zeros(len(v), np.int32) if return_maps else None
    tmap = np.zeros(len(t), np.int32) if return_maps else None
    nv, nt = C.c_int32(0), C.c_int32(0)
    check(lib().esfm_mesh_simplify(ctx.handle, len(v), len(t), _ptr(v), _ptr(c), _ptr(t), _ptr(o), float(cell), C.byref(opt), _ptr(out_v),
                                   _ptr(out_n), _ptr(out_c), _ptr(out_t), _ptr(vmap), _ptr(tmap), C.byref(nv), C.byref(nt)))
    cut = lambda a, m: None if a is None else a[:m].copy()
    out = (cut(out_v, nv.value), cut(out_n, nv.value), cut(out_c, nv.value), cut(out_t, nt.value))
    return out + (vmap, cut(tmap, nt.value)) if return_maps else out


def default_mesh_texture_options() -> MeshTextureOptions:
    """esfm_mesh_texture_options_default: min_cos 0.2, occlusion_tol 0.02."""
    opt = MeshTextureOptions()
    lib().esfm_mesh_texture_options_default(C.byref(opt))
    return opt


def _cameras(K4, poses):
    K = np.ascontiguousarray(np.asarray(K4, np.float32).reshape(-1, 4))
    n = len(K)
    P = np.ascontiguousarray(np.asarray(poses, np.float32).reshape(n, -1, 4)[:, :3, :].reshape(n, 12))
    return K, P


def mesh_texture_views(vertices, triangles, rows: int, cols: int, K4, poses, opt: Optional[MeshTextureOptions] = None,
                       ctx: Optional[Context] = None, return_buffers: bool = False):
    """esfm_mesh_texture_views on vertices [V, 3] float32 and triangles [T, 3] int32 under n views of rows x cols pixels (K4 [n, 4],
    poses [n, 12] or [n, 3 | 4, 4]).  Returns (label [T] int32: the chosen view or -1, score [T] float32: half the triangle's
    screen area there in pixels), and with return_buffers also the views' buffers [n, rows, cols] uint32 (the bit pattern of the
    largest inverse depth at each pixel, 0 = nothing)."""
    opt = opt or default_mesh_texture_options()
    ctx = ctx or default_context()
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    t = _triangle_array(triangles)
    K, P = _cameras(K4, poses)
    label, score = np.full(len(t), -1, np.int32), np.zeros(len(t), np.float32)
    buffers = np.zeros((len(K), max(int(rows), 0), max(int(cols), 0)), np.uint32) if return_buffers else None
    check(lib().esfm_mesh_texture_views(ctx.handle, len(v), len(t), _ptr(v), _ptr(t), len(K), int(rows), int(cols), _ptr(K), _ptr(P),
                                        C.byref(opt), _ptr(label), _ptr(score), _ptr(buffers)))
    return (label, score, buffers) if return_buffers else (label, score)


def default_atlas_width(n_triangles: int) -> int:
    """ceil(sqrt(ceil(T / 2))) squares per atlas row, at least 1: a square atlas."""
    squares = (int(n_triangles) + 1) // 2
    a = int(np.ceil(np.sqrt(squares)))
    while a * a < squares:
        a += 1
    return max(a, 1)


def default_mesh_texture_level_options() -> MeshTextureLevelOptions:
    """esfm_mesh_texture_level_options_default: lam (lambda) 0.1, mu 0.001, tolerance 1e-4, max_iterations 200."""
    opt = MeshTextureLevelOptions()
    lib().esfm_mesh_texture_level_options_default(C.byref(opt))
    return opt


def _image_array(images):
    imgs = np.ascontiguousarray(images, np.uint8)
    if imgs.ndim == 3:
        imgs = imgs[..., None]
    if imgs.ndim != 4:
        raise ValueError("images must be [n_views, rows, cols(, channels)]")
    return imgs


def mesh_texture_level(vertices, triangles, label, images, K4, poses, opt: Optional[MeshTextureLevelOptions] = None,
                       ctx: Optional[Context] = None):
    """esfm_mesh_texture_level: one additive colour offset per (vertex, view) such that the views agree where triangles of
    different labels meet.  Returns (offsets [T, 3, 3] float32: corner x RGB, for mesh_texture_bake(offsets=...), samples [T, 3, 3]
    float32: the unrounded image values at the corners, stats: MeshTextureLevelStats with nodes, seam_vertices, iterations,
    converged)."""
    opt = opt or default_mesh_texture_level_options()
    ctx = ctx or default_context()
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    t = _triangle_array(triangles)
    lab = np.ascontiguousarray(label, np.int32).reshape(-1)
    if len(lab) != len(t):
        raise ValueError("label must hold one view per triangle")
    imgs = _image_array(images)
    n, rows, cols, ch = imgs.shape
    K, P = _cameras(K4, poses)
    if len(K) != n:
        raise ValueError("one K4 and one pose per image")
    offsets, samples = np.zeros((len(t), 3, 3), np.float32), np.zeros((len(t), 3, 3), np.float32)
    stats = MeshTextureLevelStats()
    check(lib().esfm_mesh_texture_level(ctx.handle, len(v), len(t), _ptr(v), _ptr(t), _ptr(lab), n, rows, cols, ch, _ptr(imgs), _ptr(K), _ptr(P),
                                        C.byref(opt), _ptr(offsets), _ptr(samples), C.byref(stats)))
    return offsets, samples, stats


def mesh_texture_bake(vertices, rgb, triangles, label, images, K4, poses, texels: int, atlas_width: Optional[int] = None,
                      ctx: Optional[Context] = None, offsets=None):
    """esfm_mesh_texture_bake, or with offsets [T, 3, 3] float32 (mesh_texture_level's) esfm_mesh_texture_bake_ex: every triangle gets a chart of `texels` x `texels` / 2 texels, two per square and `atlas_width`
    squares per atlas row (None = a square atlas), filled from the view label[t] names (images [n, rows, cols(, 1 | 3)] uint8, BGR)
    or, for label -1, from the vertex colours (grey without them).  Returns (atlas [H, W, 3] uint8 RGB, uv [T, 3, 2] float32,
    normalised, origin at the outer corner of the atlas's first texel, v down the rows)."""
    ctx = ctx or default_context()
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    c = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3) if rgb is not None else None
    if c is not None and len(c) != len(v):
        raise ValueError("rgb must hold one colour per vertex")
    t = _triangle_array(triangles)
    lab = np.ascontiguousarray(label, np.int32).reshape(-1)
    if len(lab) != len(t):
        raise ValueError("label must hold one view per triangle")
    imgs = np.ascontiguousarray(images, np.uint8)
    if imgs.ndim == 3:
        imgs = imgs[..., None]
    if imgs.ndim != 4:
        raise ValueError("images must be [n_views, rows, cols(, channels)]")
    n, rows, cols, ch = imgs.shape
    K, P = _cameras(K4, poses)
    if len(K) != n:
        raise ValueError("one K4 and one pose per image")
    width = default_atlas_width(len(t)) if atlas_width is None else int(atlas_width)
    off = np.ascontiguousarray(offsets, np.float32).reshape(-1, 3, 3) if offsets is not None else None
    if off is not None and len(off) != len(t):
        raise ValueError("offsets must hold three corners of three channels per triangle")
    uv = np.zeros((len(t), 3, 2), np.float32)
    need = C.c_int32(-1)
    cap = 0
    atlas = np.zeros((0, 0, 3), np.uint8)
    for attempt in range(2):                                            # the first call asks for the height, the second bakes
        args = (ctx.handle, len(v), len(t), _ptr(v), _ptr(c), _ptr(t), _ptr(lab), n, rows, cols, ch, _ptr(imgs), _ptr(K), _ptr(P), int(texels), width,
                cap, _ptr(atlas) if cap else None, _ptr(uv), C.byref(need))
        status = lib().esfm_mesh_texture_bake(*args) if off is None else lib().esfm_mesh_texture_bake_ex(*args, _ptr(off))
        if attempt == 0 and status == -1 and need.value > cap:
            cap = need.value
            atlas = np.zeros((cap, width * int(texels), 3), np.uint8)
            continue
        check(status)
        break
    return atlas.reshape(cap, max(width, 0) * max(int(texels), 0), 3), uv


def auto_texels(label, score) -> int:
    """The chart size mesh_texture derives: the median over the labelled triangles of sqrt(2 score) -- the leg in pixels of an
    equal-legged right triangle of that screen area --, rounded up and clamped to 4 .. 64 (4 if nothing is labelled)."""
    s = np.asarray(score, np.float64)[np.asarray(label) >= 0]
    if len(s) == 0:
        return 4
    return int(min(64, max(4, np.ceil(np.median(np.sqrt(2.0 * s))))))


def mesh_texture(vertices, rgb, triangles, images, K4, poses, texels: Optional[int] = None, atlas_width: Optional[int] = None,
                 opt: Optional[MeshTextureOptions] = None, ctx: Optional[Context] = None, level=False):
    """View choice and bake in one: returns (atlas [H, W, 3] uint8 RGB, uv [T, 3, 2] float32, label [T] int32, score [T] float32).
    texels=None derives the chart size from the triangles' screen areas (auto_texels).  level=True (or a MeshTextureLevelOptions)
    levels the seams between the views before the bake (mesh_texture_level)."""
    ctx = ctx or default_context()
    imgs = np.asarray(images)
    label, score = mesh_texture_views(vertices, triangles, imgs.shape[1], imgs.shape[2], K4, poses, opt, ctx)
    S = auto_texels(label, score) if texels is None else int(texels)
    offsets = None
    if level:
        offsets = mesh_texture_level(vertices, triangles, label, imgs, K4, poses, level if isinstance(level, MeshTextureLevelOptions) else None, ctx)[0]
    atlas, uv = mesh_texture_bake(vertices, rgb, triangles, label, imgs, K4, poses, S, atlas_width, ctx, offsets)
    return atlas, uv, label, score


__all__ = ["TSDFGrid", "TSDFOptions", "MeshOptions", "MeshCleanOptions", "MeshSimplifyOptions", "default_tsdf_options",
           "default_mesh_clean_options", "default_mesh_simplify_options", "tsdf_grid", "tsdf_integrate", "tsdf_extract", "mvs_mesh",
           "masked_depth", "mesh_grid", "mesh_arrays", "dense_mesh", "mesh_components", "mesh_clean", "mesh_simplify",
           "MeshTextureOptions", "default_mesh_texture_options", "default_atlas_width", "auto_texels", "mesh_texture_views",
           "mesh_texture_bake", "mesh_texture", "MeshTextureLevelOptions", "MeshTextureLevelStats", "default_mesh_texture_level_options",
           "mesh_texture_level"]
