"""Host-side mirror of the reference's sparse-cloud post-processing over the C ABI:
``CProceesing.SORFilter`` (cpp_code/include/cloudprocessing.hpp:24-36) and ``DataIO.writePlyFile``
(cpp_code/src/data_io.cpp:147-165).  The k-nearest-neighbour pass of the filter runs in libesfm_hip.so on the GPU; the
.ply writer is plain host I/O."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Tuple

import numpy as np

from ._lib import Context, check, default_context, lib
from .types import SparsePointCloud


def sor_filter(points, mean_k: int = 50, std_mul: float = 2.0, ctx: Optional[Context] = None) -> Tuple[np.ndarray, np.ndarray, float]:
    """esfm_sor_filter.  points: [n, stride >= 3] float32 with x, y, z first.
    Returns (keep mask [n] bool, mean k-NN distances [n] float32, threshold)."""
    ctx = ctx or default_context()
    pts = np.ascontiguousarray(points, np.float32)
    if pts.ndim != 2 or pts.shape[1] < 3:
        raise ValueError("points must be [n, >= 3]")
    n, stride = pts.shape
    md = np.zeros(max(n, 1), np.float32); keep = np.zeros(max(n, 1), np.uint8)
    n_keep = C.c_int32(0); thr = C.c_double(0.0)
    check(lib().esfm_sor_filter(ctx.handle, C.c_void_p(pts.ctypes.data), n, stride, int(mean_k), float(std_mul),
                                C.c_void_p(md.ctypes.data), C.c_void_p(keep.ctypes.data), C.byref(n_keep), C.byref(thr)))
    return keep[:n].astype(bool), md[:n], thr.value


def voxel_merge(xyz, rgb=None, normals=None, tags=None, voxel_size: float = 1.0, min_points: int = 1, min_tags: int = 0,
                ctx: Optional[Context] = None):
    """esfm_cloud_voxel_merge: one point per occupied voxel of side voxel_size, in ascending voxel-key order.  xyz [n, 3] float32;
    rgb [n, 3] uint8, normals [n, 3] float32 and tags [n] int32 (0..63) are optional.  Returns (xyz [m, 3], rgb [m, 3] or None,
    normals [m, 3] or None, count [m] int32, tagmask [m] uint64 or None)."""
    ctx = ctx or default_context()
    pts = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = len(pts)

    def opt_in(a, dtype, width):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype).reshape((n, width) if width else (n,))
        return a

    c, nr, tg = opt_in(rgb, np.uint8, 3), opt_in(normals, np.float32, 3), opt_in(tags, np.int32, 0)
    cap = max(n, 1)
    o_xyz = np.zeros((cap, 3), np.float32)
    o_rgb = np.zeros((cap, 3), np.uint8) if c is not None else None
    o_nrm = np.zeros((cap, 3), np.float32) if nr is not None else None
    o_cnt = np.zeros(cap, np.int32)
    o_msk = np.zeros(cap, np.uint64) if tg is not None else None
    m = C.c_int32(0)

    def ptr(a):
        return C.c_void_p(a.ctypes.data) if a is not None else None

    check(lib().esfm_cloud_voxel_merge(ctx.handle, n, ptr(pts), ptr(c), ptr(nr), ptr(tg), float(voxel_size), int(min_points), int(min_tags),
                                       ptr(o_xyz), ptr(o_rgb), ptr(o_nrm), ptr(o_cnt), ptr(o_msk), C.byref(m)))
    k = m.value
    cut = lambda a: None if a is None else a[:k].copy()
    return cut(o_xyz), cut(o_rgb), cut(o_nrm), cut(o_cnt), cut(o_msk)


class CProceesing:
    """Mirror of ``CProceesing<PointT>`` (cloudprocessing.hpp:20-72; the reference's spelling), SOR filter only."""

    def __init__(self, ctx: Optional[Context] = None):
        self._ctx = ctx

    def SORFilter(self, incloud: SparsePointCloud, MeanK: int = 50, std: float = 2.0) -> SparsePointCloud:
        """cloudprocessing.hpp:24-36.  Returns the filtered cloud (the reference fills ``outcloud``); survivors keep
        their input order, colours travel with the points; track ids / inlier flags are not part of a pcl cloud."""
        xyz = np.ascontiguousarray(incloud.xyz, np.float32).reshape(-1, 3)
        keep, _, _ = sor_filter(xyz, MeanK, std, self._ctx)
        out = SparsePointCloud(xyz=xyz[keep].copy())
        rgb = np.asarray(incloud.rgb)
        if rgb.shape[0] == xyz.shape[0]:
            out.rgb = rgb[keep].copy()
        print(f"apply SOR filter: [ {xyz.shape[0]} ] points before filtering, [ {int(keep.sum())} ] points after filtering.")
        return out


def _fmt(v: float) -> str:
    """operator<< of a float on a stream with precision 8 (pcl::PLYWriter::writeASCII's default): %.8g."""
    return "%.8g" % float(np.float32(v))


def write_ply(file_name: str, cloud: SparsePointCloud) -> bool:
    """DataIO::writePlyFile (data_io.cpp:147-165): width = 1, height = N (:151-152), then pcl::io::savePLYFile, i.e. an
    ASCII PLY of PointXYZRGB with the camera element PCL appends [upstream pcl/io/ply_io.cpp PLYWriter::generateHeader /
    writeASCII, restated from memory; the reference ships no example file, SURVEY.md section 8 f-3]."""
    xyz = np.asarray(cloud.xyz, np.float32).reshape(-1, 3)
    n = xyz.shape[0]
    rgb = np.asarray(cloud.rgb, np.uint8).reshape(-1, 3) if len(cloud.rgb) == n else np.zeros((n, 3), np.uint8)
    width, height = 1, n
    head = ["ply", "format ascii 1.0", "comment PCL generated", f"element vertex {n}",
            "property float x", "property float y", "property float z",
            "property uchar red", "property uchar green", "property uchar blue",
            "element camera 1",
            "property float view_px", "property float view_py", "property float view_pz",
            "property float x_axisx", "property float x_axisy", "property float x_axisz",
            "property float y_axisx", "property float y_axisy", "property float y_axisz",
            "property float z_axisx", "property float z_axisy", "property float z_axisz",
            "property float focal", "property float scalex", "property float scaley",
            "property float centerx", "property float centery",
            "property int viewportx", "property int viewporty",
            "property float k1", "property float k2", "end_header"]
    try:
        with open(file_name, "w") as f:
            f.write("\n".join(head) + "\n")
            for i in range(n):
                f.write(f"{_fmt(xyz[i, 0])} {_fmt(xyz[i, 1])} {_fmt(xyz[i, 2])} {int(rgb[i, 0])} {int(rgb[i, 1])} {int(rgb[i, 2])}\n")
            # sensor origin 0, identity orientation, no focal / scale / centre, viewport = width x height, no k1 k2
            f.write(f"0 0 0 1 0 0 0 1 0 0 0 1 0 0 0 0 0 {width} {height} 0 0\n")
    except OSError:
        print("Couldn't write file ")
        return False
    print(f"Output [ {n} ] points.\nOutput ply file done.")
    return True


def write_ply_normals(file_name: str, cloud: SparsePointCloud, normals) -> bool:
    """ASCII PLY with oriented points: properties x y z nx ny nz red green blue (what surface reconstruction tools read)."""
    xyz = np.asarray(cloud.xyz, np.float32).reshape(-1, 3)
    n = xyz.shape[0]
    nrm = np.asarray(normals, np.float32).reshape(-1, 3)
    if len(nrm) != n:
        raise ValueError("one normal per point")
    rgb = np.asarray(cloud.rgb, np.uint8).reshape(-1, 3) if len(cloud.rgb) == n else np.zeros((n, 3), np.uint8)
    head = ["ply", "format ascii 1.0", f"element vertex {n}"] + [f"property float {p}" for p in ("x", "y", "z", "nx", "ny", "nz")] + \
           [f"property uchar {p}" for p in ("red", "green", "blue")] + ["end_header"]
    try:
        with open(file_name, "w") as f:
            f.write("\n".join(head) + "\n")
            for i in range(n):
                f.write(" ".join(_fmt(v) for v in (*xyz[i], *nrm[i])) + f" {int(rgb[i, 0])} {int(rgb[i, 1])} {int(rgb[i, 2])}\n")
    except OSError:
        print("Couldn't write file ")
        return False
    print(f"Output [ {n} ] points.\nOutput ply file done.")
    return True


def read_ply_normals(file_name: str):
    """Reader for the files write_ply_normals produces: (xyz [n, 3] f32, normals [n, 3] f32, rgb [n, 3] u8)."""
    with open(file_name) as f:
        lines = f.read().split("\n")
    n = int([l for l in lines if l.startswith("element vertex")][0].split()[-1])
    props = [l.split()[-1] for l in lines[:lines.index("end_header")] if l.startswith("property")]
    if props != ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue"]:
        raise ValueError(f"not a write_ply_normals file: {props}")
    body = lines[lines.index("end_header") + 1:]
    arr = np.array([l.split() for l in body[:n]], np.float64).reshape(n, 9)
    return arr[:, :3].astype(np.float32), arr[:, 3:6].astype(np.float32), arr[:, 6:].astype(np.uint8)


def write_ply_mesh(file_name: str, vertices, normals, rgb, triangles) -> bool:
    """ASCII PLY of an indexed triangle mesh: the vertex properties of write_ply_normals (x y z nx ny nz red green blue; normals
    or rgb None: zeros), then ``element face`` with ``property list uchar int vertex_indices``."""
    xyz = np.asarray(vertices, np.float32).reshape(-1, 3)
    n = xyz.shape[0]
    nrm = np.asarray(normals, np.float32).reshape(-1, 3) if normals is not None else np.zeros((n, 3), np.float32)
    col = np.asarray(rgb, np.uint8).reshape(-1, 3) if rgb is not None else np.zeros((n, 3), np.uint8)
    tri = np.asarray(triangles, np.int32).reshape(-1, 3)
    if len(nrm) != n or len(col) != n:
        raise ValueError("one normal and one colour per vertex")
    if len(tri) and (tri.min() < 0 or tri.max() >= n):
        raise ValueError("a triangle index is out of range")
    head = ["ply", "format ascii 1.0", f"element vertex {n}"] + [f"property float {p}" for p in ("x", "y", "z", "nx", "ny", "nz")] + \
           [f"property uchar {p}" for p in ("red", "green", "blue")] + \
           [f"element face {len(tri)}", "property list uchar int vertex_indices", "end_header"]
    try:
        with open(file_name, "w") as f:
            f.write("\n".join(head) + "\n")
            for i in range(n):
                f.write(" ".join(_fmt(v) for v in (*xyz[i], *nrm[i])) + f" {int(col[i, 0])} {int(col[i, 1])} {int(col[i, 2])}\n")
            for a, b, c in tri.tolist():
                f.write(f"3 {a} {b} {c}\n")
    except OSError:
        print("Couldn't write file ")
        return False
    print(f"Output [ {n} ] vertices, [ {len(tri)} ] triangles.\nOutput ply file done.")
    return True


def read_ply_mesh(file_name: str):
    """Reader for the files write_ply_mesh produces: (vertices [n, 3] f32, normals [n, 3] f32, rgb [n, 3] u8, triangles [m, 3] i32)."""
    with open(file_name) as f:
        lines = f.read().split("\n")
    end = lines.index("end_header")
    n = int([l for l in lines[:end] if l.startswith("element vertex")][0].split()[-1])
    m = int([l for l in lines[:end] if l.startswith("element face")][0].split()[-1])
    props = [l.split()[-1] for l in lines[:end] if l.startswith("property")]
    if props != ["x", "y", "z", "nx", "ny", "nz", "red", "green", "blue", "vertex_indices"]:
        raise ValueError(f"not a write_ply_mesh file: {props}")
    body = lines[end + 1:]
    arr = np.array([l.split() for l in body[:n]], np.float64).reshape(n, 9)
    faces = np.array([l.split() for l in body[n:n + m]], np.int64).reshape(m, 4)
    if m and np.any(faces[:, 0] != 3):
        raise ValueError("not a triangle mesh")
    return arr[:, :3].astype(np.float32), arr[:, 3:6].astype(np.float32), arr[:, 6:].astype(np.uint8), faces[:, 1:].astype(np.int32)


def write_png_rgb(file_name: str, image) -> bool:
    """An 8-bit RGB PNG of image [rows, cols, 3] uint8: one IDAT chunk, scanline filter 0 (the host layer's C++ writer stores the
    same scanlines without compression; both decode to the same pixels)."""
    import struct
    import zlib
    img = np.ascontiguousarray(image, np.uint8)
    if img.ndim != 3 or img.shape[2] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError("image must be [rows, cols, 3] with at least one pixel")
    rows, cols = img.shape[:2]
    raw = np.concatenate([np.zeros((rows, 1), np.uint8), img.reshape(rows, cols * 3)], axis=1).tobytes()

    def chunk(kind: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data) & 0xFFFFFFFF)
    try:
        with open(file_name, "wb") as f:
            f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", cols, rows, 8, 2, 0, 0, 0)) + chunk(b"IDAT", zlib.compress(raw, 6)) +
                    chunk(b"IEND", b""))
    except OSError:
        print("Couldn't write file ")
        return False
    return True


def texture_file_name(file_name: str) -> str:
    """The atlas of mesh.ply goes beside it as mesh.png."""
    return os.path.splitext(file_name)[0] + ".png"


def write_ply_textured_mesh(file_name: str, vertices, normals, triangles, uv, atlas) -> bool:
    """ASCII PLY of a textured triangle mesh as MeshLab and Blender read it: ``comment TextureFile <name>.png`` in the header, the
    vertex properties x y z nx ny nz (normals None: zeros), and per face ``property list uchar int vertex_indices`` and
    ``property list uchar float texcoord`` with the six values u0 v0 u1 v1 u2 v2.  uv [T, 3, 2] is mesh_texture's (v down the atlas
    rows); the file holds (u, 1 - v), the readers' convention with v up.  The atlas [H, W, 3] uint8 RGB goes beside the file as an
    8-bit RGB PNG of the same stem."""
    xyz = np.asarray(vertices, np.float32).reshape(-1, 3)
    n = xyz.shape[0]
    nrm = np.asarray(normals, np.float32).reshape(-1, 3) if normals is not None else np.zeros((n, 3), np.float32)
    tri = np.asarray(triangles, np.int32).reshape(-1, 3)
    tex = np.asarray(uv, np.float32).reshape(-1, 3, 2)
    if len(nrm) != n or len(tex) != len(tri):
        raise ValueError("one normal per vertex and three texture coordinates per triangle")
    if len(tri) and (tri.min() < 0 or tri.max() >= n):
        raise ValueError("a triangle index is out of range")
    png = texture_file_name(file_name)
    head = ["ply", "format ascii 1.0", f"comment TextureFile {os.path.basename(png)}", f"element vertex {n}"] + \
           [f"property float {p}" for p in ("x", "y", "z", "nx", "ny", "nz")] + \
           [f"element face {len(tri)}", "property list uchar int vertex_indices", "property list uchar float texcoord", "end_header"]
    flipped = np.stack([tex[..., 0], np.float32(1.0) - tex[..., 1]], axis=-1).reshape(-1, 6)
    try:
        with open(file_name, "w") as f:
            f.write("\n".join(head) + "\n")
            for i in range(n):
                f.write(" ".join(_fmt(v) for v in (*xyz[i], *nrm[i])) + "\n")
            for (a, b, c), t in zip(tri.tolist(), flipped):
                f.write(f"3 {a} {b} {c} 6 " + " ".join(_fmt(v) for v in t) + "\n")
    except OSError:
        print("Couldn't write file ")
        return False
    if not write_png_rgb(png, atlas):
        return False
    print(f"Output [ {n} ] vertices, [ {len(tri)} ] triangles, texture [ {np.asarray(atlas).shape[1]} x {np.asarray(atlas).shape[0]} ].\nOutput ply file done.")
    return True


def read_ply_textured_mesh(file_name: str):
    """Reader for the files write_ply_textured_mesh produces: (vertices [n, 3] f32, normals [n, 3] f32, triangles [m, 3] i32, uv
    [m, 3, 2] f32 with v down the atlas rows again, the texture's file name as the header gives it)."""
    with open(file_name) as f:
        lines = f.read().split("\n")
    end = lines.index("end_header")
    n = int([l for l in lines[:end] if l.startswith("element vertex")][0].split()[-1])
    m = int([l for l in lines[:end] if l.startswith("element face")][0].split()[-1])
    props = [l.split()[-1] for l in lines[:end] if l.startswith("property")]
    if props != ["x", "y", "z", "nx", "ny", "nz", "vertex_indices", "texcoord"]:
        raise ValueError(f"not a write_ply_textured_mesh file: {props}")
    texture = [l for l in lines[:end] if l.startswith("comment TextureFile ")][0][len("comment TextureFile "):]
    body = lines[end + 1:]
    arr = np.array([l.split() for l in body[:n]], np.float64).reshape(n, 6)
    faces = np.array([l.split() for l in body[n:n + m]], np.float64).reshape(m, 11)
    if m and (np.any(faces[:, 0] != 3) or np.any(faces[:, 4] != 6)):
        raise ValueError("not a textured triangle mesh")
    uv = faces[:, 5:].astype(np.float32).reshape(m, 3, 2)
    uv[..., 1] = np.float32(1.0) - uv[..., 1]
    return arr[:, :3].astype(np.float32), arr[:, 3:].astype(np.float32), faces[:, 1:4].astype(np.int32), uv, texture


def read_ply_vertices(file_name: str):
    """Minimal reader for the files write_ply produces (round-trip tests)."""
    with open(file_name) as f:
        lines = f.read().split("\n")
    n = int([l for l in lines if l.startswith("element vertex")][0].split()[-1])
    body = lines[lines.index("end_header") + 1:]
    arr = np.array([l.split() for l in body[:n]], np.float64).reshape(n, 6)
    return arr[:, :3].astype(np.float32), arr[:, 3:].astype(np.uint8), body[n]
