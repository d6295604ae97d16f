"""Meshes the mesh clean-up's CPU and GPU tests share, built with tests/tsdf_ref.py: three closed spheres of different sizes in
one volume, the sphere a weight-0 slab opens, and triangle strips with chosen vertex numberings."""
import numpy as np

from tsdf_ref import extract, sphere_volume

F = np.float32
THREE_DIMS, THREE_H = (20, 18, 16), 0.1
THREE_COUNTS = (3708, 644, 256)                                   # triangles of the three spheres


def three_sphere_volume(noise=None):
    """min of three exact sphere distances on 20 x 18 x 16 voxels of 0.1, weight 2 everywhere: (tsdf, weight, centre and radius
    of the large sphere).  noise (an array of the volume's shape) is added to the distances."""
    f, w, centre, radius = sphere_volume(THREE_DIMS, THREE_H)
    f2 = sphere_volume(THREE_DIMS, THREE_H, centre_voxel=[3.2, 3.4, 3.1], radius_voxels=1.6)[0]
    f3 = sphere_volume(THREE_DIMS, THREE_H, centre_voxel=[16.3, 3.3, 12.6], radius_voxels=2.4)[0]
    f = np.minimum(np.minimum(f, f2), f3)
    if noise is not None:
        f = (f + np.asarray(noise, F)).astype(F)
    return f, w, centre, radius


def three_spheres(noise=None, colours=True):
    """(vertices, gradient normals, rgb, triangles, centre, radius) of the three-sphere mesh."""
    f, w, centre, radius = three_sphere_volume(noise)
    rgb = np.random.default_rng(4).integers(0, 256, f.shape + (3,)).astype(np.uint8) if colours else None
    return extract(f, w, rgb, (0, 0, 0), THREE_H) + (centre, radius)


def opened_sphere():
    """The 14 x 15 x 16 sphere with a slab of weight 0 through it: an open mesh (tests/test_tsdf_cpu.py
    test_invalid_slab_opens_the_mesh)."""
    f, w, _, _ = sphere_volume((14, 15, 16))
    w[:, 6:8, :] = 0
    return extract(f, w, None, (0, 0, 0), 0.1)


def strip(n_vertices, numbering, seed=0, repeat_index=False):
    """A triangle strip (i, i + 1, i + 2) over n_vertices vertices, renumbered "ascending", "descending" or "random" (seeded),
    its triangles shuffled; repeat_index makes one triangle in the middle name a vertex twice (the strip stays connected)."""
    rng = np.random.default_rng(seed)
    i = np.arange(n_vertices - 2)
    t = np.stack([i, i + 1, i + 2], 1)
    if repeat_index:
        t[len(t) // 2, 2] = t[len(t) // 2, 0]
    perm = {"ascending": np.arange(n_vertices), "descending": np.arange(n_vertices)[::-1], "random": rng.permutation(n_vertices)}[numbering]
    return np.ascontiguousarray(perm[t][rng.permutation(len(t))].astype(np.int32))
