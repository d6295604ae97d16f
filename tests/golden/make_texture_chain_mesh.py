"""Writes tests/golden/texture_chain_mesh.npz: the synthetic scene (tests/mvs_scene.py) through the numpy restatements of the
dense chain -- 48-plane depth maps, the fusion's mask, the TSDF mesh on tsdf_ref.CHAIN_GRID, the clean-up with its defaults and
the simplification at two voxels per cell from the grid origin, as tests/test_mesh_simplify_gpu.py builds it on the GPU (1 138
vertices, 2 000 triangles; the GPU's mesh has the same bits).  About 15 s on a CPU.  Run from the repository root:
python tests/golden/make_texture_chain_mesh.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import merge_ref as G  # noqa: E402
import mesh_clean_ref as C  # noqa: E402
import mvs_ref as M  # noqa: E402
import mvs_scene as S  # noqa: E402
import simplify_ref as Q  # noqa: E402
import tsdf_ref as T  # noqa: E402

scene = S.make_scene()
nb, rng, ro = T.chain_plan(scene, M)
depth, _ = M.depth_maps(scene["images"], scene["K4"], scene["poses"], nb, rng, ro)
index = G.fuse_index(scene["K4"], scene["poses"], nb, depth, ro)
origin, h, dims = T.CHAIN_GRID
f, w, rgb = T.integrate(scene["images"], scene["K4"], scene["poses"], T.masked_depth(depth, index), origin, h, dims)
v, _, c, t = T.extract(f, w, rgb, origin, h)
cv, _, crgb, ct = C.clean(v, c, t)[:4]
out = Q.simplify(cv, crgb, ct, np.float32(2 * 0.04), origin)
assert (len(out[0]), len(out[3])) == (1138, 2000)
np.savez_compressed(os.path.join(HERE, "texture_chain_mesh.npz"), vertices=out[0], rgb=out[2], triangles=out[3])
