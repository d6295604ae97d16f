"""Observation-sharded bundle adjustment with free radial distortion in two groups: two ranks on cuda:0 over gloo, as
tests/test_ba_groups_multirank_gpu.py runs its case, sharded by point so that rank 0 holds NO observation of group 1.  Whether a
group has observations -- hence whether its six values are boxed and stepped -- must come from the all-reduced counts, and a rank's
empty share of a group's 6 x 6 sums and 6-wide block rows must simply add nothing."""
import os
import sys

import numpy as np
import pytest

from test_ba_multirank_gpu import _free_port

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

GRP = np.array([0, 0, 0, 0, 1, 1, 1, 1], np.int32)
RADIAL_TRUE = np.array([[-0.12, 0.03], [0.05, 0.0]])
ITERS = 6


def _problem():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from easysfm_amd import synth
    import ba_radial_ref as ref
    K0 = np.array(synth.FOUNTAIN_K4, np.float64)
    true = K0[None, :] * np.array([[1.0, 1.0, 1.0, 1.0], [0.8, 1.01, 0.8, 0.99]])
    sc = synth.ba_scene(8, 600, 3, radius=5.0, seed=21, K4_per_cam=true[GRP])
    uv = ref.distort_observations(sc.uv, sc.K4.astype(np.float64)[sc.cam_idx], RADIAL_TRUE[GRP[sc.cam_idx]])
    calib0 = true * np.array([[1.02, 0.99, 0.98, 1.01], [0.98, 1.01, 1.02, 0.99]])
    # rank 0: the points all of whose cameras belong to group 0; rank 1: every other point
    mixed = np.zeros(sc.n_pt, bool)
    mixed[sc.pt_idx[GRP[sc.cam_idx] == 1]] = True
    return sc, uv, calib0, mixed.astype(np.int32)


def _solve(E, sc, uv, calib0, keep, ctx, allreduce=None):
    opt = E.default_options(); opt.max_num_iterations = ITERS
    return E.ba_solve_radial(sc.cam_idx[keep], sc.pt_idx[keep], uv[keep], sc.cams0, sc.pts0, GRP, calib0, [20.0, 20.0], np.zeros((2, 2)), [1.0, 1.0],
                             options=opt, ctx=ctx, allreduce=allreduce)


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    import torch
    import torch.distributed as dist
    try:
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        import easysfm_amd as E
        sc, uv, calib0, shard = _problem()
        keep = shard[sc.pt_idx] == rank
        ctx = E.Context.on_torch_stream(0)
        with torch.cuda.stream(ctx.torch_stream):
            cams, pts, cal, rad, summ = _solve(E, sc, uv, calib0, keep, ctx, E.torch_allreduce_callback())
        q.put((rank, "ok", cams, pts, np.concatenate([cal, rad], 1), [it.cost for it in summ.log()], [it.line_search_steps for it in summ.log()],
               int(np.count_nonzero(GRP[sc.cam_idx[keep]] == 1)), int(keep.sum())))
        dist.barrier()
    except Exception:
        import traceback
        q.put((rank, "FAIL: " + traceback.format_exc(), None, None, None, None, None, None, None))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


def test_two_ranks_one_without_a_radial_groups_observations(gpu_ctx):
    import torch.multiprocessing as mp
    import easysfm_amd as E
    sc, uv, calib0, shard = _problem()
    assert 0 < np.count_nonzero(shard == 0) < sc.n_pt
    cams, pts, cal, rad, summ = _solve(E, sc, uv, calib0, np.ones(sc.n_obs, bool), gpu_ctx)
    blk = np.concatenate([cal, rad], 1)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=600) for _ in range(2)]
    for p in procs:
        p.join(timeout=60)
    assert all(r[1] == "ok" for r in res), [r[1] for r in res]
    res = sorted(res, key=lambda r: r[0])
    assert res[0][7] == 0 and res[0][8] > 0 and res[1][7] > 0            # rank 0 holds observations, none of them of group 1
    ref_cost = [it.cost for it in summ.log()]
    for rank, _, c, p, k, costs, ls, _n1, _n in res:
        assert len(costs) == len(ref_cost) == ITERS + 1
        assert np.allclose(costs, ref_cost, rtol=1e-9)                     # every rank sees the global cost trace
        assert ls == [it.line_search_steps for it in summ.log()]
        assert np.allclose(c, cams, rtol=1e-6, atol=1e-6) and np.allclose(p, pts, rtol=1e-6, atol=1e-6)
        assert np.allclose(k, blk, rtol=1e-7, atol=1e-5)
        assert np.all(np.abs(k[:, :4] - calib0) <= 20.0) and np.all(np.abs(k[:, 4:]) <= 1.0)
    assert np.array_equal(res[0][2], res[1][2]) and np.array_equal(res[0][4], res[1][4])      # cameras and blocks: the same bits on both ranks
    assert not np.any(res[0][4][1, 4:] == 0.0)                             # group 1's k1, k2 moved on rank 0 too
    assert summ.final_cost < 0.5 * summ.initial_cost
