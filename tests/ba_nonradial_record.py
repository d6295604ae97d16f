"""The non-radial solves whose bytes tests/test_ba_radial_gpu.py::test_non_radial_entry_points_unchanged holds to a recording: three
existing-style problems, each solved through the shared-block entry point (esfm_ba_solve_ex) and through the grouped one
(esfm_ba_solve_groups, two alternating groups).  tests/golden/ba_nonradial_parent.npz holds what this function returned on an MI355X
with the library built from the commit BEFORE the radial entry points existed; to record again, build that commit and run
`python tests/ba_nonradial_record.py out.npz` with its package first on the path."""
import ctypes
import sys

import numpy as np

# scene shape (cameras, points, observations per point), seed, box half width: the one-workgroup solve with the LDS-slab Schur
# kernel, BA-25's shape with the register-sum sweep, and the table Schur kernels with the tiled solve
PROBLEMS = [(4, 60, 3, 41, 100.0), (25, 2000, 8, 3, 15.0), (31, 1500, 5, 331, 100.0)]


def _log_bytes(summ):
    """every field of the iteration log and of the summary except the wall time"""
    n = min(summ.num_iterations + 1, len(summ.iterations))
    its = bytes(ctypes.string_at(ctypes.addressof(summ.iterations), ctypes.sizeof(summ.iterations[0]) * n))
    head = np.array([summ.termination, summ.num_iterations, summ.num_successful_steps, summ.num_unsuccessful_steps, summ.num_active_cameras,
                     summ.num_active_points], np.int64).tobytes()
    return np.frombuffer(head + np.float64(summ.initial_cost).tobytes() + np.float64(summ.final_cost).tobytes() + its, np.uint8)


def solves(E, ctx=None):
    from easysfm_amd import synth
    K0 = np.array(synth.FOUNTAIN_K4, np.float64)
    out = {}
    for i, (n_cam, n_pt, per, seed, tol) in enumerate(PROBLEMS):
        sc = synth.ba_scene(n_cam, n_pt, per, seed=seed)
        opt = E.default_options(); opt.max_num_iterations = 4
        calib0 = K0 * np.array([1.02, 0.99, 0.98, 1.01])
        c, p, k, s = E.ba_solve_ex(sc.cam_idx, sc.pt_idx, sc.uv, None, sc.cams0, sc.pts0, calib=calib0, calib_tol=tol, options=opt, ctx=ctx)
        out.update({f"p{i}.shared.cams": c, f"p{i}.shared.pts": p, f"p{i}.shared.calib": k, f"p{i}.shared.log": _log_bytes(s)})
        grp = (np.arange(n_cam) % 2).astype(np.int32)
        cal2 = np.stack([calib0, K0 * np.array([0.98, 1.01, 1.02, 0.99])])
        c, p, k, s = E.ba_solve_groups(sc.cam_idx, sc.pt_idx, sc.uv, sc.cams0, sc.pts0, grp, cal2, [tol, tol], options=opt, ctx=ctx)
        out.update({f"p{i}.groups.cams": c, f"p{i}.groups.pts": p, f"p{i}.groups.calib": k, f"p{i}.groups.log": _log_bytes(s)})
    return out


if __name__ == "__main__":
    import easysfm_amd as E
    np.savez(sys.argv[1], **solves(E))
    print("recorded", sys.argv[1])
