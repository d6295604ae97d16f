"""easysfm_amd -- MI355X-native hot path of EasySFM (pairwise descriptor matching + bundle adjustment).

The compute lives in libesfm_hip.so (hand-written HIP for gfx950 behind the C ABI of include/esfm.h);
this package is the Python-side mirror of the reference's FeatureMatching / BundleAdjustment interface.
Importing the package does not touch the GPU; the shared library is loaded on first use and there is
no CPU fallback.
"""
from ._lib import BAOptions, BASummary, Context, EsfmError, ESFM_HAMMING, ESFM_L2_F32, LIB_PATH, lib  # noqa: F401
from .types import DMatch, Frame, SparsePointCloud  # noqa: F401
from .matching import (DescriptorBank, FeatureMatching, PairMatcher, knn_match_hamming, knn_match_l2,  # noqa: F401
                       match_cross_hamming, match_cross_l2, match_cross_pairs_host, match_guided_hamming, match_guided_l2,
                       match_guided_pairs_host, match_hamming, match_l2, match_pairs_host, shard_pair_list)
from .ba import (BAProblem, BundleAdjustment, Comm, ba_solve, ba_solve_ex, ba_solve_groups, ba_solve_radial, ba_sweep_bytes_per_obs, default_options, line_search_next_step, reduced_plan, shard_points,  # noqa: F401
                 torch_allreduce_callback)

from .cloud import (CProceesing, read_ply_mesh, read_ply_normals, read_ply_textured_mesh, read_ply_vertices, sor_filter,  # noqa: F401
                    voxel_merge, write_ply, write_ply_mesh, write_ply_normals, write_ply_textured_mesh, write_png_rgb)
from .motion import (MotionEstimator, find_essential_mat, find_essential_pairs, find_homography, find_homography_pairs, five_point_models,
                     homography_models, homography_refit_host, homography_sample_stream, pixel2cam, ransac_sample_stream, recover_pose,  # noqa: F401
                     recover_pose_pairs, solve_pnp_ransac, triangulate_pairs, triangulate_points)
from .motion import (find_fundamental, find_fundamental_pairs, focal_candidates, focal_cost, focal_from_fundamentals,  # noqa: F401
                     fundamental_models, fundamental_refit_host, fundamental_sample_stream)

from .features import (detectFeaturesORB, detectFeaturesSIFT, detectFeaturesSURF, import_distort, orb_detect_and_compute,  # noqa: F401
                       sift_detect_and_compute, surf_detect_and_compute, undistort)
from .mvs import (MergeOptions, MVSNormalOptions, MVSOptions, default_mvs_normal_options, default_mvs_options, dense_merge,  # noqa: F401
                  dense_reconstruct, dense_reconstruction, merge_arrays, merge_voxel_size, mvs_depth_maps, mvs_fuse, mvs_normals,
                  mvs_plan)
from .mesh import (MeshCleanOptions, MeshOptions, MeshSimplifyOptions, MeshTextureLevelOptions, MeshTextureLevelStats,  # noqa: F401
                   MeshTextureOptions, TSDFGrid, TSDFOptions,
                   default_mesh_clean_options, default_mesh_simplify_options, default_mesh_texture_level_options,
                   default_mesh_texture_options, default_tsdf_options,
                   dense_mesh, masked_depth, mesh_arrays, mesh_clean, mesh_components, mesh_grid, mesh_simplify, mesh_texture,
                   mesh_texture_bake, mesh_texture_level, mesh_texture_views, mvs_mesh, tsdf_extract, tsdf_grid, tsdf_integrate)
from .render import MeshRenderOptions, default_mesh_render_options, mesh_render, mesh_render_error, orbit_poses  # noqa: F401
from .tracks import TrackOptions, TrackResult, refine_tracks, track_evaluate, track_observations, track_triangulate  # noqa: F401
from .tracks import TrackCompleteOptions, TrackCompleteResult, complete_inputs, complete_tracks, free_keypoints, track_complete  # noqa: F401
from .retrieval import (RetrievalOptions, retrieval_pair_list, retrieval_rank, retrieval_train, retrieval_vlad,  # noqa: F401
                        select_pairs)
from .pipeline import MATCH_FILTERS, AutoFocalOptions, FramePair, match_and_verify_all_pairs, propagate_track_ids, run_sfm  # noqa: F401

__version__ = "0.1.0"
from .cameras import (canonical_camera, cameras_line, check_one_image_size, pair_stage_view, parse_camera_distort, parse_camera_file,  # noqa: F401
                      remap_keypoints, split_cameras_token)
