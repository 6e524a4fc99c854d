"""The reference's ``evals.utils.correspondence`` names (evals/utils/correspondence.py) on the HIP path: the NAVI and ScanNet 3-D
correspondence functions live in mvp.corr3d (faiss replaced by mvp_knn_ratio, grid_sample by mvp_pointcloud_sample), ``argmax_2d``
in mvp.spair.  ``knn_points`` / ``faiss_knn`` have no counterpart of their own: ``knn_ratio`` is the search."""
from mvp.corr3d import (calculate_ratio_test, compute_binned_performance, error_auc, estimate_correspondence_depth,  # noqa: F401
                        estimate_correspondence_xyz, get_correspondences_ratio_test, get_grid, get_topk_matches, grid_to_pointcloud,
                        knn_ratio, project_3dto2d, sample_pointcloud_features)
from mvp.spair import argmax_2d  # noqa: F401
