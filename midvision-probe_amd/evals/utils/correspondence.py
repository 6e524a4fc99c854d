"""The reference's ``evals.utils.correspondence`` names (evals/utils/correspondence.py) on the HIP path: the NAVI 3-D
correspondence functions live in mvp.corr3d (faiss replaced by mvp_knn_ratio), ``argmax_2d`` in mvp.spair.  Not built:
``estimate_correspondence_depth`` / ``sample_pointcloud_features`` / ``grid_to_pointcloud`` (ScanNet) and ``error_auc``."""
from mvp.corr3d import (calculate_ratio_test, compute_binned_performance, estimate_correspondence_xyz,  # noqa: F401
                        get_correspondences_ratio_test, get_grid, get_topk_matches, knn_ratio, project_3dto2d)
from mvp.spair import argmax_2d  # noqa: F401
