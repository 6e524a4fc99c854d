"""The reference's ``evals.utils.transformations`` names (evals/utils/transformations.py), device-tensor functions of mvp.corr3d."""
from mvp.corr3d import so3_relative_angle, so3_rotation_angle, transform_points_Rt  # noqa: F401
