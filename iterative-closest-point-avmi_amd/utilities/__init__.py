"""Drop-in for the reference's ``utilities`` package (utilities/__init__.py:1-9):
``ICP``, ``voxel_downsample``, ``rotation_search``, ``feature_based_alignment``
(with its stages ``compute_curvature``, ``extract_keypoints``, ``compute_descriptors``,
``match_descriptors``, ``ransac_align``), ``OccupancyGrid2D`` and ``PoseGraph2D`` run on the
MI355X through libicpmi.so."""
from . import features, icp, mapping, pose_graph  # noqa: F401

ICP, voxel_downsample = icp.ICP, icp.voxel_downsample
rotation_search, feature_based_alignment = features.rotation_search, features.feature_based_alignment
compute_curvature, extract_keypoints = features.compute_curvature, features.extract_keypoints
compute_descriptors, match_descriptors = features.compute_descriptors, features.match_descriptors
ransac_align = features.ransac_align
OccupancyGrid2D = mapping.OccupancyGrid2D
PoseGraph2D = pose_graph.PoseGraph2D
pose_matrix_to_vec, pose_vec_to_matrix = pose_graph.pose_matrix_to_vec, pose_graph.pose_vec_to_matrix
relative_transform_vec = pose_graph.relative_transform_vec

__all__ = ["ICP", "voxel_downsample", "rotation_search", "feature_based_alignment", "compute_curvature", "extract_keypoints",
           "compute_descriptors", "match_descriptors", "ransac_align", "OccupancyGrid2D", "PoseGraph2D",
           "pose_matrix_to_vec", "pose_vec_to_matrix", "relative_transform_vec"]
