"""Pose refinement of Predator_APR's KITTI loader (/root/reference/Predator_APR/datasets/kitti.py:419-428).

The loader moves frame 0 by the odometry pose M, registers it onto frame 1 with point-to-point ICP (0.2 m, 200
iterations, full clouds: "for ICP we don't voxelize") and composes the two.  That is FCGF_APR's `_get_icp` with source
and target swapped and the 5 cm reduction off, so it runs on the same code (apr_amd/fcgf/lib/apg.py, csrc/icp.hip).
Disk caches and KITTI file IO stay with the caller.

The loader's complement frames take the multiway route (kitti.py:197-297: pairwise_registration, full_registration,
multiway_registration, the same text as FCGF_APR's loader, on clouds reduced to one point per 5 cm voxel), so that too
runs on FCGF's code: `multiway_registration` below is apr_amd/fcgf/lib/apg.py's (csrc/icp.hip, csrc/posegraph.hip).
"""
from ...fcgf.lib.apg import (full_registration, multiway_registration, pairwise_init, pairwise_inits,  # noqa: F401
                             refine_complement_poses, refine_pose)


def refine_pair_pose(xyz_0, xyz_1, M, icp_voxel_size=None, max_dist=0.2, max_iteration=200):
    """kitti.py:419-428: float64 [4,4] pose moving frame 0 into frame 1 (xyz_1 ~= xyz_0 @ R.T + t), refined from M."""
    return refine_pose(xyz_1, xyz_0, M, icp_voxel_size, max_dist, max_iteration)
