from pyslam_amd.pipelines.sim3 import *  # noqa: F401,F403
from pyslam_amd.pipelines.sim3 import Sim3RANSAC, align_maps, align_trajectories, invert, transform_map  # noqa: F401
