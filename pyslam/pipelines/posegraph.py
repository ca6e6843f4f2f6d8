from pyslam_amd.pipelines.posegraph import *  # noqa: F401,F403
from pyslam_amd.pipelines.posegraph import Sim3PoseGraph, correct_loop, loop_graph, apply_correction  # noqa: F401
