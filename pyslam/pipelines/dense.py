from pyslam_amd.pipelines.dense import *  # noqa: F401,F403
from pyslam_amd.pipelines.dense import DenseVOPipeline, DenseRGBDPipeline  # noqa: F401
