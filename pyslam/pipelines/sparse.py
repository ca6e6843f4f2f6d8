from pyslam_amd.pipelines.sparse import *  # noqa: F401,F403
from pyslam_amd.pipelines.sparse import SparseVOPipeline, SparseStereoPipeline, SparseRGBDPipeline  # noqa: F401
