from pyslam_amd.pipelines.mono import *  # noqa: F401,F403
from pyslam_amd.pipelines.mono import track_frame, relocalise_frame, SparseMonoPipeline, SparseMonoKeyframe, window_tables  # noqa: F401
