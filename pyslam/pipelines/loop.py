from pyslam_amd.pipelines.loop import *  # noqa: F401,F403
from pyslam_amd.pipelines.loop import loop_candidates, verify_loop, detect_loop, MIN_SCORE  # noqa: F401
