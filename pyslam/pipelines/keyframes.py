from pyslam_amd.pipelines.keyframes import *  # noqa: F401,F403
from pyslam_amd.pipelines.keyframes import (Keyframe, DenseKeyframe, DenseRGBDKeyframe,  # noqa: F401
                                            SparseStereoKeyframe, SparseRGBDKeyframe)
