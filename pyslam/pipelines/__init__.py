"""``pyslam.pipelines``: the frame-to-frame RANSAC and the dense RGB-D VO pipeline with its keyframes (device
implementations).  The cv2 / viso2 front ends of the reference's sparse and stereo pipelines are out of scope
(DESIGN.md)."""
from pyslam_amd.pipelines.ransac import FrameToFrameRANSAC, compute_transform_fast  # noqa: F401
from pyslam_amd.pipelines.dense import DenseVOPipeline, DenseRGBDPipeline  # noqa: F401
from pyslam_amd.pipelines.keyframes import (Keyframe, DenseKeyframe, DenseRGBDKeyframe,  # noqa: F401
                                            SparseStereoKeyframe, SparseRGBDKeyframe)
