"""Pipeline steps with a device implementation: the frame-to-frame RANSAC of the reference's sparse VO pipeline
(pyslam/pipelines/ransac.py), the step that feeds the motion-only solve, and the dense RGB-D VO pipeline
(pyslam/pipelines/dense.py, keyframes.py) with its image front end (imgproc: host restatements of the two cv2 calls it
makes).  The cv2 / viso2 front ends of the sparse pipeline and the stereo dense pipeline (cv2.StereoBM) are not in scope
(out of scope)."""
from .ransac import FrameToFrameRANSAC, compute_transform_fast  # noqa: F401
from .dense import DenseVOPipeline, DenseRGBDPipeline  # noqa: F401
from .keyframes import Keyframe, DenseKeyframe, DenseRGBDKeyframe, SparseStereoKeyframe, SparseRGBDKeyframe  # noqa: F401
