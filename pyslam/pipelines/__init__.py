"""``pyslam.pipelines``: the frame-to-frame RANSAC, the dense RGB-D VO pipeline and the sparse stereo / RGB-D VO
pipelines with their keyframes, and the sparse monocular pipeline (device implementations).  The sparse pipelines' matcher is this project's own device
matcher, not libviso2; the dense stereo pipeline (cv2.StereoBM) is out of scope."""
from pyslam_amd.pipelines.ransac import FrameToFrameRANSAC, compute_transform_fast  # noqa: F401
from pyslam_amd.pipelines.dense import DenseVOPipeline, DenseRGBDPipeline  # noqa: F401
from pyslam_amd.pipelines.keyframes import (Keyframe, DenseKeyframe, DenseRGBDKeyframe,  # noqa: F401
                                            SparseStereoKeyframe, SparseRGBDKeyframe)
from pyslam_amd.pipelines.sparse import SparseVOPipeline, SparseStereoPipeline, SparseRGBDPipeline  # noqa: F401
from pyslam_amd.pipelines.mono import track_frame, relocalise_frame, SparseMonoPipeline, SparseMonoKeyframe  # noqa: F401
from pyslam_amd.pipelines.loop import loop_candidates, verify_loop, detect_loop  # noqa: F401
from pyslam_amd.pipelines.posegraph import Sim3PoseGraph, correct_loop  # noqa: F401
