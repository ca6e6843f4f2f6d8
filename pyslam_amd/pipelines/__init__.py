"""Pipeline steps with a device implementation: the frame-to-frame RANSAC of the reference's sparse VO pipeline
(pyslam/pipelines/ransac.py), the step that feeds the motion-only solve, and the dense RGB-D VO pipeline
(pyslam/pipelines/dense.py, keyframes.py) with its image front end (imgproc: host restatements of the two cv2 calls it
makes), and the sparse stereo / RGB-D VO pipelines (pyslam/pipelines/sparse.py) with a feature matcher of this
project's own in place of libviso2 (matcher: the device matcher; featproc: its host restatement).
twoview: essential-matrix RANSAC and the two-view bootstrap of monocular bundle adjustment (epipolar: its host restatement).
pnp: absolute-pose (P3P) RANSAC, the registration of a further monocular frame against the map (absolute: its host restatement).
sim3: similarity (Sim(3)) alignment RANSAC of two matched 3-D point sets -- a monocular map against a trajectory in metres, a second
map or another keyframe (similarity: its host restatement).
mono: matching by projection composed into ``track_frame``, matching without a prior composed into ``relocalise_frame``, and the
monocular pipeline ``SparseMonoPipeline``.
loop: the matcher's keyframe database composed with matching without a prior and the Sim(3) RANSAC into ``detect_loop`` (place
recognition and its geometric verification).
posegraph: the Sim(3) pose graph that consumes a verified loop constraint and corrects the map -- ``Sim3PoseGraph``, ``correct_loop``
(simgraph: its host restatement).
The stereo dense pipeline (cv2.StereoBM) is not in scope (out of scope)."""
from .ransac import FrameToFrameRANSAC, compute_transform_fast  # noqa: F401
from .twoview import EssentialRANSAC, bootstrap  # noqa: F401
from .pnp import PnPRANSAC, register_frame  # noqa: F401
from .sim3 import Sim3RANSAC, align_maps, align_trajectories, transform_map  # noqa: F401
from .dense import DenseVOPipeline, DenseRGBDPipeline  # noqa: F401
from .keyframes import Keyframe, DenseKeyframe, DenseRGBDKeyframe, SparseStereoKeyframe, SparseRGBDKeyframe  # noqa: F401
from .sparse import SparseVOPipeline, SparseStereoPipeline, SparseRGBDPipeline  # noqa: F401
from .matcher import Matcher, Matcher_parameters  # noqa: F401
from .mono import track_frame, relocalise_frame, SparseMonoPipeline, SparseMonoKeyframe  # noqa: F401
from .loop import loop_candidates, verify_loop, detect_loop  # noqa: F401
from .posegraph import Sim3PoseGraph, correct_loop  # noqa: F401
