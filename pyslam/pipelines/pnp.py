from pyslam_amd.pipelines.pnp import *  # noqa: F401,F403
from pyslam_amd.pipelines.pnp import PnPRANSAC, register_frame, three_view_tables  # noqa: F401
