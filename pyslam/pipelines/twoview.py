from pyslam_amd.pipelines.twoview import *  # noqa: F401,F403
from pyslam_amd.pipelines.twoview import EssentialRANSAC, bootstrap, two_view_tables  # noqa: F401
