"""C-camera scenes whose cameras have a model each, pinhole or fisheye, for the tests of rigs with fisheye cameras in them.  The
geometry, the scene maker, the views and the exact rig cost are tests/rig_exact.py's, which serve cameras of either model
(stereo_exact.project_view); this module binds what is these scenes' own: their random stream, the cameras "F", "F0", "P", "P0"
and "FN" of stereo_exact.CAMS, whose scenes state ``models`` to the entry points (``rig_exact.entry_args``).  Nothing here imports deepcharuco_amd.

A ``Scene`` is rig_exact's, so ``rig_exact.prefix``, ``pool_views``, ``rig_errors`` and ``chain_visibility`` serve these scenes too."""
import rig_exact as rx
import stereo_exact as sx
from rig_exact import (Scene, cam_args, cost, jacobian_fd, make_rig, models, on_axis, residuals, stationarity,
                       theta_max, with_pose)

THETA_D_MAX_FN = 0.8607                   # the largest theta_d of camera "FN" (stereo_exact.CAMS)
STREAM = 9300


def scene(seed, n_stamps, angles, cams, board=sx.BOARD_S, visible=None, sigma=0.0, rows=None, tag="", rig=None):
    """rig_exact.scene from this module's random stream."""
    return rx.scene(seed, n_stamps, angles, cams, board, visible, sigma, rows, tag, rig, STREAM)
