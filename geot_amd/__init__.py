"""geot_amd -- MI355X (gfx950) implementation of GeoT's point-cloud sampling / grouping /
interpolation hot path behind the reference's operator API.

    from geot_amd.pointnet2 import pointnet2_utils          # furthest_point_sample, ball_query, ...
    from geot_amd.pointops.functions import pointops        # fps, knn, ...
    from geot_amd.knn_cuda import KNN
    import geot_amd.aliases; geot_amd.aliases.install()     # reference import names -> this package
    from geot_amd import fit, train_one_epoch, epoch_batches, LrSchedule      # the training driver (fit.py, schedule.py)
    from geot_amd import ToothScores, tooth_scores_from_moments, tooth_instances     # the Teeth3DS challenge scores (validation.py)
    from geot_amd import clean_scans, scan_components, scan_neighbours, teeth3ds_result  # connected teeth, the challenge's result
    from geot_amd import mesh_neighbours                    # the scan meshes' one-ring tables for them (DeviceScanSet(faces=))

The compute path is libgeot_hip.so (C ABI in include/geot_hip.h); there is no CPU fallback.
"""
__version__ = "0.1.0"

import os as _os
import sys as _sys


# hipGraph replays (geot_amd/graph_step.py) and the runtime's "graph packet capture" (on by default in ROCm 7.0): with it on,
# the AQL packets of a graph's hipMemsetAsync / hipMemcpyAsync NODES keep pointing at kernel-argument slots of the device's
# shared ring, and a few thousand eager launches between two replays recycle those slots -- the memsets then clear something
# else, and every torch reduction that zeroes its semaphores that way returns garbage, silently
# (profiles/r04_graph_capture_notes.txt has the reproducer).  Graphs of kernel nodes alone are not affected.
# The HIP runtime reads the switch at ITS first call -- which can be earlier than any torch.cuda call this module could see
# (torch.cuda.is_available() / device_count() before the import, or a preloaded tool such as rocprofv3) -- so a value this
# module sets itself is a best effort, never a proof.  Hence three states:
#   exported "0" by the launcher (the process environment had DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 before this import):
#                   packet capture is known to be off; any graph replays correctly (7-20 ms of host time per launch);
#   GEOT_GRAPH_LAUNCH=safe (default), not exported: this module sets the variable to 0 now (in time when nothing has touched
#                   HIP yet), but since that cannot be verified every captured graph is INSPECTED (hipGraphGetNodes) and one
#                   that holds anything but kernel nodes is refused -- exactly as in fast mode;
#   GEOT_GRAPH_LAUNCH=fast: packet capture stays ON (0.5 ms per launch); every captured graph is inspected, kernel-only accepted.
# The training steps of this package capture kernel-only (tests/test_graph_step_gpu.py); code added around them may not --
# then export the variable in the launcher.
GRAPH_PACKET_CAPTURE_ENV = "DEBUG_CLR_GRAPH_PACKET_CAPTURE"
GRAPH_LAUNCH = _os.environ.get("GEOT_GRAPH_LAUNCH", "safe")
if GRAPH_LAUNCH not in ("safe", "fast"):
    raise ImportError("GEOT_GRAPH_LAUNCH must be 'safe' or 'fast', not %r" % GRAPH_LAUNCH)
_EXPORTED_BEFORE_IMPORT = _os.environ.get(GRAPH_PACKET_CAPTURE_ENV)
if GRAPH_LAUNCH == "safe":
    _os.environ.setdefault(GRAPH_PACKET_CAPTURE_ENV, "0")


def graph_replay_is_safe():
    """True only when the launcher exported DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 (the process environment held it before this
    import): hipGraph packet capture is then off for certain and any captured graph replays correctly.  Otherwise graph_step
    (and bench.py's own captures) inspect every graph and accept kernel nodes only."""
    return _EXPORTED_BEFORE_IMPORT == "0"


# The training driver's names, bound on first use (importing the package itself imports nothing else: the switch above has to
# be set before anything touches HIP).  `fit` needs no entry: geot_amd.fit is the module, and the module is callable.
_EXPORTS = {"train_one_epoch": "fit", "epoch_batches": "fit", "LrSchedule": "schedule",
            "ToothScores": "validation", "tooth_scores_from_moments": "validation", "tooth_instances": "validation",
            "clean_scans": "validation", "scan_components": "validation", "scan_neighbours": "validation",
            "teeth3ds_result": "validation", "mesh_neighbours": "validation"}


def __getattr__(name):
    if name in _EXPORTS:
        import importlib
        return getattr(importlib.import_module("." + _EXPORTS[name], __name__), name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
