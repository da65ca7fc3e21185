"""The tracker's depth-image source without a GPU (dsr_tracker_track_frame): the
symbol in the header, the exports and the ctypes layer (the method of test_abi_cpu.py), the null
handle, and ObjectTracker.track_frame / Optimizer.track_frame refusing a prior list that does not
match the detections, or a prior without a pose, before anything touches a device."""
from __future__ import annotations

import re
import subprocess
import types

import numpy as np
import pytest

from test_abi_cpu import declared_functions

NAME = "dsr_tracker_track_frame"
CAM = dict(width=8, height=6, fx=10.0, fy=10.0, cx=3.5, cy=2.5)


def test_header_declares_and_library_exports_the_entry_point():
    from reconstruct import _libdsr as L

    lib = L.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", L.lib_path()], capture_output=True, text=True, check=True).stdout
    assert NAME in declared_functions() and NAME in L.SIGNATURES and NAME in L.BY_SYMBOL
    assert hasattr(lib, NAME)
    assert re.search(rf"\bT {NAME}$", out, flags=re.M)
    assert len(L.SIGNATURES[NAME][1]) == 8
    assert lib.dsr_abi_version() == L.ABI_VERSION == 12


def test_a_null_handle_is_refused():
    from reconstruct import _libdsr as L
    from reconstruct import utils as U

    lib = L.load_library()
    depth, inst = np.ones((6, 8), np.float32), np.zeros((6, 8), np.int32)
    dets = (L.FrameDet * 1)()
    pri = (L.TrackDet * 1)()
    assert lib.dsr_tracker_track_frame(None, U.frame_camera(CAM), U.frame_params(), L.fptr(depth), L.iptr(inst), 1,
                                       dets, pri) == -2
    assert lib.dsr_tracker_track_frame(None, None, None, None, None, 0, None, None) == -2


class _NoDevice:
    """Stands where the tracker's handle and decoder are: any use of it is a device call."""

    def __getattr__(self, name):
        raise AssertionError(f"track_frame touched {name} before refusing its arguments")


@pytest.mark.parametrize("n_priors", [0, 1, 3])
def test_track_frame_refuses_a_prior_count_mismatch_before_any_device_call(n_priors):
    from reconstruct.optimizer import Optimizer
    from reconstruct.tracker import ObjectTracker

    depth, inst = np.ones((6, 8), np.float32), np.zeros((6, 8), np.int32)
    dets = [dict(label=0, code=np.zeros(64, np.float32))] * 2
    priors = [(1.0, np.eye(4, dtype=np.float32))] * n_priors
    with pytest.raises(ValueError):
        ObjectTracker.track_frame(_NoDevice(), depth, inst, dets, priors, CAM)
    with pytest.raises(ValueError):
        Optimizer.track_frame(_NoDevice(), depth, inst, dets, priors, CAM, max_pts=16)


def test_track_frame_refuses_a_prior_without_a_pose_before_any_device_call():
    from reconstruct.tracker import ObjectTracker

    depth, inst = np.ones((6, 8), np.float32), np.zeros((6, 8), np.int32)
    dets = [dict(label=0, code=np.zeros(64, np.float32))] * 2
    for priors in ([(1.0, np.eye(4, dtype=np.float32)), 1.0], [(1.0, None), (1.0, np.eye(4, dtype=np.float32))]):
        with pytest.raises(ValueError):
            ObjectTracker.track_frame(_NoDevice(), depth, inst, dets, priors, CAM)


def test_track_frame_refuses_unknown_parameters():
    from reconstruct.tracker import ObjectTracker

    stub = types.SimpleNamespace(code_len=64, decoder=_NoDevice())
    depth, inst = np.ones((6, 8), np.float32), np.zeros((6, 8), np.int32)
    dets = [dict(label=0, code=np.zeros(64, np.float32))]
    with pytest.raises(TypeError):
        ObjectTracker.track_frame(stub, depth, inst, dets, [(1.0, np.eye(4))], CAM, dict(max_bg=3))
