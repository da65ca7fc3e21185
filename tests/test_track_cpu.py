"""The resident object tracker without a GPU: the host rule of a sweep call's
start pose (dsr_lidar_track_prep_host) against its restatement in python floats, bitwise, and
against the ingest's own t_cam_obj; the header, the exports and the ctypes layouts of the new
structs (the method of test_abi_cpu.py); and ObjectTracker failing loudly without a device."""
from __future__ import annotations

import ctypes
import math
import os
import re
import subprocess
import tempfile
import types

import numpy as np
import pytest

import lidar_cases as LC
import track_oracle as TO
from test_abi_cpu import HDR, declared_functions

NEW = ("dsr_tracker_create", "dsr_tracker_destroy", "dsr_tracker_track", "dsr_tracker_track_lidar",
       "dsr_tracker_query", "dsr_tracker_download", "dsr_lidar_track_prep_host")
TCV = LC.t_cam_velo(yaw=0.3, pitch=-0.2, t=(0.4, -0.3, 1.1))
THETAS = (0.0, 0.4, 1.3, 2.0, 3.0, -0.4, -1.3, -2.0, -3.0)      # 0 and two per quadrant


def dets():
    rng = np.random.default_rng(31)
    out = []
    for th in THETAS:
        x, y, z = rng.uniform(-20, 20), rng.uniform(-20, 20), rng.uniform(-2, 0)
        w, l, h = rng.uniform(1.4, 2.6), rng.uniform(3.0, 12.0), rng.uniform(1.3, 3.5)
        out.append(dict(trans=(x, y, z), size=(w, l, h), theta=th))
    return out


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("margin", [1.0, 1.1])
def test_prep_equals_its_restatement(margin):
    from reconstruct import utils as U

    d = dets()
    assert {(math.cos(t) > 0, math.sin(t) > 0) for t in THETAS[1:]} == {(a, b) for a in (True, False) for b in (True, False)}
    t, sc = U.lidar_track_prep(d, TCV, box_margin=margin)
    assert t.shape == (9, 4, 4) and sc.shape == (9,) and t.dtype == sc.dtype == np.float32
    for i, det in enumerate(d):
        to, so = TO.track_prep(det, TCV, margin)
        assert np.array_equal(bits(t[i]), bits(to)), i
        assert bits(sc[i]) == bits(so), i
        assert np.array_equal(t[i][3], np.array([0, 0, 0, 1], np.float32))


@pytest.mark.parametrize("margin", [1.0, 1.1])
def test_prep_decomposes_the_ingests_pose(margin):
    """Independent of the restatement: scale x rotation (fp64 product of the two stored float32
    values) is the rule's t_cam_obj to within 4 * 2^-24 * sum |terms| per entry — the bound form
    DESIGN.md §3.5d uses for a re-ordered fp32 sum — and the translation is the same float."""
    from reconstruct import utils as U

    d = dets()
    t, sc = U.lidar_track_prep(d, TCV, box_margin=margin)
    rc, _, _, _, recs = LC.run("host", np.zeros((0, 3), np.float32), LC.blank(), [], d, LC.CAM, TCV, dict(box_margin=margin))
    assert rc == 0
    worst = 0.0
    for i, det in enumerate(d):
        ref = np.asarray(recs[i].t_cam_obj, np.float32).reshape(4, 4)
        got = t[i, :3, :3].astype(np.float64) * float(sc[i])
        bound = 4.0 * 2.0 ** -24 * TO.t_cam_obj_terms(det, TCV, margin)
        err = np.abs(got - ref[:3, :3].astype(np.float64))
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert np.all(err <= bound), (i, err, bound)
        assert np.array_equal(bits(t[i, :, 3]), bits(ref[:, 3])), i
        # SE(3): the rotation block is orthonormal to float32 rounding
        R = t[i, :3, :3].astype(np.float64)
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(R) - 1.0) < 1e-6
    print("largest share of the bound", worst)


def test_prep_argument_errors():
    from reconstruct import _libdsr as L
    from reconstruct import utils as U

    lib = L.load_library()
    d = dets()[:2]
    ld, keep = U.lidar_dets(d)
    p = U.lidar_params()
    tcv = np.ascontiguousarray(TCV.reshape(16))
    t, sc = np.zeros((2, 16), np.float32), np.zeros(2, np.float32)
    call = lambda p=p, tcv=tcv, n=2, ld=ld, t=t, sc=sc: lib.dsr_lidar_track_prep_host(  # noqa: E731
        p, L.fptr(tcv) if tcv is not None else None, n, ld, L.fptr(t), L.fptr(sc))
    assert call() == 0
    assert call(n=0) == 0
    assert call(p=None) < 0 and call(tcv=None) < 0 and call(ld=None) < 0 and call(t=None) < 0 and call(sc=None) < 0
    assert call(n=-1) < 0
    assert call(tcv=np.ascontiguousarray((TCV * 2.0).reshape(16))) < 0          # not rigid
    assert call(p=U.lidar_params(box_margin=0.0)) < 0
    assert call(p=U.lidar_params(radius=0.0, max_pts=0, max_bg=-1)) == 0        # fields that are not read
    bad, _ = U.lidar_dets([dict(d[0], size=(1.0, 0.0, 1.0)), d[1]])
    assert call(ld=bad) < 0
    bad, _ = U.lidar_dets([d[0], dict(d[1], theta=float("nan"))])
    assert call(ld=bad) < 0
    with pytest.raises(L.DsrError):
        U.lidar_track_prep([dict(d[0], theta=float("inf"))], TCV)


def test_header_declares_and_library_exports_the_tracker():
    from reconstruct import _libdsr as L

    lib = L.load_library()
    fns = declared_functions()
    out = subprocess.run(["nm", "-D", "--defined-only", L.lib_path()], capture_output=True, text=True, check=True).stdout
    for f in NEW:
        assert f in fns and f in L.SIGNATURES and f in L.BY_SYMBOL, f
        assert hasattr(lib, f), f
        assert re.search(rf"\bT {f}$", out, flags=re.M), f
    assert lib.dsr_abi_version() == L.ABI_VERSION == 12


STRUCTS = {"dsr_track_out": "TrackOut", "dsr_track_det": "TrackDet"}


def test_struct_layouts_match_ctypes():
    from reconstruct import _libdsr as L

    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HDR}"', "int main(void){"]
    for cname, pyname in STRUCTS.items():
        lines.append(f'printf("{pyname} size %zu\\n", sizeof({cname}));')
        for fld, _ in getattr(L, pyname)._fields_:
            lines.append(f'printf("{pyname} {fld} %zu\\n", offsetof({cname}, {fld}));')
    lines.append('printf("enum %d %d %d\\n", DSR_TRACK_OK, DSR_TRACK_NO_POINTS, DSR_TRACK_NO_INLIERS);')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "layout.c")
        exe = os.path.join(d, "layout")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c99", "-o", exe, src], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    n = 0
    for line in out.strip().splitlines():
        py, what, *val = line.split()
        if py == "enum":
            assert [int(what)] + [int(v) for v in val] == [L.TRACK_OK, L.TRACK_NO_POINTS, L.TRACK_NO_INLIERS]
            continue
        cls = getattr(L, py)
        if what == "size":
            assert ctypes.sizeof(cls) == int(val[0]), line
        else:
            assert getattr(cls, what).offset == int(val[0]), line
        n += 1
    assert n == 2 + 5 + 3


def test_tracker_fails_loudly_without_a_device_or_a_decoder():
    """No CPU fallback: without a gfx950 device the context cannot be created, and with one a
    tracker without a decoder is refused — DsrError either way."""
    from reconstruct import _libdsr as L
    from reconstruct.tracker import ObjectTracker

    class NoDecoder:
        handle = None

        @property
        def ctx(self):
            return L.Context.get()

    opt = types.SimpleNamespace(decoder=NoDecoder(), code_len=64, params=L.OptimParams())
    with pytest.raises(L.DsrError):
        ObjectTracker(opt, 4, 256)
