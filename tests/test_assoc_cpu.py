"""Data association (dsr_scene_associate_*, dsr_assoc_*; include/dsr.h) without a
GPU: the test scene against the float64 oracle decoder alone, the host twins (dsr_assoc_pick_host,
dsr_assoc_points_host) against the numpy restatement (tests/assoc_oracle.py), their argument
errors, the structs against their ctypes mirrors and the exported symbols."""
from __future__ import annotations

import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import assoc_cases as AC
import assoc_oracle as AO
import frame_cases as FC
import frame_oracle as FO
import lidar_oracle as LO
import scene_oracle as SO
from conftest import REPO

HDR = os.path.join(REPO, "include", "dsr.h")
SYMBOLS = ("dsr_assoc_params_default", "dsr_scene_associate_frame", "dsr_scene_associate_points",
           "dsr_assoc_points_host", "dsr_assoc_pick_host")
STRUCTS = {"dsr_assoc_params": "AssocParams", "dsr_assoc_out": "AssocOut"}
P = dict(far=10.0, min_mask_area=100, max_pts=64)


@pytest.fixture(scope="module")
def dec64(full_layers):
    from oracle.dsr_oracle import Decoder

    return Decoder(full_layers, 64, (4,), dtype=np.float64)


def load():
    from reconstruct import _libdsr as L

    return L, L.load_library()


def rigid(seed=3, t=(0.4, -1.2, 2.5)):
    T = np.eye(4)
    T[:3, :3] = SO.rotation(seed)
    T[:3, 3] = t
    return T.astype(np.float32)


def test_symbols_exported_declared_and_abi_unchanged():
    L, lib = load()
    out = subprocess.run(["nm", "-D", "--defined-only", L.lib_path()], capture_output=True, text=True,
                         check=True).stdout
    hdr = open(HDR).read()
    for f in SYMBOLS:
        assert hasattr(lib, f), f
        assert re.search(rf"\bT {f}$", out, flags=re.M), f
        assert f in L.SIGNATURES and f in L.BY_SYMBOL, f
        assert re.search(rf"^int {f}\(", hdr, flags=re.M), f
    assert lib.dsr_abi_version() == 12 == L.ABI_VERSION
    assert "#define DSR_ABI_VERSION 12" in hdr
    for name, value in (("DSR_ASSOC_MATCHED", L.ASSOC_MATCHED), ("DSR_ASSOC_NEW", L.ASSOC_NEW),
                        ("DSR_ASSOC_NO_POINTS", L.ASSOC_NO_POINTS)):
        assert re.search(rf"\b{name} = {value}\b", hdr), name
    assert (AO.MATCHED, AO.NEW, AO.NO_POINTS) == (L.ASSOC_MATCHED, L.ASSOC_NEW, L.ASSOC_NO_POINTS)


def test_struct_layouts_match_ctypes():
    L, _ = load()
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HDR}"', "int main(void){"]
    for cname, pyname in STRUCTS.items():
        lines.append(f'printf("{pyname} size %zu\\n", sizeof({cname}));')
        for fld, _ in getattr(L, pyname)._fields_:
            lines.append(f'printf("{pyname} {fld} %zu\\n", offsetof({cname}, {fld}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c99", "-o", exe, src], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    seen = 0
    for line in out.strip().splitlines():
        py, what, val = line.split()
        cls = getattr(L, py)
        if what == "size":
            assert ctypes.sizeof(cls) == int(val), line
        else:
            assert getattr(cls, what).offset == int(val), line
        seen += 1
    assert seen == sum(1 + len(getattr(L, p)._fields_) for p in STRUCTS.values())


def test_defaults():
    from reconstruct import utils as U

    p = U.assoc_params()
    assert (p.inlier_tol, p.min_hits, p.min_pct) == (np.float32(0.05), 20, 50)
    assert (p.inlier_tol, p.min_hits, p.min_pct) == tuple(np.float32(v) if k == "inlier_tol" else v
                                                          for k, v in AO.DEFAULTS.items())
    _, lib = load()
    assert lib.dsr_assoc_params_default(None) == -2


def test_the_scene_is_the_one_the_gpu_tests_rely_on(dec64):
    """counts, tables, decisions and both margins of the issue's scene, on the restatement alone"""
    recs = AC.assert_conditions(dec64)
    assert (recs[1]["n_hit"], recs[1]["n_pts"]) == (41, 65)
    assert (recs[4]["n_hit"], recs[4]["second_hit"]) == (33, 32) and 100 * 33 > 50 * 65
    assert recs[5]["n_pts"] == 21


def test_pick_host_equals_the_numpy_pick_on_the_scene(dec64):
    from reconstruct import utils as U

    _, n_rows, _, (n_in, n_hit, n_neg) = AC.oracle(dec64)
    for kw in ({}, dict(min_hits=22), dict(min_hits=21), dict(min_pct=64), dict(min_pct=0, min_hits=1),
               dict(inlier_tol=0.01)):
        got = [dict(r) for r in U.assoc_pick(n_in, n_hit, n_neg, n_rows, **kw)]
        assert got == AO.pick(n_in, n_hit, n_neg, n_rows, **kw), kw
    # det 5 has 21 hits: matched at min_hits 21, new at 22
    assert U.assoc_pick(n_in, n_hit, n_neg, n_rows, min_hits=21)[5].status == AO.MATCHED
    r = U.assoc_pick(n_in, n_hit, n_neg, n_rows, min_hits=22)[5]
    assert (r.status, r.obj, r.n_hit, r.second) == (AO.NEW, -1, 21, 0)


def test_pick_host_on_hand_made_tables():
    from reconstruct import utils as U

    #          ties -> lower index   runner-up tie     all zero        one clear winner   66 objects
    n_hit = np.zeros((6, 66), np.int32)
    n_hit[0, [5, 9, 40]] = 30
    n_hit[1, 7], n_hit[1, [3, 65]] = 50, 25
    n_hit[3, 64] = 60
    n_hit[4, :] = 20
    n_hit[5, 65], n_hit[5, 0] = 40, 39
    n_in = n_hit + np.arange(66, dtype=np.int32)[None, :]
    n_neg = (np.arange(6 * 66, dtype=np.int32).reshape(6, 66) % 3)
    n_rows = np.asarray([59, 100, 10, 119, 39, 80], np.int32)
    got = U.assoc_pick(n_in, n_hit, n_neg, n_rows)
    assert [dict(r) for r in got] == AO.pick(n_in, n_hit, n_neg, n_rows)
    assert (got[0].obj, got[0].second, got[0].second_hit) == (5, 9, 30)
    assert (got[1].status, got[1].second, got[1].second_hit) == (AO.NEW, 3, 25)          # 100 * 50 == 50 * 100: not >
    assert (got[2].status, got[2].n_hit, got[2].second) == (AO.NEW, 0, 1)
    assert (got[3].status, got[3].obj, got[3].n_in) == (AO.MATCHED, 64, 60 + 64)         # 100 * 60 > 50 * 119
    assert (got[4].status, got[4].obj, got[4].second) == (AO.MATCHED, 0, 1)              # 2000 > 1950
    assert (got[5].status, got[5].second, got[5].second_hit) == (AO.NEW, 0, 39)          # 4000 == 50 * 80
    # min_pct at exact equality: 100 * 50 > 49 * 100 but not > 50 * 100
    assert U.assoc_pick(n_in, n_hit, n_neg, n_rows, min_pct=49)[1].status == AO.MATCHED
    assert U.assoc_pick(n_in, n_hit, n_neg, n_rows, min_pct=50)[1].status == AO.NEW
    # one object: no runner-up; a zero-object map: all new or without points, empty tables
    one = U.assoc_pick([[3]], [[3]], [[0]], [4], min_hits=3)
    assert dict(one[0]) == AO.pick([[3]], [[3]], [[0]], [4], min_hits=3)[0]
    assert (one[0].status, one[0].obj, one[0].second, one[0].second_hit) == (AO.MATCHED, 0, -1, 0)
    empty = np.zeros((3, 0), np.int32)
    none = U.assoc_pick(empty, empty, empty, [12, 0, 1])
    assert [dict(r) for r in none] == AO.pick(empty, empty, empty, [12, 0, 1])
    assert [(r.status, r.obj, r.second, r.n_hit) for r in none] == [(AO.NEW, -1, -1, 0), (AO.NO_POINTS, -1, -1, 0),
                                                                    (AO.NEW, -1, -1, 0)]


def test_points_host_is_the_numpy_restatement():
    from reconstruct import utils as U

    depth, inst = FC.base_frame()
    labels = [1, 2, 3, 77, 4, 1]                # ok (capped), ok, no depth, absent, small mask, a label twice
    T = rigid()
    before = LO.SUSPECTS
    for params in (P, dict(P, max_pts=5000), dict(P, max_pts=1)):
        pts, n_rows, recs = U.assoc_points(depth, inst, labels, FC.CAM, T, **params)
        q = dict(params, max_bg=0, downsample=1, expand=0)
        _, hrecs = U.frame_inputs(depth, inst, [FC.det(label) for label in labels], FC.CAM, **q)
        assert recs == hrecs
        assert [r.status for r in recs] == [0, 0, 3, 1, 2, 0]
        rows = [FO.ingest(depth, inst, FC.det(label), FC.CAM, **q)[0] for label in labels]
        want, want_rows = AO.strided(rows, params["max_pts"], T)
        assert np.array_equal(n_rows, want_rows) and list(n_rows) == [r.n_pts for r in recs]
        assert pts.shape == (len(labels), params["max_pts"], 3)
        assert np.array_equal(FC.bits(pts.reshape(-1, 3)), FC.bits(want))                # NaN fill included
        assert np.isnan(pts[2]).all() and np.isnan(pts[3]).all() and np.isnan(pts[4]).all()
        assert not np.isnan(pts[0, :n_rows[0]]).any()
    assert n_rows[0] == 1
    assert LO.SUSPECTS == before                # the fp64 emulation of fmaf met no double rounding


def test_host_argument_errors():
    L, lib = load()
    from reconstruct import utils as U

    depth, inst = FC.base_frame()
    cam, fp = U.frame_camera(FC.CAM), U.frame_params(**P)
    lab = np.asarray([1, 2], np.int32)
    T = rigid().reshape(16)
    pts = np.zeros((2, 64, 3), np.float32)
    n_rows = np.zeros(2, np.int32)
    good = [cam, fp, L.fptr(T), L.fptr(depth), L.iptr(inst), 2, L.iptr(lab), L.fptr(pts), L.iptr(n_rows), None]
    assert lib.dsr_assoc_points_host(*good) == 0
    for k in (0, 1, 2, 3, 4, 6, 7, 8):
        args = list(good)
        args[k] = None
        assert lib.dsr_assoc_points_host(*args) == -2, k
    for n in (0, -1):
        assert lib.dsr_assoc_points_host(*(good[:5] + [n] + good[6:])) == -2
    for bad in (dict(FC.CAM, fx=0.0), dict(FC.CAM, fy=float("nan")), dict(FC.CAM, width=0), dict(FC.CAM, height=-3)):
        c = L.Camera(bad["width"], bad["height"], bad["fx"], bad["fy"], bad["cx"], bad["cy"])
        assert lib.dsr_assoc_points_host(*([c] + good[1:])) == -2, bad
    assert lib.dsr_assoc_points_host(*([good[0], U.frame_params(**dict(P, max_pts=0))] + good[2:])) == -2
    row, mirror, nan, shear, inf = (rigid() for _ in range(5))
    row[3, 3] = 2.0
    mirror[:3, 0] *= -1.0
    nan[1, 1] = np.nan
    shear[0, 1] += 0.01
    inf[2, 3] = np.inf
    for t in (row, mirror, nan, shear, inf):
        t = np.ascontiguousarray(t.reshape(16))
        assert lib.dsr_assoc_points_host(*(good[:2] + [L.fptr(t)] + good[3:])) == -2
    with pytest.raises(L.DsrError):
        U.assoc_points(depth, inst, [1], FC.CAM, shear, **P)
    with pytest.raises(TypeError):
        U.assoc_points(depth, inst, [1], FC.CAM, rigid(), max_bg=3)
    # the pick
    tab = np.zeros(3 * 2 * 3, np.int32)
    out = (L.AssocOut * 2)()
    ok = U.assoc_params()
    good = [ok, 2, 3, L.iptr(tab), L.iptr(n_rows), out]
    assert lib.dsr_assoc_pick_host(*good) == 0
    for k in (0, 3, 4, 5):
        args = list(good)
        args[k] = None
        assert lib.dsr_assoc_pick_host(*args) == -2, k
    assert lib.dsr_assoc_pick_host(ok, 0, 3, L.iptr(tab), L.iptr(n_rows), out) == -2
    assert lib.dsr_assoc_pick_host(ok, 2, -1, L.iptr(tab), L.iptr(n_rows), out) == -2
    assert lib.dsr_assoc_pick_host(ok, 2, 0, None, L.iptr(n_rows), out) == 0
    assert lib.dsr_assoc_pick_host(ok, 2, 3, L.iptr(tab), L.iptr(np.asarray([1, -1], np.int32)), out) == -2
    for kw in (dict(inlier_tol=0.0), dict(inlier_tol=-1.0), dict(inlier_tol=float("nan")), dict(inlier_tol=float("inf")),
               dict(min_hits=0), dict(min_pct=-1), dict(min_pct=100)):
        assert lib.dsr_assoc_pick_host(U.assoc_params(**kw), 2, 3, L.iptr(tab), L.iptr(n_rows), out) == -2, kw
    for kw in (dict(min_pct=0), dict(min_pct=99), dict(min_hits=1), dict(inlier_tol=1e-6)):
        assert lib.dsr_assoc_pick_host(U.assoc_params(**kw), 2, 3, L.iptr(tab), L.iptr(n_rows), out) == 0, kw
    with pytest.raises(TypeError):
        U.assoc_params(tol=0.1)
    # the device entry points without a handle
    assert lib.dsr_scene_associate_frame(None, cam, fp, ok, L.fptr(T), L.fptr(depth), L.iptr(inst), 2, L.iptr(lab),
                                         out, None) == -2
    assert lib.dsr_scene_associate_points(None, ok, None, 2, 64, L.iptr(n_rows), L.fptr(pts), out, None) == -2
