"""Frame ingest without a GPU: dsr_frame_params_default, the new struct layouts,
dsr_frame_inputs_host against the numpy restatement of the rule (tests/frame_oracle.py) on
synthetic frames (tests/frame_cases.py), its argument errors, and reconstruct.utils.frame_inputs.
Every comparison is bitwise."""
from __future__ import annotations

import ctypes
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import REPO, make_cfg

import frame_cases as FC
import frame_oracle as FO

HDR = os.path.join(REPO, "include", "dsr.h")


@pytest.fixture(scope="module")
def cases():
    return FC.cases()


def test_frame_params_default():
    from reconstruct import _libdsr as L

    p = L.FrameParams()
    assert L.load_library().dsr_frame_params_default(p) == 0
    assert (p.max_pts, p.max_bg, p.downsample, p.expand, p.min_mask_area) == (250, 200, 4, 5, 1000)
    assert p.near == np.float32(0.01) and math.isinf(p.far) and p.far > 0
    assert L.load_library().dsr_frame_params_default(None) < 0
    assert FO.DEFAULTS == dict(max_pts=250, max_bg=200, downsample=4, expand=5, min_mask_area=1000, near=0.01,
                               far=np.inf)


STRUCTS = {"dsr_frame_params": "FrameParams", "dsr_frame_det": "FrameDet", "dsr_frame_det_out": "FrameDetOut"}


def test_frame_struct_layouts_match_ctypes():
    from reconstruct import _libdsr as L

    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HDR}"', "int main(void){"]
    for cname, pyname in STRUCTS.items():
        lines.append(f'printf("{pyname} size %zu\\n", sizeof({cname}));')
        for fld, _ in getattr(L, pyname)._fields_:
            lines.append(f'printf("{pyname} {fld} %zu\\n", offsetof({cname}, {fld}));')
    lines.append('printf("enum %d %d %d %d\\n", DSR_FRAME_OK, DSR_FRAME_NO_MASK, DSR_FRAME_SMALL_MASK, '
                 'DSR_FRAME_NO_DEPTH);')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c99", "-o", exe, src], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    seen = 0
    for line in out.strip().splitlines():
        if line.startswith("enum"):
            assert [int(x) for x in line.split()[1:]] == [L.FRAME_OK, L.FRAME_NO_MASK, L.FRAME_SMALL_MASK,
                                                          L.FRAME_NO_DEPTH] == [0, 1, 2, 3]
            continue
        py, what, val = line.split()
        cls = getattr(L, py)
        if what == "size":
            assert ctypes.sizeof(cls) == int(val), line
        else:
            assert getattr(cls, what).offset == int(val), line
        seen += 1
    assert seen == sum(1 + len(getattr(L, n)._fields_) for n in STRUCTS.values())


def test_sel_is_the_integer_rule_not_the_float_idiom():
    """N = 1080, n = 250: np.linspace(0, N-1, n).astype(int32) lands below the integer rule in some
    entries (fp64 i * step just under an integer); the specification is the integer rule."""
    exact = np.asarray(FO.sel(250, 1080))
    assert exact.tolist() == [(i * 1079) // 249 for i in range(250)]
    idiom = np.linspace(0, 1079, 250).astype(np.int32)
    assert (idiom != exact).sum() > 0
    assert np.all(idiom <= exact) and np.all(exact - idiom <= 1)


CASE_NAMES = ["cap_hit", "cap_not_hit", "n1080", "borders", "boxes", "downsample1", "downsample1_cap", "gh1", "gh0",
              "max_bg0", "dup_label", "absent", "area_eq", "area_plus1", "no_depth", "one_pt", "n_det0", "nine"]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_host_equals_oracle(cases, name):
    (depth, inst), cam, dets, params = cases[name]
    res = FC.run("host", depth, inst, cam, dets, params)
    FC.assert_matches_oracle(depth, inst, cam, dets, params, res)


def test_case_list_is_complete(cases):
    assert sorted(CASE_NAMES) == sorted(cases)


def test_cases_take_the_paths_they_are_named_for(cases):
    """The fixtures hit what they claim: caps, statuses, grids, the 1080 / 250 entries."""
    def recs(name):
        (depth, inst), cam, dets, params = cases[name]
        return FC.run("host", depth, inst, cam, dets, params), params

    (rc, pts, rays, dobs, r), p = recs("cap_hit")
    assert r[0].status == 0 and r[0].n_valid > 250 and r[0].n_pts == 250 and r[0].n_bg == 200
    (_, _, _, _, r), p = recs("cap_not_hit")
    assert all(x.n_pts == x.n_valid < 5000 and 0 < x.n_bg < 3000 for x in r)
    (_, pts, _, dobs, r), p = recs("n1080")
    assert r[0].n_valid == 1080 and r[0].n_pts == 250
    (depth, inst), cam, _, _ = cases["n1080"]
    z = depth[(inst == 1) & (depth == depth) & (depth > 0.01) & (depth < 10.0)]     # row-major valid depths
    assert np.array_equal(dobs[0], z[np.asarray(FO.sel(250, 1080))])
    assert not np.array_equal(dobs[0], z[np.linspace(0, 1079, 250).astype(np.int32)])
    (_, _, _, _, r), p = recs("borders")
    assert r[0].box == (0, 0, FC.W - 1, FC.H - 1) and r[0].status == 0
    (_, _, _, _, r), p = recs("boxes")
    assert r[0].box != r[1].box and r[2].box[0] == 0 and r[2].box[1] == 0 and r[2].box[3] == FC.H - 1
    assert r[3].box[2] == FC.W - 1 and r[4].box == (0, 0, -1, -1) and r[4].n_bg == 0 and r[5].box == (0, 0, -1, -1)
    (_, _, _, _, r), p = recs("gh1")
    assert r[0].grid_h == 1 and r[0].grid_w == 2 and r[0].n_bg == 1 and r[1] == r[0]
    (_, _, _, _, r), p = recs("gh0")
    assert (r[0].grid_h, r[1].grid_w) == (0, 0) and r[0].n_bg == r[1].n_bg == 0 and r[0].n_pts > 0
    (_, _, _, _, r), p = recs("max_bg0")
    assert all(x.n_bg == 0 and x.n_pts > 0 for x in r)
    (_, pts, rays, _, r), p = recs("dup_label")
    assert r[0] == r[2] and np.array_equal(pts[0], pts[2]) and np.array_equal(rays[0], rays[2])
    (_, _, _, _, r), p = recs("absent")
    assert [x.status for x in r] == [1, 0, 1] and r[0].box == (0, 0, -1, -1) and r[2].grid_h > 0
    assert r[0].n_pts == r[2].n_pts == r[2].n_bg == 0
    (_, _, _, _, r), p = recs("area_eq")
    assert r[0].status == 2 and r[0].n_mask == p["min_mask_area"] and r[0].n_pts == 0
    (_, _, _, _, r), p = recs("area_plus1")
    assert r[0].status == 0 and r[0].n_mask == p["min_mask_area"] + 1
    (_, _, _, _, r), p = recs("no_depth")
    assert r[0].status == 3 and r[0].n_mask > 0 and r[0].n_valid == 0 and r[0].n_pts == r[0].n_bg == 0
    (_, _, _, _, r), p = recs("downsample1")
    assert r[0].grid_h == r[0].box[3] - r[0].box[1] + 1 and r[0].n_bg > 200
    (_, _, _, _, r), p = recs("downsample1_cap")
    assert r[0].n_bg == 37
    (_, _, _, _, r), p = recs("one_pt")
    assert (r[0].n_pts, r[0].n_bg) == (1, 1)


def test_argument_errors_return_negative():
    from reconstruct import _libdsr as L
    from reconstruct import utils as U

    lib = L.load_library()
    depth, inst = FC.base_frame()
    dets, keep = U.frame_dets([FC.det(1)])
    out = (L.FrameDetOut * 1)()

    def call(cam=None, depth_=depth, inst_=inst, n=1, dets_=dets, **params):
        cam = U.frame_camera(dict(FC.CAM, **(cam or {})))
        p = U.frame_params(**dict(dict(max_pts=8, max_bg=8), **params))
        pts, rays, dobs = np.zeros((1, 8, 3), np.float32), np.zeros((1, 16, 3), np.float32), np.zeros((1, 8), np.float32)
        return lib.dsr_frame_inputs_host(cam, p, L.fptr(depth_), L.iptr(inst_), n, dets_, L.fptr(pts), L.fptr(rays),
                                         L.fptr(dobs), out)

    assert call() == 0
    assert call(depth_=None) < 0 and call(inst_=None) < 0
    assert call(cam=dict(width=0)) < 0 and call(cam=dict(height=-3)) < 0
    assert call(cam=dict(fx=0.0)) < 0 and call(cam=dict(fy=-1.0)) < 0 and call(cam=dict(fx=float("nan"))) < 0
    assert call(max_pts=0) < 0 and call(max_bg=-1) < 0 and call(downsample=0) < 0 and call(expand=-1) < 0
    assert call(n=-1) < 0 and call(dets_=None) < 0
    assert lib.dsr_frame_inputs_host(None, None, None, None, 0, None, None, None, None, None) < 0
    assert call(max_bg=0) == 0 and call(expand=0) == 0 and call(downsample=1) == 0


def test_frame_inputs_feeds_object_in(cases):
    """utils.frame_inputs: trimmed arrays whose shapes, dtypes and counts agree with the records
    and go into Optimizer._object_in unchanged."""
    import synthetic as S
    from reconstruct import utils as U
    from reconstruct.optimizer import Optimizer

    (depth, inst), cam, dets, params = cases["absent"]
    code = np.linspace(-0.1, 0.1, 64).astype(np.float32)
    dets = [dict(d, code=code if i == 1 else None) for i, d in enumerate(dets)]
    objects, records = U.frame_inputs(depth, inst, dets, cam, **params)
    assert len(objects) == len(records) == 3
    opt = Optimizer(None, make_cfg(S.KITTI_OPTIM))
    for i, ((t, pts, rays, dobs, c), r) in enumerate(zip(objects, records)):
        opts, orays, odobs, orec = FO.ingest(depth, inst, dets[i], cam, **params)
        assert dict(r, box=tuple(r.box)) == orec
        assert pts.shape == (r.n_pts, 3) and rays.shape == (r.n_pts + r.n_bg, 3) and dobs.shape == (r.n_pts,)
        assert pts.dtype == rays.dtype == dobs.dtype == np.float32 and t.shape == (4, 4)
        assert np.array_equal(FC.bits(pts), FC.bits(opts)) and np.array_equal(FC.bits(rays), FC.bits(orays))
        assert np.array_equal(FC.bits(dobs), FC.bits(odobs))
        keep = []
        rec = opt._object_in(t, pts, rays, dobs, c, keep)
        assert (rec.n_pts, rec.n_rays, rec.n_depth) == (r.n_pts, r.n_pts + r.n_bg, r.n_pts)
        for held, mine in zip(keep[:3], (pts, rays, dobs)):                  # no copy, no conversion
            assert mine.size == 0 or np.shares_memory(held, mine)
        assert (c is None) == (i != 1)
    assert records[0].status == 1 and records[1].status == 0
    with pytest.raises(TypeError):
        U.frame_inputs(depth, inst, dets, cam, max_points=3)
    with pytest.raises(ValueError):
        U.frame_inputs(depth[:-1], inst, dets, cam)
