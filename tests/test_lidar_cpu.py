"""LiDAR keyframe ingest without a GPU: dsr_lidar_params_default, the new struct
layouts, dsr_lidar_inputs_host against the numpy restatement of the rule (tests/lidar_oracle.py) on
synthetic sweeps (tests/lidar_cases.py) bitwise, its argument errors, reconstruct.utils.lidar_inputs,
and the rule against the reference's own get_detections output (tests/golden/f24_lidar_frame.npz,
written by tests/golden/make_lidar_frame.py) within derived bounds."""
from __future__ import annotations

import ctypes
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import REPO, make_cfg

import lidar_cases as LC
import lidar_oracle as LO

HDR = os.path.join(REPO, "include", "dsr.h")
U24 = 2.0 ** -24


@pytest.fixture(scope="module")
def cases():
    return LC.cases()


def test_lidar_params_default():
    from reconstruct import _libdsr as L

    p = L.LidarParams()
    assert L.load_library().dsr_lidar_params_default(p) == 0
    assert (p.max_pts, p.max_bg, p.downsample, p.expand, p.min_mask_area) == (250, 200, 4, 5, 1000)
    assert p.radius == np.float32(3.0) and p.box_margin == np.float32(1.1)
    assert L.load_library().dsr_lidar_params_default(None) < 0
    assert LO.DEFAULTS == dict(max_pts=250, max_bg=200, downsample=4, expand=5, min_mask_area=1000, radius=3.0,
                               box_margin=1.1)


STRUCTS = {"dsr_lidar_params": "LidarParams", "dsr_lidar_mask": "LidarMask", "dsr_lidar_det": "LidarDet",
           "dsr_lidar_det_out": "LidarDetOut"}


def test_lidar_struct_layouts_match_ctypes():
    from reconstruct import _libdsr as L

    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HDR}"', "int main(void){"]
    for cname, pyname in STRUCTS.items():
        lines.append(f'printf("{pyname} sizeof %zu\\n", sizeof({cname}));')
        for fld, _ in getattr(L, pyname)._fields_:
            lines.append(f'printf("{pyname} {fld} %zu\\n", offsetof({cname}, {fld}));')
    lines.append('printf("enum %d %d %d %d %d %d\\n", DSR_LIDAR_OK, DSR_LIDAR_BEHIND, DSR_LIDAR_NO_POINTS, '
                 'DSR_LIDAR_NO_MATCH, DSR_LIDAR_SMALL_MASK, DSR_LIDAR_MAX_MASKS);')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c99", "-o", exe, src], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    seen = 0
    for line in out.strip().splitlines():
        if line.startswith("enum"):
            assert [int(x) for x in line.split()[1:]] == [L.LIDAR_OK, L.LIDAR_BEHIND, L.LIDAR_NO_POINTS, L.LIDAR_NO_MATCH,
                                                          L.LIDAR_SMALL_MASK, L.LIDAR_MAX_MASKS] == [0, 1, 2, 3, 4, 256]
            assert [LO.OK, LO.BEHIND, LO.NO_POINTS, LO.NO_MATCH, LO.SMALL_MASK, LO.MAX_MASKS] == [0, 1, 2, 3, 4, 256]
            continue
        py, what, val = line.split()
        cls = getattr(L, py)
        if what == "sizeof":                                   # (dsr_lidar_det has a field called size)
            assert ctypes.sizeof(cls) == int(val), line
        else:
            assert getattr(cls, what).offset == int(val), line
        seen += 1
    assert seen == sum(1 + len(getattr(L, n)._fields_) for n in STRUCTS.values())


def test_emulated_fmaf_is_exact_and_flags_double_rounding():
    """The oracle's fmaf against exact rational arithmetic on random float32 triples, and its guard
    on a constructed double-rounding case."""
    from fractions import Fraction

    rng = np.random.default_rng(0)
    a, b, c = (rng.standard_normal(2000).astype(np.float32) * np.float32(10.0) ** rng.integers(-3, 4, 2000).astype(np.float32)
               for _ in range(3))
    before = LO.SUSPECTS
    got = LO.fmaf(a, b, c)
    flagged = LO.SUSPECTS - before
    wrong = 0
    for x, y, z, g in zip(a.tolist(), b.tolist(), c.tolist(), got.tolist()):
        exact = Fraction(x) * Fraction(y) + Fraction(z)
        lo, hi = np.nextafter(np.float32(g), np.float32(-np.inf)), np.nextafter(np.float32(g), np.float32(np.inf))
        # g is a nearest float32: no farther from the exact value than either neighbour
        d = abs(Fraction(g) - exact)
        wrong += not (d <= abs(Fraction(float(lo)) - exact) and d <= abs(Fraction(float(hi)) - exact))
    assert wrong == 0 and flagged == 0
    # an exact fp64 sum that sits half-way between two float32 values is not a double rounding
    before = LO.SUSPECTS
    r = LO.fmaf(np.float32(1.0), np.float32(2.0 ** -24), np.float32(1.0))           # 1 + 2^-24: ties to even
    assert LO.SUSPECTS == before and r == np.float32(1.0)
    # a b = (1 + 2^-20)(1 - 2^-20) = 1 - 2^-40, c = 2^24 + 2 (float32 ulp 2): exactly 2^24 + 3 - 2^-40, below
    # half-way, so one rounding gives 2^24 + 2; fp64 (ulp 2^-28) first rounds to 2^24 + 3, half-way, which
    # then goes to even, 2^24 + 4.  The guard must flag it.
    r = LO.fmaf(np.float32(1.0 + 2.0 ** -20), np.float32(1.0 - 2.0 ** -20), np.float32(2.0 ** 24 + 2))
    assert LO.SUSPECTS == before + 1 and r == np.float32(2.0 ** 24 + 4)
    LO.SUSPECTS = before


@pytest.mark.parametrize("name", LC.CASE_NAMES)
def test_host_equals_oracle(cases, name):
    c = cases[name]
    LC.assert_matches_oracle(*c, LC.run("host", *c))


def test_case_list_is_complete(cases):
    assert sorted(LC.CASE_NAMES) == sorted(cases)


def test_cases_take_the_paths_they_are_named_for(cases):
    """The fixtures hit what they claim: sizes, caps, faces, statuses, counts."""
    def recs(name):
        res = LC.run("host", *cases[name])
        assert res[0] == 0
        return res

    _, pts, rays, dobs, r = recs("scene")
    assert cases["scene"][0].shape == (5003, 4) and cases["scene_stride3"][0].shape == (5003, 3)
    assert [x.status for x in r] == [0, 0, 0] and [x.mask for x in r] == [0, 1, 2]
    assert r[0].n_crop == 700 and r[0].n_near > 700 and r[0].n_pts == 250 and r[1].n_crop > 250 and r[2].n_pts == r[2].n_crop < 250
    assert all(x.n_proj == x.n_pts == x.n_hits and 0 < x.n_bg <= 200 for x in r)
    assert np.all(dobs[0] > 0) and np.all(rays[0, :250, 2] == 1)
    _, _, _, _, r3 = recs("scene_stride3")
    assert [dict(x, t_cam_obj=0) for x in r3] == [dict(x, t_cam_obj=0) for x in r]    # the same points in another order
    _, _, _, _, r = recs("scene_nocap")
    assert [x.n_pts for x in r] == [x.n_crop for x in r] and r[0].n_pts == 700
    assert len(recs("nine")[4]) == 9 and recs("n_det0")[4] == []
    _, pts, _, _, r = recs("n_masks0")
    assert r[0].status == 3 and r[0].mask == -1 and r[0].n_hits == 0 and r[0].n_proj == 250 and r[0].n_bg == 0
    assert np.all(pts[0] != LC.SENTINEL)                                   # rows are written for every detection
    assert all(x.status == 0 and x.n_bg == 0 for x in recs("max_bg0")[4])
    _, _, _, _, r = recs("shared_mask")
    assert r[0].mask == r[1].mask == 0 and r[0].status == r[1].status == 0 and r[0].n_near != r[1].n_near
    _, _, _, _, r = recs("dup_label")
    assert [x.mask for x in r] == [0, 2] and r[0].box != (0, 0, 35, 35)
    _, _, _, _, r = recs("absent_from_grid")
    assert r[0].status == 0 and r[0].box == (0, 0, 35, 25) and r[0].n_bg == r[0].grid_h * r[0].grid_w
    assert r[1].box[2] == LC.W - 1 and r[1].box[3] == LC.H - 1 and r[1].n_bg == 200
    _, _, _, _, r = recs("area_eq")
    assert r[0].status == 4 and r[0].n_mask_px == cases["area_eq"][6]["min_mask_area"] and r[0].n_bg == 0 and r[0].n_pts == 250
    _, _, _, _, r = recs("area_plus1")
    assert r[0].status == 0 and r[0].n_mask_px == cases["area_plus1"][6]["min_mask_area"] + 1
    for n in (0, 1, 63, 64, 65, 257):
        assert cases[f"n_velo{n}"][0].shape[0] == n
        r = recs(f"n_velo{n}")[4]
        assert r[0].n_crop == min(n, 40) and r[0].status == (2 if n == 0 else 0)
    assert {cases[f"n_velo{n}"][0].shape[1] for n in (0, 1, 63, 64, 65, 257)} == {3, 4}
    for name, n_crop, n_pts in (("crop0", 0, 0), ("crop1", 1, 1), ("crop_eq", 250, 250), ("crop_plus1", 251, 250),
                                ("crop1080", 1080, 250)):
        r = recs(name)[4]
        assert (r[0].n_crop, r[0].n_pts, r[0].n_near) == (n_crop, n_pts, n_crop + 130), name
    # 1080 against 250: the integer sel differs from the float idiom
    assert (np.linspace(0, 1079, 250).astype(np.int32) != np.asarray(LO.FO.sel(250, 1080))).sum() > 0
    # faces: of 14 points 7 are near and 5 in (see lidar_cases: on a face is out, one ulp inside is in)
    _, pts, _, _, r = recs("faces")
    assert (r[0].n_near, r[0].n_crop, r[0].n_pts) == (7, 5, 5) and r[0].status == 0
    # association
    r = recs("tie")[4]
    assert (r[0].n_proj, r[0].n_hits, r[0].mask, r[0].status) == (8, 3, -1, 3)
    r = recs("half")[4]
    assert (r[0].n_proj, r[0].n_hits, r[0].mask, r[0].status) == (8, 4, -1, 3)
    r = recs("half_plus1")[4]
    assert (r[0].n_proj, r[0].n_hits, r[0].mask, r[0].status, r[0].n_mask_px) == (9, 5, 0, 0, 5)
    r = recs("fov")[4]
    assert 0 < r[0].n_proj < r[0].n_pts == 250 and r[0].status == 0
    _, _, _, dobs, r = recs("behind_rows")
    assert (dobs[0] <= 0).sum() > 0 and 0 < r[0].n_proj <= (dobs[0] > 0).sum() and r[0].status == 0 and r[0].n_bg == 0
    _, pts, _, _, r = recs("behind")
    assert [x.status for x in r] == [1, 0] and r[0].t_cam_obj[11] < 0 and r[0].n_pts == 100 and r[0].n_proj == 0
    assert np.all(pts[0, :100] != LC.SENTINEL)
    for name in ("image641x5", "image63x70"):
        r = recs(name)[4]
        assert all(x.status == 0 and x.mask == 1 and x.n_bg == 64 for x in r), name


def test_argument_errors_return_negative(cases):
    from reconstruct import _libdsr as L
    from reconstruct import utils as U

    lib = L.load_library()
    velo, inst, masks, dets, cam0, tcv0, params = cases["n_velo65"]
    out = (L.LidarDetOut * 1)()

    def call(cam=None, velo_=velo, inst_=inst, n_velo=None, stride=None, tcv=tcv0, n_masks=None, masks_=masks, n=1,
             det=None, dets_=True, **par):
        cam = U.frame_camera(dict(cam0, **(cam or {})))
        p = U.lidar_params(**dict(dict(max_pts=8, max_bg=8), **par))
        ld, keep = U.lidar_dets([dict(dets[0], **(det or {}))])
        ml = U.lidar_masks(masks_) if masks_ is not None else None
        pts, rays, dobs = np.zeros((1, 8, 3), np.float32), np.zeros((1, 16, 3), np.float32), np.zeros((1, 8), np.float32)
        t = None if tcv is None else np.ascontiguousarray(np.asarray(tcv, np.float32).reshape(16))
        return lib.dsr_lidar_inputs_host(cam, p, L.fptr(t), L.fptr(velo_), velo.shape[0] if n_velo is None else n_velo,
                                         velo.shape[1] if stride is None else stride, L.iptr(inst_),
                                         len(masks) if n_masks is None else n_masks, ml, n, ld if dets_ else None,
                                         L.fptr(pts), L.fptr(rays), L.fptr(dobs), out)

    assert call() == 0
    assert call(inst_=None) < 0 and call(velo_=None) < 0 and call(velo_=None, n_velo=0) == 0
    assert call(cam=dict(width=0)) < 0 and call(cam=dict(height=-3)) < 0
    assert call(cam=dict(fx=0.0)) < 0 and call(cam=dict(fy=-1.0)) < 0 and call(cam=dict(fx=float("nan"))) < 0
    assert call(max_pts=0) < 0 and call(max_bg=-1) < 0 and call(downsample=0) < 0 and call(expand=-1) < 0
    assert call(n=-1) < 0 and call(dets_=False) < 0
    # t_cam_velo: null, scaled, a reflection, a bad last row, a non-finite translation
    t = np.asarray(tcv0, np.float32).reshape(4, 4)
    scaled, mirror, row, inf = t.copy(), t.copy(), t.copy(), t.copy()
    scaled[:3, :3] *= np.float32(1.01)
    mirror[0, :3] *= -1
    row[3, 0] = 0.5
    inf[1, 3] = np.inf
    assert call(tcv=None) < 0 and call(tcv=scaled) < 0 and call(tcv=mirror) < 0 and call(tcv=row) < 0 and call(tcv=inf) < 0
    assert call(stride=2) < 0 and call(stride=0) < 0 and call(n_velo=-1) < 0 and call(n_velo=(1 << 24) + 1) < 0
    assert call(n_masks=-1) < 0 and call(n_masks=257) < 0 and call(masks_=None) < 0 and call(masks_=None, n_masks=0) == 0
    for bad in (float("nan"), float("inf")):
        assert call(det=dict(theta=bad)) < 0 and call(det=dict(trans=(bad, 0.0, 0.0))) < 0
        assert call(det=dict(size=(1.0, bad, 1.0))) < 0
        assert call(radius=bad) < 0 and call(box_margin=bad) < 0
    assert call(det=dict(size=(0.0, 1.0, 1.0))) < 0 and call(det=dict(size=(1.0, 1.0, -2.0))) < 0
    assert call(radius=0.0) < 0 and call(radius=-1.0) < 0 and call(box_margin=0.0) < 0 and call(box_margin=-1.1) < 0
    assert lib.dsr_lidar_inputs_host(None, None, None, None, 0, 3, None, 0, None, 0, None, None, None, None, None) < 0
    assert call(max_bg=0) == 0 and call(expand=0) == 0 and call(downsample=1) == 0 and call(n=0) == 0
    # 256 masks are accepted
    assert call(masks_=[(100 + j, None) for j in range(256)], n_masks=256) == 0


def test_lidar_inputs_feeds_object_in(cases):
    """utils.lidar_inputs: trimmed arrays whose shapes, dtypes and counts agree with the records
    and go into Optimizer._object_in unchanged; a detection that is not ok is an empty object."""
    import synthetic as S
    from reconstruct import utils as U
    from reconstruct.optimizer import Optimizer

    velo, inst, masks, dets, cam, tcv, params = cases["behind"]
    code = np.linspace(-0.1, 0.1, 64).astype(np.float32)
    dets = [dict(d, code=code if i == 1 else None) for i, d in enumerate(dets)]
    objects, records = U.lidar_inputs(velo, inst, masks, dets, cam, tcv, **params)
    rows = U.lidar_inputs(velo, inst, masks, [[*d["trans"], *d["size"], d["theta"], 0.9] for d in dets], cam, tcv, **params)
    assert rows[1] == records                                              # detector rows are accepted too
    assert len(objects) == len(records) == 2 and [r.status for r in records] == [1, 0]
    opt = Optimizer(None, make_cfg(S.KITTI_OPTIM))
    for i, ((t, pts, rays, dobs, c), r) in enumerate(zip(objects, records)):
        opts, orays, odobs, orec = LO.ingest(velo, inst, masks, dets[i], cam, tcv, **params)
        assert dict(r) == orec
        n_p, n_r = (r.n_pts, r.n_pts + r.n_bg) if r.status == 0 else (0, 0)
        assert pts.shape == (n_p, 3) and rays.shape == (n_r, 3) and dobs.shape == (n_p,)
        assert pts.dtype == rays.dtype == dobs.dtype == t.dtype == np.float32 and t.shape == (4, 4)
        assert tuple(t.reshape(16).tolist()) == orec["t_cam_obj"]
        assert np.array_equal(LC.bits(pts), LC.bits(opts[:n_p])) and np.array_equal(LC.bits(rays), LC.bits(orays[:n_r]))
        assert np.array_equal(LC.bits(dobs), LC.bits(odobs[:n_p]))
        keep = []
        rec = opt._object_in(t, pts, rays, dobs, c, keep)
        assert (rec.n_pts, rec.n_rays, rec.n_depth) == (n_p, n_r, n_p)
        for held, mine in zip(keep[:3], (pts, rays, dobs)):                  # no copy, no conversion
            assert mine.size == 0 or np.shares_memory(held, mine)
        assert (c is None) == (i != 1)
    with pytest.raises(TypeError):
        U.lidar_inputs(velo, inst, masks, dets, cam, tcv, max_points=3)
    with pytest.raises(ValueError):
        U.lidar_inputs(velo, inst[:-1], masks, dets, cam, tcv)
    with pytest.raises(ValueError):
        U.lidar_inputs(velo[:, :2], inst, masks, dets, cam, tcv)


# ---------------------------------------------------------------------------- the reference's output
def test_rule_matches_the_reference_on_the_golden_frame():
    """FrameWithLiDAR.get_detections' recorded output against dsr_lidar_inputs_host on the same
    inputs.  The fixture was screened (make_lidar_frame.py): no point near a face, linspace equal to
    sel, no projection near a pixel boundary, no count near the threshold — so the decisions must
    agree exactly and the values within bounds derived from the arithmetic:

    * surface points / depth: the reference adds the same four fp32 terms in another order, each
      partial sum rounded: <= 4 * 2^-24 * sum|terms|;
    * rays: the reference goes through K and inverse(K) in fp32 / fp64: <= 8 * 2^-24 * max(1, |r|);
    * T_cam_obj: fp32 cos / sin, an fp32 4 x 4 product, then the fp32 scale: <= 16 * 2^-24 *
      sum|terms| of the fp64 product the rule rounds once."""
    z, c = LC.golden_inputs()
    velo, inst, mlist, dets, cam, tcv, params = c
    assert z["screen_face"] > z["screen_limits"][0] and z["screen_pixel"] > z["screen_limits"][1]
    assert z["screen_hit"] > z["screen_limits"][2] and params == LO.DEFAULTS
    res = LC.run("host", *c)
    LC.assert_matches_oracle(*c, res)
    rc, pts, rays, dobs, recs = res
    assert int(z["n_instances"]) == len(dets) == 3
    C = np.asarray(tcv, np.float64).reshape(4, 4)
    P = dict(LO.DEFAULTS, **params)
    seen_rays = set()
    for i, (d, r) in enumerate(zip(dets, recs)):
        n = r.n_pts
        assert n == int(z[f"ref{i}_num_surface_points"]) and bool(z[f"ref{i}_is_front"]) == (r.status != 1)
        assert r.mask == int(z[f"ref{i}_mask"])
        has_rays = bool(z[f"ref{i}_has_rays"])
        assert has_rays == (r.status == 0)
        seen_rays.add(has_rays)
        # the sweep points behind the rows, for the bounds
        L = LO.prepare(d, tcv, P)
        _, _, pick = LO.crop_rows(np.ascontiguousarray(velo[:, :3]), L, P)
        p = velo[pick, :3].astype(np.float64)
        terms = np.abs(p) @ np.abs(C[:3, :3]).T + np.abs(C[:3, 3])
        ref_pts = z[f"ref{i}_surface_points"]
        assert ref_pts.shape == (n, 3)
        err = np.abs(ref_pts.astype(np.float64) - pts[i, :n].astype(np.float64))
        print(f"instance {i}: points max err / bound {np.max(err / (4 * U24 * terms)):.3f}")
        assert np.all(err <= 4 * U24 * terms)
        # T_cam_obj against the fp64 product
        th = float(d["theta"])
        cs, sn = math.cos(th), math.sin(th)
        R = np.array([[cs, 0, -sn], [-sn, 0, -cs], [0, 1, 0]], np.float64)
        sigma = float(np.float32(P["box_margin"])) * float(d["size"][1]) / 2.0
        o = np.array([float(d["trans"][0]), float(d["trans"][1]), float(d["trans"][2]) + float(d["size"][2]) / 2.0])
        T = np.eye(4)
        T[:3, :3] = C[:3, :3] @ (sigma * R)
        T[:3, 3] = C[:3, :3] @ o + C[:3, 3]
        tt = np.zeros((4, 4))
        tt[:3, :3] = np.abs(C[:3, :3]) @ np.abs(sigma * R)
        tt[:3, 3] = np.abs(C[:3, :3]) @ np.abs(o) + np.abs(C[:3, 3])
        mine = np.asarray(r.t_cam_obj, np.float64).reshape(4, 4)
        assert np.all(np.abs(mine - T) <= U24 * np.abs(T) + 1e-300)         # the rule: the product rounded once
        terr = np.abs(z[f"ref{i}_t_cam_obj"].astype(np.float64) - T)
        print(f"instance {i}: T_cam_obj max err / bound {np.max(terr[:3] / (16 * U24 * tt[:3] + 1e-300)):.3f}")
        assert np.all(terr[:3] <= 16 * U24 * tt[:3]) and np.array_equal(z[f"ref{i}_t_cam_obj"][3], [0, 0, 0, 1])
        if not has_rays:
            assert r.n_bg == 0 and z[f"ref{i}_rays"].shape[0] == 0
            continue
        ref_rays, ref_depth = z[f"ref{i}_rays"], z[f"ref{i}_depth"]
        assert ref_rays.shape == (n + r.n_bg, 3) and ref_depth.shape == (n,)
        m = n + r.n_bg
        rerr = np.abs(ref_rays.astype(np.float64) - rays[i, :m].astype(np.float64))
        rb = 8 * U24 * np.maximum(1.0, np.abs(rays[i, :m].astype(np.float64)))
        print(f"instance {i}: fg rays max err / bound {np.max(rerr[:n] / rb[:n]):.3f}, "
              f"bg rays {np.max(rerr[n:] / rb[n:]):.3f} ({r.n_bg} rays)")
        assert np.all(rerr <= rb)
        assert np.all(np.abs(ref_depth.astype(np.float64) - dobs[i, :n].astype(np.float64)) <= 4 * U24 * terms[:, 2])
    assert seen_rays == {True, False}
