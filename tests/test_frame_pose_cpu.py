"""Cuboid start poses and outlier removal without a GPU:
dsr_frame_pose_params_default, the new struct layouts, dsr_frame_poses_host against the numpy
restatement of the rule (tests/frame_pose_oracle.py) bitwise on synthetic frames
(tests/frame_pose_cases.py), properties of the result that do not depend on the restatement, the
argument errors, and reconstruct.utils.frame_poses."""
from __future__ import annotations

import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import REPO

import frame_cases as FC
import frame_pose_cases as PC
import frame_pose_oracle as PO

HDR = os.path.join(REPO, "include", "dsr.h")


@pytest.fixture(scope="module")
def cases():
    return PC.cases()


@pytest.fixture(scope="module")
def host(cases):
    """Every case through dsr_frame_poses_host, once."""
    return {name: PC.run_case("host", cases[name]) for name in PC.CASE_NAMES}


def test_pose_params_default():
    from reconstruct import _libdsr as L

    p = L.FramePoseParams()
    lib = L.load_library()
    assert lib.dsr_frame_pose_params_default(p) == 0
    assert (p.outlier_radius, p.lo_pct, p.hi_pct, p.min_points) == (1.0, 5, 95, 50)
    assert p.box_margin == np.float32(1.2) and p.scale_factor == np.float32(0.40) and tuple(p.up) == (0.0, -1.0, 0.0)
    assert lib.dsr_frame_pose_params_default(None) < 0
    assert PO.DEFAULTS == dict(outlier_radius=1.0, lo_pct=5, hi_pct=95, box_margin=1.2, scale_factor=0.40,
                               min_points=50, up=(0.0, -1.0, 0.0))
    assert lib.dsr_abi_version() == 12


def test_pose_struct_layouts_match_ctypes():
    from reconstruct import _libdsr as L

    structs = {"dsr_frame_pose_params": "FramePoseParams", "dsr_frame_pose_out": "FramePoseOut"}
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HDR}"', "int main(void){"]
    for cname, pyname in structs.items():
        lines.append(f'printf("{pyname} size %zu\\n", sizeof({cname}));')
        for fld, _ in getattr(L, pyname)._fields_:
            lines.append(f'printf("{pyname} {fld} %zu\\n", offsetof({cname}, {fld}));')
    lines.append('printf("enum %d %d %d %d %d %d %d %d\\n", DSR_FRAME_POSE_GIVEN, DSR_FRAME_POSE_CUBOID, '
                 'DSR_FRAME_POSE_CUBOID_FLIPPED, DSR_FRAME_POSE_OK, DSR_FRAME_POSE_NOT_ASKED, DSR_FRAME_POSE_NO_INPUT, '
                 'DSR_FRAME_POSE_FEW_POINTS, DSR_FRAME_POSE_DEGENERATE);')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c99", "-o", exe, src], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    seen = 0
    for line in out.strip().splitlines():
        if line.startswith("enum"):
            assert [int(x) for x in line.split()[1:]] == [
                L.FRAME_POSE_GIVEN, L.FRAME_POSE_CUBOID, L.FRAME_POSE_CUBOID_FLIPPED, L.FRAME_POSE_OK,
                L.FRAME_POSE_NOT_ASKED, L.FRAME_POSE_NO_INPUT, L.FRAME_POSE_FEW_POINTS, L.FRAME_POSE_DEGENERATE]
            assert [PO.GIVEN, PO.CUBOID, PO.CUBOID_FLIPPED, PO.OK, PO.NOT_ASKED, PO.NO_INPUT, PO.FEW_POINTS,
                    PO.DEGENERATE] == [0, 1, 2, 0, 1, 2, 3, 4]
            continue
        py, what, val = line.split()
        cls = getattr(L, py)
        if what == "size":
            assert ctypes.sizeof(cls) == int(val), line
        else:
            assert getattr(cls, what).offset == int(val), line
        seen += 1
    assert seen == sum(1 + len(getattr(L, n)._fields_) for n in structs.values())
    for f in ("dsr_frame_pose_params_default", "dsr_frame_poses_host", "dsr_frame_poses",
              "dsr_batch_refill_frame_poses", "dsr_batch_frame_pose_info"):
        assert f in L.SIGNATURES and f in L.BY_SYMBOL, f


@pytest.mark.parametrize("name", PC.CASE_NAMES)
def test_host_equals_oracle(cases, host, name):
    PC.assert_matches_oracle(cases[name], host[name])


def test_case_list_is_complete(cases):
    assert sorted(PC.CASE_NAMES) == sorted(cases)


def test_cases_take_the_paths_they_are_named_for(cases, host):
    def prec(name, i=0):
        return host[name][5][i]

    r = prec("clean")
    assert r.status == PO.OK and r.n_in == r.n_near > 1000 and r.n_kept >= 50
    r = prec("leak")
    assert r.status == PO.OK and 50 <= r.n_near < r.n_in
    r = prec("spike")
    assert r.status == PO.OK and 50 <= r.n_kept < r.n_near == r.n_in
    r = prec("n_in_49")
    assert (r.status, r.n_in, r.n_kept) == (PO.FEW_POINTS, 49, 0) and not r.dims.any()
    r = prec("n_in_50")
    assert r.n_in == r.n_near == 50 and r.eig[2] > 0
    r = prec("few_near")
    assert r.status == PO.FEW_POINTS and r.n_near == cases["few_near"][5]["min_points"] - 1 < r.n_in and not r.eig.any()
    r = prec("few_kept")
    assert r.status == PO.FEW_POINTS and r.n_kept == cases["few_kept"][5]["min_points"] - 1 < r.n_near and r.dims[2] > 0
    assert np.array_equal(r.t_cam_obj, np.eye(4, dtype=np.float32))
    r = prec("one_pixel")
    assert (r.status, r.n_in, r.n_near) == (PO.DEGENERATE, 1, 1) and not r.dims.any() and not r.eig.any()
    r = prec("cap700")
    assert r.status == PO.OK and r.n_in == 700 and host["cap700"][4][0].n_valid > 700 and r.n_near % 256 != 0
    for name, n in (("n60", 60), ("n99", 99)):
        r = prec(name)
        assert r.n_in == r.n_near == n and r.status == PO.OK
    assert (60 * 5) // 100 == 3 and (60 * 95) // 100 == 57 and (99 * 5) // 100 == 4 and (99 * 95) // 100 == 94
    assert [prec("shared_label", i).status for i in range(4)] == [PO.NOT_ASKED, PO.OK, PO.NO_INPUT, PO.OK]


def test_plane_patch_has_ties(cases, host):
    """The fronto-parallel patch: every point has z = 2 exactly, so the projections on the normal
    axis are all equal and the selection meets ties; its extent there is exactly 0."""
    r = host["plane"][5][0]
    assert r.status == PO.OK and r.dims[1] == 0.0 and r.dims[2] > r.dims[0] > 0 and r.eig[0] == 0.0


def _R(prec):
    T = prec.t_cam_obj.astype(np.float64)[:3, :3]
    return T / np.cbrt(np.linalg.det(T))


def test_up_flips_columns_0_and_1(host):
    a, b = host["clean"][5][0], host["up_plus_y"][5][0]
    assert np.array_equal(a.t_cam_obj[:3, 0], -b.t_cam_obj[:3, 0]) and np.array_equal(a.t_cam_obj[:3, 1], -b.t_cam_obj[:3, 1])
    assert np.array_equal(a.t_cam_obj[:, 2:], b.t_cam_obj[:, 2:])
    assert np.array_equal(PC.bits64(a.dims), PC.bits64(b.dims))
    assert a.t_cam_obj[1, 1] < 0 < b.t_cam_obj[1, 1]


def test_given_is_the_plain_ingest(cases, host):
    (depth, inst), cam, dets, modes, params, _ = cases["given"]
    plain = FC.run("host", depth, inst, cam, dets, params)
    rc, pts, rays, dobs, recs, precs = host["given"]
    assert rc == 0 and recs == plain[4]
    for mine, theirs in zip((pts, rays, dobs), plain[1:4]):                  # sentinel rows included
        assert np.array_equal(PC.bits(mine), PC.bits(theirs))
    assert precs[0].status == PO.NOT_ASKED and precs[0].n_in == recs[0].n_pts == 300
    assert np.array_equal(precs[0].t_cam_obj, PC.GIVEN_POSE)


def test_flipped_negates_columns_0_and_2(host):
    rc, pts, rays, dobs, recs, (a, b) = host["flipped"]
    assert a.status == b.status == PO.OK and (a.n_in, a.n_near, a.n_kept) == (b.n_in, b.n_near, b.n_kept)
    want = a.t_cam_obj.copy()
    want[:3, 0], want[:3, 2] = -want[:3, 0], -want[:3, 2]                    # the bottom row stays 0 0 0 1
    assert np.array_equal(PC.bits(b.t_cam_obj), PC.bits(want))
    assert a.t_cam_obj[0, 0] != 0
    n, m = a.n_kept, a.n_kept + recs[0].n_bg
    assert np.array_equal(PC.bits(pts[0, :n]), PC.bits(pts[1, :n])) and np.array_equal(PC.bits(rays[0, :m]), PC.bits(rays[1, :m]))
    assert np.array_equal(PC.bits(dobs[0, :n]), PC.bits(dobs[1, :n]))


def test_passes_off_leaves_the_plain_ingest(cases, host):
    (depth, inst), cam, dets, modes, params, _ = cases["passes_off"]
    plain = FC.run("host", depth, inst, cam, [PC.U._with_pose(d) for d in dets], params)
    rc, pts, rays, dobs, recs, precs = host["passes_off"]
    assert precs[0].status == PO.OK and precs[0].n_kept == precs[0].n_near == precs[0].n_in == recs[0].n_pts
    n, m = recs[0].n_pts, recs[0].n_pts + recs[0].n_bg
    assert np.array_equal(PC.bits(pts[0, :n]), PC.bits(plain[1][0, :n]))
    assert np.array_equal(PC.bits(rays[0, :m]), PC.bits(plain[2][0, :m]))
    assert np.array_equal(PC.bits(dobs[0, :n]), PC.bits(plain[3][0, :n]))


@pytest.mark.parametrize("name", ["clean", "leak", "spike", "cap700", "n60", "plane", "up_plus_y"])
def test_properties_independent_of_the_restatement(cases, host, name):
    """R is a rotation whose column 1 does not oppose up, it diagonalises the scatter matrix of the
    near points, the pose scale is 0.40 l, and the kept / dropped points are inside / outside the
    box_margin cuboid — all recomputed here from the record and the plain ingest."""
    (depth, inst), cam, dets, modes, params, pose_params = cases[name]
    Q = dict(PO.DEFAULTS, **pose_params)
    rc, pts, rays, dobs, recs, precs = host[name]
    r = precs[0]
    assert r.status == PO.OK
    R = _R(r)
    assert np.abs(R.T @ R - np.eye(3)).max() < 1e-6                          # fp32 entries of the pose
    assert abs(np.linalg.det(R) - 1) < 1e-6
    assert np.dot(np.asarray(Q["up"]), R[:, 1]) >= 0
    s = np.cbrt(np.linalg.det(r.t_cam_obj.astype(np.float64)[:3, :3]))
    assert abs(s - np.float32(0.40) * r.dims[2]) <= 4 * 2.0 ** -24 * s       # nine entries rounded to fp32
    # the ingested points, then the passes in numpy
    plain = FC.run("host", depth, inst, cam, [PC.U._with_pose(d) for d in dets], params)
    P = plain[1][0, :r.n_in].astype(np.float64)
    near = np.linalg.norm(P - P.mean(0), axis=1) <= Q["outlier_radius"]
    assert near.sum() == r.n_near
    X = P[near] - P[near].mean(0)
    Cm = X.T @ X
    w, V = np.linalg.eigh(Cm)
    assert np.allclose(w, r.eig, rtol=1e-9, atol=1e-12 * np.linalg.norm(Cm))
    # R's columns are eigenvectors: R^T C R is diagonal (fp32 pose entries bound the check)
    D = R.T @ Cm @ R
    assert np.abs(D - np.diag(np.diag(D))).max() <= 1e-5 * np.linalg.norm(Cm)
    q = P[near] @ R
    lo, hi = (r.n_near * Q["lo_pct"]) // 100, (r.n_near * Q["hi_pct"]) // 100
    qs = np.sort(q, 0)
    assert np.allclose(qs[hi] - qs[lo], r.dims, atol=1e-5)
    co = (qs[hi] + qs[lo]) / 2
    inside = (np.abs(q - co) <= np.float32(Q["box_margin"]) * r.dims / 2 + 1e-5).all(1)
    outside = (np.abs(q - co) > np.float32(Q["box_margin"]) * r.dims / 2 - 1e-5).any(1)
    kept = pts[0, :r.n_kept].astype(np.float64)
    # the kept rows are a subsequence of the near points, all inside; what was dropped is outside
    idx = np.nonzero(near)[0]
    pos, j = [], 0
    for row in kept:
        while not np.array_equal(P[idx[j]], row):
            j += 1
        pos.append(j)
        j += 1
    pos = np.asarray(pos)
    assert inside[pos].all()
    dropped = np.setdiff1d(np.arange(idx.shape[0]), pos)
    assert outside[dropped].all() and dropped.shape[0] == r.n_near - r.n_kept
    assert np.allclose(R @ co, r.t_cam_obj[:3, 3], atol=1e-5)


def test_jacobi_in_fp64(cases, host):
    """The record carries R only as the fp32 pose (checked at fp32 rounding above), so the fp64
    bounds are checked on the rule's own Jacobi and axes steps (bitwise the host's, by
    test_host_equals_oracle) on the fixtures' scatter matrices and on random ones: R^T R = I and
    det R = +1 within 1e-12, off-diagonals of V^T C V at most 1e-12 |C| (fp64 Jacobi, eps x O(10)),
    and the host's recorded eigenvalues within 1e-12 |C| of LAPACK's."""
    rng = np.random.default_rng(5)
    mats = []
    for name in ("clean", "leak", "spike", "cap700", "plane"):
        (depth, inst), cam, dets, modes, params, pose_params = cases[name]
        plain = FC.run("host", depth, inst, cam, [PC.U._with_pose(d) for d in dets], params)
        r = host[name][5][0]
        P = plain[1][0, :r.n_in].astype(np.float64)
        near = np.linalg.norm(P - P.mean(0), axis=1) <= 1.0
        X = P[near] - P[near].mean(0)
        mats.append(X.T @ X)
        assert np.abs(np.linalg.eigvalsh(mats[-1]) - r.eig).max() <= 1e-12 * np.linalg.norm(mats[-1]), name
    for k in range(20):
        X = rng.standard_normal((40, 3)) * rng.uniform(0.01, 3.0, 3)
        mats.append(X.T @ X)
    for Cm in mats:
        eig, v = PO.jacobi(Cm.tolist())
        V = np.asarray(v).T
        assert np.abs(V.T @ V - np.eye(3)).max() < 1e-12
        D = V.T @ Cm @ V
        assert np.abs(D - np.diag(np.diag(D))).max() <= 1e-12 * np.linalg.norm(Cm)
        assert eig == sorted(eig) and np.allclose(eig, np.linalg.eigvalsh(Cm), rtol=1e-10, atol=1e-12 * np.linalg.norm(Cm))
        R = np.asarray(PO.axes(v, (0.0, -1.0, 0.0)))
        assert np.abs(R.T @ R - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1) < 1e-12
        assert -R[1, 1] >= 0


def test_fronto_parallel_rectangle(host):
    """60 x 24 pixels at depth 2: the largest variance lies along the 60-pixel side, so R[:,2] =
    +-e_x; the smallest (exactly 0) along the normal, so R[:,1] = +-e_z — the normal, not the
    in-plane short axis, which is R[:,0] = +-e_y; up = (0,-1,0) is orthogonal to R[:,1] and decides
    nothing here."""
    R = _R(host["plane"][5][0])
    for col, axis in ((2, 0), (1, 2), (0, 1)):
        e = np.zeros(3)
        e[axis] = 1.0
        assert min(np.abs(R[:, col] - e).max(), np.abs(R[:, col] + e).max()) < 1e-9, (col, R)


def test_argument_errors_return_negative(cases):
    from reconstruct import _libdsr as L
    from reconstruct import utils as U

    lib = L.load_library()
    (depth, inst), cam, dets, modes, params, _ = cases["clean"]
    fd, keep = U.frame_dets([U._with_pose(d) for d in dets])
    out, pout = (L.FrameDetOut * 1)(), (L.FramePoseOut * 1)()
    nan = float("nan")

    def call(mode=PO.CUBOID, modes_=True, null=None, frame=None, **pose_params):
        p = U.frame_params(**dict(dict(max_pts=64, max_bg=8, min_mask_area=100), **(frame or {})))
        q = U.frame_pose_params(pose_params)
        m = np.asarray([mode], np.int32)
        arr = dict(pts=np.zeros((1, 64, 3), np.float32), rays=np.zeros((1, 72, 3), np.float32),
                   dobs=np.zeros((1, 64), np.float32))
        a = {k: (None if k == null else L.fptr(v)) for k, v in arr.items()}
        return lib.dsr_frame_poses_host(U.frame_camera(cam), p, q, L.fptr(depth), L.iptr(inst), 1, fd,
                                        L.iptr(m) if modes_ else None, a["pts"], a["rays"], a["dobs"],
                                        None if null == "out" else out, None if null == "pose_out" else pout)

    assert call() == 0
    assert call(min_points=0) < 0 and call(min_points=1) == 0
    assert call(lo_pct=-1) < 0 and call(lo_pct=95) < 0 and call(lo_pct=96) < 0 and call(hi_pct=100) < 0
    assert call(lo_pct=0, hi_pct=99) == 0
    for name in ("outlier_radius", "box_margin", "scale_factor"):
        assert call(**{name: 0.0}) < 0 and call(**{name: -1.0}) < 0 and call(**{name: nan}) < 0, name
    assert call(outlier_radius=PC.INF) == 0 and call(box_margin=PC.INF) == 0 and call(scale_factor=PC.INF) < 0
    assert call(up=(0.0, 0.0, 0.0)) < 0 and call(up=(nan, 1.0, 0.0)) < 0 and call(up=(0.0, PC.INF, 0.0)) < 0
    assert call(up=(0.0, 0.0, 2.0)) == 0
    assert call(mode=3) < 0 and call(mode=-1) < 0 and call(modes_=False) < 0
    for null in ("pts", "rays", "dobs", "out", "pose_out"):
        assert call(null=null) < 0, null
    assert call(frame=dict(max_pts=0)) < 0 and call(frame=dict(max_bg=-1)) < 0             # dsr_frame_inputs_host's
    assert lib.dsr_frame_poses_host(U.frame_camera(cam), U.frame_params(), None, L.fptr(depth), L.iptr(inst), 0, None,
                                    None, None, None, None, None, None) < 0


def test_frame_poses_feeds_reconstruct_objects(cases, host):
    """utils.frame_poses: objects trimmed to the counted rows with the start pose, both records."""
    from reconstruct import utils as U

    (depth, inst), cam, dets, modes, params, pose_params = cases["shared_label"]
    dets = [dict(d, mode=int(m) if m == PO.CUBOID_FLIPPED else None) for d, m in zip(dets, modes)]
    assert U.frame_pose_modes(dets).tolist() == list(modes)
    objects, records, poses = U.frame_poses(depth, inst, dets, cam, pose_params, **params)
    rc, pts, rays, dobs, recs, precs = host["shared_label"]
    assert records == recs
    for i, ((t, p, r, z, c), pr) in enumerate(zip(objects, poses)):
        assert PC.same_pose_record(pr, precs[i])
        n, m = PC.counted(recs[i], precs[i])
        assert p.shape == (n, 3) and r.shape == (m, 3) and z.shape == (n,) and t.shape == (4, 4)
        assert p.dtype == r.dtype == z.dtype == t.dtype == np.float32 and c is None
        assert np.array_equal(PC.bits(p), PC.bits(pts[i, :n])) and np.array_equal(PC.bits(r), PC.bits(rays[i, :m]))
        assert np.array_equal(PC.bits(z), PC.bits(dobs[i, :n])) and np.array_equal(t, precs[i].t_cam_obj)
    assert objects[2][1].shape == (0, 3) and np.array_equal(objects[2][0], np.eye(4, dtype=np.float32))
    with pytest.raises(TypeError):
        U.frame_poses(depth, inst, dets, cam, dict(radius=2.0), **params)
    with pytest.raises(TypeError):
        U.frame_poses(depth, inst, dets, cam, None, max_points=3)
