"""Synthetic frames for the start-pose tests (test_frame_pose_cpu.py, test_gpu_frame_pose.py):
the depth of a tilted, yawed ellipsoid in front of a far wall, computed analytically per pixel
(ray-ellipsoid intersection) at frame_cases.py's 160 x 96 camera, the variations that walk every
path of the rule, and the runners that call an entry point on them."""
from __future__ import annotations

import functools

import numpy as np

from reconstruct import _libdsr as L
from reconstruct import utils as U

import frame_cases as FC
import frame_pose_oracle as PO

W, H, CAM = FC.W, FC.H, FC.CAM
SENTINEL = FC.SENTINEL
WALL = 6.0
INF = float("inf")


def rot(yaw, tilt):
    cy, sy, ct, st = np.cos(yaw), np.sin(yaw), np.cos(tilt), np.sin(tilt)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rx = np.array([[1, 0, 0], [0, ct, -st], [0, st, ct]])
    return Rx @ Ry


def ellipsoid_frame(centre=(0.1, -0.05, 3.0), s=0.5, yaw=0.6, tilt=0.25, cam=CAM, label=1):
    """Depth (z along the optical axis) of the ellipsoid with semi-axes (0.9, 0.5, 1.6) s, yawed
    about y and tilted about x, in front of a wall at z = WALL; instance = label on the ellipsoid."""
    w, h = cam["width"], cam["height"]
    v, u = np.mgrid[0:h, 0:w].astype(np.float64)
    d = np.stack([(u - cam["cx"]) / cam["fx"], (v - cam["cy"]) / cam["fy"], np.ones_like(u)], -1)
    Ro, a = rot(yaw, tilt), np.array([0.9, 0.5, 1.6]) * s
    dn = (d @ Ro) / a                                        # the ray and the centre in unit-sphere space
    cn = (np.asarray(centre) @ Ro) / a
    A, B, Cc = (dn * dn).sum(-1), (dn * cn).sum(-1), (cn * cn).sum() - 1.0
    disc = B * B - A * Cc
    hit = disc > 0
    t = (B - np.sqrt(np.where(hit, disc, 0.0))) / A
    depth = np.where(hit, t, WALL).astype(np.float32)
    inst = np.where(hit, label, -1).astype(np.int32)
    return depth, inst


def leak_frame():
    """A strip of the mask lies on the wall: pass 1 removes it."""
    depth, inst = ellipsoid_frame()
    vs, us = np.nonzero(inst == 1)
    inst = inst.copy()
    inst[vs.min():vs.min() + 3, us.max() + 2:us.max() + 14] = 1
    return depth, inst


def spike_frame():
    """A few object pixels pushed 0.45 back: within the radius, outside 1.2 x the box."""
    depth, inst = ellipsoid_frame()
    vs, us = np.nonzero(inst == 1)
    depth = depth.copy()
    pick = np.arange(40, vs.shape[0], 211)
    depth[vs[pick], us[pick]] += np.float32(0.45)
    return depth, inst


def plane_frame():
    """A fronto-parallel 60 x 24 pixel rectangle at depth 2."""
    depth = np.full((H, W), WALL, np.float32)
    inst = np.full((H, W), -1, np.int32)
    inst[30:54, 50:110] = 1
    depth[inst == 1] = 2.0
    return depth, inst


def pixel_frame():
    depth, inst = plane_frame()
    inst = np.full((H, W), -1, np.int32)
    inst[40, 70] = 1
    return depth, inst


def det(label, pose=None, bbox=None):
    return dict(label=label, bbox=bbox, t_cam_obj=pose)


GIVEN_POSE = np.array([[0.5, 0.0, 0.1, 0.2], [0.0, 0.6, 0.0, -0.1], [-0.1, 0.0, 0.5, 3.0], [0, 0, 0, 1]], np.float32)
P = dict(min_mask_area=100, max_pts=4096, max_bg=200)
C, F, G = PO.CUBOID, PO.CUBOID_FLIPPED, PO.GIVEN


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (frame, camera, detections, modes, frame params, pose params)"""
    clean, leak, spike, plane = ellipsoid_frame(), leak_frame(), spike_frame(), plane_frame()

    def counts(frame, params=P, **q):
        r = PO.poses(frame[0], frame[1], [det(1)], [C], CAM, q, **params)[0][4]
        return r["n_in"], r["n_near"], r["n_kept"]

    c = {}
    c["clean"] = (clean, CAM, [det(1)], [C], P, {})
    c["leak"] = (leak, CAM, [det(1)], [C], P, {})
    c["spike"] = (spike, CAM, [det(1)], [C], P, {})
    c["n_in_49"] = (clean, CAM, [det(1)], [C], dict(P, max_pts=49), {})
    c["n_in_50"] = (clean, CAM, [det(1)], [C], dict(P, max_pts=50), {})
    n_in, n_near, _ = counts(leak)
    c["few_near"] = (leak, CAM, [det(1)], [C], P, dict(min_points=n_near + 1))
    n_in, n_near, n_kept = counts(spike)
    c["few_kept"] = (spike, CAM, [det(1)], [C], P, dict(min_points=n_kept + 1))
    c["one_pixel"] = (pixel_frame(), CAM, [det(1)], [C], dict(P, min_mask_area=0), dict(min_points=1))
    c["plane"] = (plane, CAM, [det(1)], [C], P, {})
    c["cap700"] = (clean, CAM, [det(1)], [C], dict(P, max_pts=700), {})
    c["n60"] = (clean, CAM, [det(1)], [C], dict(P, max_pts=60), dict(outlier_radius=INF))
    c["n99"] = (clean, CAM, [det(1)], [C], dict(P, max_pts=99), dict(outlier_radius=INF))
    c["up_plus_y"] = (clean, CAM, [det(1)], [C], P, dict(up=(0.0, 1.0, 0.0)))
    c["given"] = (leak, CAM, [det(1, GIVEN_POSE)], [G], dict(P, max_pts=300), {})
    c["flipped"] = (spike, CAM, [det(1), det(1)], [C, F], P, {})
    c["shared_label"] = (leak, CAM, [det(1, GIVEN_POSE), det(1), det(9), det(1)], [G, C, C, F], dict(P, max_pts=500), {})
    c["passes_off"] = (leak, CAM, [det(1)], [C], P, dict(outlier_radius=INF, box_margin=INF))
    return c


CASE_NAMES = ["clean", "leak", "spike", "n_in_49", "n_in_50", "few_near", "few_kept", "one_pixel", "plane", "cap700",
              "n60", "n99", "up_plus_y", "given", "flipped", "shared_label", "passes_off"]


def run(entry, depth, inst, cam, dets, modes, params, pose_params, ctx=None):
    """``dsr_frame_poses_host`` (entry "host") or ``dsr_frame_poses`` ("device", with a context) on
    sentinel-filled arrays; returns (rc, pts, rays, dobs, ingest records, pose records)."""
    lib = L.load_library()
    cam = U.frame_camera(cam)
    p = U.frame_params(**params)
    q = U.frame_pose_params(pose_params)
    depth = np.ascontiguousarray(depth, np.float32)
    inst = np.ascontiguousarray(inst, np.int32)
    n = len(dets)
    fd, keep = U.frame_dets([U._with_pose(d) for d in dets])
    m = np.ascontiguousarray(modes, np.int32)
    pts = np.full((max(n, 1), p.max_pts, 3), SENTINEL, np.float32)
    rays = np.full((max(n, 1), p.max_pts + p.max_bg, 3), SENTINEL, np.float32)
    dobs = np.full((max(n, 1), p.max_pts), SENTINEL, np.float32)
    out = (L.FrameDetOut * max(n, 1))()
    pout = (L.FramePoseOut * max(n, 1))()
    args = (cam, p, q, L.fptr(depth), L.iptr(inst), n, fd, L.iptr(m), L.fptr(pts), L.fptr(rays), L.fptr(dobs), out, pout)
    rc = lib.dsr_frame_poses_host(*args) if entry == "host" else lib.dsr_frame_poses(ctx.handle, *args)
    return rc, pts, rays, dobs, [U.frame_record(out[i]) for i in range(n)], [U.frame_pose_record(pout[i]) for i in range(n)]


def run_case(entry, case, ctx=None):
    (depth, inst), cam, dets, modes, params, pose_params = case
    return run(entry, depth, inst, cam, dets, modes, params, pose_params, ctx=ctx)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def counted(rec, prec):
    """(point rows, ray rows) a detection's records count."""
    if prec["status"] == PO.NOT_ASKED:
        return rec["n_pts"], rec["n_pts"] + rec["n_bg"]
    if prec["status"] == PO.OK:
        return prec["n_kept"], prec["n_kept"] + rec["n_bg"]
    return 0, 0


def same_pose_record(a, b):
    return (all(a[k] == b[k] for k in ("status", "n_in", "n_near", "n_kept"))
            and np.array_equal(bits64(a["dims"]), bits64(b["dims"])) and np.array_equal(bits64(a["eig"]), bits64(b["eig"]))
            and np.array_equal(bits(a["t_cam_obj"]), bits(b["t_cam_obj"])))


def assert_matches_oracle(case, result):
    (depth, inst), cam, dets, modes, params, pose_params = case
    rc, pts, rays, dobs, recs, precs = result
    assert rc == 0
    want = PO.poses(depth, inst, [U._with_pose(d) for d in dets], modes, cam, pose_params, **params)
    for i, (opts, orays, odobs, orec, oprec) in enumerate(want):
        assert dict(recs[i], box=tuple(recs[i]["box"])) == orec, (i, recs[i], orec)
        assert same_pose_record(precs[i], oprec), (i, precs[i], oprec)
        n, m = counted(orec, oprec)
        assert opts.shape[0] == n and orays.shape[0] == m
        assert np.array_equal(bits(pts[i, :n]), bits(opts)), i
        assert np.array_equal(bits(rays[i, :m]), bits(orays)), i
        assert np.array_equal(bits(dobs[i, :n]), bits(odobs)), i
    return want


def assert_same(a, b):
    """Two ``run`` results agree in records and bitwise on every counted row."""
    assert a[0] == b[0] == 0
    assert a[4] == b[4]
    assert len(a[5]) == len(b[5])
    for i, (x, y) in enumerate(zip(a[5], b[5])):
        assert same_pose_record(x, y), (i, x, y)
        n, m = counted(a[4][i], x)
        for k, rows in ((1, n), (2, m), (3, n)):
            assert np.array_equal(bits(a[k][i, :rows]), bits(b[k][i, :rows])), (i, k)
