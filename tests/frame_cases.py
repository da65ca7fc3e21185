"""Synthetic frames for the frame-ingest tests (test_frame_cpu.py, test_gpu_frame.py): small depth
+ instance images with elliptical masks and depth holes, the detection lists / parameter sets that
walk every path of the rule, and the runners that call an entry point on them."""
from __future__ import annotations

import numpy as np

from reconstruct import _libdsr as L
from reconstruct import utils as U

import frame_oracle as FO

W, H = 160, 96
CAM = dict(width=W, height=H, fx=140.0, fy=138.5, cx=79.5, cy=47.25)
SENTINEL = np.float32(-12345.5)


def ellipse(w, h, cu, cv, ru, rv):
    v, u = np.mgrid[0:h, 0:w]
    return ((u - cu) / ru) ** 2 + ((v - cv) / rv) ** 2 <= 1.0


def base_frame():
    """Labels: 1 a large ellipse with every kind of depth hole, 2 a mid-sized one at the left border,
    3 one without any valid depth, 4 a tiny one (gh = 1 / 0 boxes)."""
    rng = np.random.default_rng(11)
    inst = np.full((H, W), -1, np.int32)
    inst[ellipse(W, H, 95, 50, 45, 33)] = 1
    inst[ellipse(W, H, 8, 30, 22, 26)] = 2
    inst[ellipse(W, H, 140, 14, 16, 12)] = 3
    inst[70:77, 20:31] = 4
    inst[70, 20:24] = -1                                    # a background pixel on the gh = 1 grid
    depth = (2.0 + 0.01 * np.arange(W)[None, :] + 0.02 * np.arange(H)[:, None]
             + 0.05 * rng.standard_normal((H, W))).astype(np.float32)
    holes = rng.random((H, W))
    depth[holes < 0.04] = 0.0
    depth[(holes >= 0.04) & (holes < 0.08)] = np.nan
    depth[(holes >= 0.08) & (holes < 0.12)] = np.inf
    depth[(holes >= 0.12) & (holes < 0.16)] = 50.0          # beyond far = 10
    depth[(holes >= 0.16) & (holes < 0.18)] = -1.0
    depth[inst == 3] = 0.0
    return depth, inst


def border_frame():
    """Label 7 touches all four image borders (an ellipse larger than the image)."""
    depth, _ = base_frame()
    inst = np.full((H, W), 0, np.int32)
    inst[ellipse(W, H, 80, 48, 90, 50)] = 7
    return depth, inst


def exact_valid_frame(n_valid):
    """Label 1 with exactly ``n_valid`` valid pixels (the rest of its mask has depth 0)."""
    depth, inst = base_frame()
    depth = depth.copy()
    m = inst == 1
    depth[m & ~((depth == depth) & (depth > 0.01) & (depth < 10.0))] = 0.0
    vv, uu = np.nonzero(m & (depth > 0.01))
    assert vv.shape[0] > n_valid
    depth[vv[n_valid:], uu[n_valid:]] = 0.0
    return depth, inst


def det(label, bbox=None):
    return dict(label=label, bbox=bbox, t_cam_obj=np.eye(4, dtype=np.float32))


def cases():
    base, border = base_frame(), border_frame()
    n1 = int((base[1] == 1).sum())
    P = dict(far=10.0, min_mask_area=100)
    c = {}
    c["cap_hit"] = (base, CAM, [det(1), det(2)], dict(P, max_pts=250, max_bg=200))
    c["cap_not_hit"] = (base, CAM, [det(1), det(2)], dict(P, max_pts=5000, max_bg=3000))
    c["n1080"] = (exact_valid_frame(1080), CAM, [det(1)], dict(P, max_pts=250))
    c["borders"] = (border, CAM, [det(7), det(0)], dict(P, max_pts=300, max_bg=150))
    c["boxes"] = (base, CAM, [det(1), det(1, (40, 10, 150, 90)), det(1, (-10, -5, 60, 200)),
                              det(2, (100, 40, 400, 60)), det(2, (200, 10, 300, 50)), det(2, (30, 60, 50, 20))],
                  dict(P, max_pts=64, max_bg=500))
    c["downsample1"] = (base, CAM, [det(2), det(1)], dict(P, downsample=1, max_pts=100, max_bg=100000))
    c["downsample1_cap"] = (base, CAM, [det(2)], dict(P, downsample=1, max_pts=100, max_bg=37))
    c["gh1"] = (base, CAM, [det(4), det(4, (20, 70, 30, 76))], dict(P, expand=0, min_mask_area=10, max_bg=50))
    c["gh0"] = (base, CAM, [det(4, (20, 70, 30, 72)), det(4, (20, 70, 22, 76))],
                dict(P, expand=0, min_mask_area=10, max_bg=50))
    c["max_bg0"] = (base, CAM, [det(1), det(2)], dict(P, max_bg=0))
    c["dup_label"] = (base, CAM, [det(1), det(2), det(1)], dict(P))
    c["absent"] = (base, CAM, [det(77), det(1), det(77, (10, 10, 60, 60))], dict(P))
    c["area_eq"] = (base, CAM, [det(1)], dict(P, min_mask_area=n1))
    c["area_plus1"] = (base, CAM, [det(1)], dict(P, min_mask_area=n1 - 1))
    c["no_depth"] = (base, CAM, [det(3), det(1)], dict(P))
    c["one_pt"] = (base, CAM, [det(1)], dict(P, max_pts=1, max_bg=1))
    c["n_det0"] = (base, CAM, [], dict(P))
    c["nine"] = (base, CAM, [det(1), det(2), det(3), det(4), det(1, (0, 0, 159, 95)), det(2), det(5), det(-1),
                             det(1, (90, 40, 100, 50))], dict(P, min_mask_area=50))
    return c


def run(entry, depth, inst, cam, dets, params, ctx=None):
    """Call ``dsr_frame_inputs_host`` (entry "host") or ``dsr_frame_inputs`` ("device", with a
    context) with sentinel-filled arrays; returns (rc, pts, rays, dobs, records)."""
    lib = L.load_library()
    cam = U.frame_camera(cam)
    p = U.frame_params(**params)
    depth = np.ascontiguousarray(depth, np.float32)
    inst = np.ascontiguousarray(inst, np.int32)
    n = len(dets)
    fd, keep = U.frame_dets(dets)
    pts = np.full((max(n, 1), p.max_pts, 3), SENTINEL, np.float32)
    rays = np.full((max(n, 1), p.max_pts + p.max_bg, 3), SENTINEL, np.float32)
    dobs = np.full((max(n, 1), p.max_pts), SENTINEL, np.float32)
    out = (L.FrameDetOut * max(n, 1))()
    args = (cam, p, L.fptr(depth), L.iptr(inst), n, fd, L.fptr(pts), L.fptr(rays), L.fptr(dobs), out)
    if entry == "host":
        rc = lib.dsr_frame_inputs_host(*args)
    else:
        rc = lib.dsr_frame_inputs(ctx.handle, *args)
    return rc, pts, rays, dobs, [U.frame_record(out[i]) for i in range(n)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_matches_oracle(depth, inst, cam, dets, params, result):
    rc, pts, rays, dobs, recs = result
    assert rc == 0
    for i, d in enumerate(dets):
        opts, orays, odobs, orec = FO.ingest(depth, inst, d, cam, **params)
        assert dict(recs[i], box=tuple(recs[i]["box"])) == orec, (i, recs[i], orec)
        n, m = orec["n_pts"], orec["n_pts"] + orec["n_bg"]
        assert np.array_equal(bits(pts[i, :n]), bits(opts)), i
        assert np.array_equal(bits(rays[i, :m]), bits(orays)), i
        assert np.array_equal(bits(dobs[i, :n]), bits(odobs)), i
        # rows beyond the counts are untouched
        assert np.all(pts[i, n:] == SENTINEL) and np.all(rays[i, m:] == SENTINEL) and np.all(dobs[i, n:] == SENTINEL), i
    if len(dets) < pts.shape[0]:
        assert np.all(pts == SENTINEL) and np.all(rays == SENTINEL) and np.all(dobs == SENTINEL)


def assert_same(a, b):
    """Two ``run`` results agree bitwise (arrays in full, sentinel rows included) and in records."""
    assert a[0] == b[0] == 0
    for x, y in zip(a[1:4], b[1:4]):
        assert np.array_equal(bits(x), bits(y))
    assert a[4] == b[4]
