"""Synthetic sweeps for the LiDAR-ingest tests (test_lidar_cpu.py, test_gpu_lidar.py): small
Velodyne-like point sets around 3-D boxes, instance images painted where the points project, the
mask lists / detection lists / parameter sets that walk every path of the rule,
and the runners that call an entry point on them.  Every case runs in milliseconds."""
from __future__ import annotations

import math
import os

import numpy as np

from reconstruct import _libdsr as L
from reconstruct import utils as U

import lidar_oracle as LO

W, H = 160, 96
CAM = dict(width=W, height=H, fx=110.0, fy=108.5, cx=79.5, cy=47.25)
SENTINEL = np.float32(-12345.5)
F24 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f24_lidar_frame.npz")
f32 = np.float32


def t_cam_velo(yaw=0.01, pitch=-0.02, t=(0.05, -0.08, -0.27)):
    """A KITTI-like rigid velodyne -> camera transform: camera x = -velo y, y = -velo z, z = velo x,
    turned by two small angles (fp64, rounded once)."""
    base = np.array([[0, -1, 0], [0, 0, -1], [1, 0, 0]], np.float64)
    cy, sy, cp, sp = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch)
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    T = np.eye(4)
    T[:3, :3] = rx @ ry @ base
    T[:3, 3] = t
    return T.astype(f32)


TCV = t_cam_velo()


def det(x, y, z=-1.0, w=1.6, l=3.9, h=1.5, theta=0.3, code=None):
    return dict(trans=(x, y, z), size=(w, l, h), theta=theta, code=code)


def to_velo(d, local):
    """Box coordinates (x width, y height, z length; centre at the box centre) -> velodyne, fp64."""
    c, s = math.cos(d["theta"]), math.sin(d["theta"])
    R = np.array([[c, 0, -s], [-s, 0, -c], [0, 1, 0]], np.float64)
    o = np.array([d["trans"][0], d["trans"][1], d["trans"][2] + d["size"][2] / 2.0])
    return np.asarray(local, np.float64) @ R.T + o


def box_points(d, n, rng, shrink=0.9):
    """n points well inside the box (shrink < 1 of the unwidened half extents)."""
    w, l, h = d["size"]
    half = np.array([w / 2, h / 2, l / 2]) * shrink
    return to_velo(d, rng.uniform(-1, 1, (n, 3)) * half).astype(f32)


def above_points(d, n, rng):
    """n points in the cube but above the box: near, never in."""
    w, l, h = d["size"]
    local = rng.uniform(-1, 1, (n, 3)) * np.array([w / 2, 0.2, min(l / 2, 1.5)]) * 0.9
    local[:, 1] += h / 2 + 0.6
    return to_velo(d, local).astype(f32)


def line_points(d, k, frac=0.8):
    """k points on the box's length axis, evenly spread over +-frac of its half length."""
    zs = np.linspace(-frac, frac, k) * d["size"][1] / 2
    return to_velo(d, np.stack([np.zeros(k), np.zeros(k), zs], 1)).astype(f32)


def sweep(parts, stride=4, rng=None, pad_to=None):
    """Stack point sets into an (n, stride) sweep, shuffled when rng is given; columns >= 3 carry
    a reflectance-like value that nothing may read; pad_to appends far-away points."""
    p = np.concatenate([np.asarray(x, f32).reshape(-1, 3) for x in parts] + [np.zeros((0, 3), f32)], 0)
    if pad_to is not None and p.shape[0] < pad_to:
        far = np.full((pad_to - p.shape[0], 3), 60.0, f32) + np.arange(pad_to - p.shape[0], dtype=f32)[:, None]
        p = np.concatenate([p, far], 0)
    if rng is not None:
        p = p[rng.permutation(p.shape[0])]
    out = np.full((p.shape[0], stride), np.nan, f32)       # NaN in the unread columns
    out[:, :3] = p
    return np.ascontiguousarray(out)


def project(p, cam=CAM, tcv=TCV):
    """(u, v, in_fov) of velodyne points by the rule's arithmetic (the oracle's helpers)."""
    q = LO.affine(np.asarray(tcv, f32).reshape(4, 4)[:3], np.asarray(p, f32).reshape(-1, 3))
    with np.errstate(invalid="ignore", divide="ignore"):
        rx, ry = q[:, 0] / q[:, 2], q[:, 1] / q[:, 2]
        uf = LO.fmaf(f32(cam["fx"]), rx, np.full(rx.shape, cam["cx"], f32))
        vf = LO.fmaf(f32(cam["fy"]), ry, np.full(ry.shape, cam["cy"], f32))
        fov = (q[:, 2] > 0) & (uf > 0) & (uf < f32(cam["width"])) & (vf > 0) & (vf < f32(cam["height"]))
    u, v = np.zeros(uf.shape, np.int64), np.zeros(vf.shape, np.int64)
    u[fov], v[fov] = uf[fov].astype(np.int32), vf[fov].astype(np.int32)
    return u, v, fov


def blank(cam=CAM):
    return np.full((cam["height"], cam["width"]), -1, np.int32)


def paint_rect(inst, p, label, pad=3, cam=CAM, tcv=TCV):
    """Fill the rectangle around the points' pixels (grown by pad) with label."""
    u, v, fov = project(p, cam, tcv)
    assert fov.any()
    l, r = max(int(u[fov].min()) - pad, 0), min(int(u[fov].max()) + pad, cam["width"] - 1)
    t, b = max(int(v[fov].min()) - pad, 0), min(int(v[fov].max()) + pad, cam["height"] - 1)
    inst[t:b + 1, l:r + 1] = label
    return l, t, r, b


def paint_pixels(inst, p, label, cam=CAM, tcv=TCV):
    """Set exactly the points' pixels (which must be distinct and in the image) to label."""
    u, v, fov = project(p, cam, tcv)
    assert fov.all() and len({(a, b) for a, b in zip(u.tolist(), v.tolist())}) == len(u)
    inst[v, u] = label


def counted_rows(k_a, k_b, k_none, labels=(5, 6)):
    """One car seen as k_a + k_b + k_none points on a line: the first k_a project onto pixels of
    labels[0], the next k_b onto labels[1], the rest onto unlabelled pixels."""
    d = det(8.0, 0.5, theta=0.15)
    p = line_points(d, k_a + k_b + k_none)
    inst = blank()
    paint_pixels(inst, p, -1)                                   # asserts distinct pixels in the image
    paint_pixels(inst, p[:k_a], labels[0])
    if k_b:
        paint_pixels(inst, p[k_a:k_a + k_b], labels[1])
    return d, p, inst


def odd_image(w, h):
    """A w x h image mostly of label 1 with bands of label 2, and its camera."""
    v, u = np.mgrid[0:h, 0:w]
    inst = np.where((u + 2 * v) % 7 < 5, 1, 2).astype(np.int32)
    cam = dict(width=w, height=h, fx=0.45 * w, fy=0.9 * h + 20.0, cx=0.5 * w - 0.25, cy=0.5 * h + 0.125)
    return inst, cam


def cases():
    """name -> (velo, instance, masks, dets, cam, t_cam_velo, params); masks: [(label, bbox or None)]."""
    rng = np.random.default_rng(17)
    P = dict(min_mask_area=40)
    c = {}
    cars = [det(8.0, 0.3, theta=0.3), det(9.0, -3.6, theta=-1.2), det(12.0, 6.2, theta=1.5)]

    # ---- a whole small scene: three cars, clutter, a ragged tail (5003 points), stride 4 and 3
    pts = [box_points(d, n, rng) for d, n in zip(cars, (700, 260, 90))]
    inst = blank()
    for i in (2, 0, 1):                                        # nearer cars painted over farther ones
        paint_rect(inst, pts[i], 10 + i)
    masks = [(10, None), (11, None), (12, None)]
    clutter = np.concatenate([above_points(cars[0], 300, rng), rng.uniform(-20, 20, (3000, 3)).astype(f32)], 0)
    scene = pts + [clutter]
    c["scene"] = (sweep(scene, 4, rng, pad_to=5003), inst, masks, cars, CAM, TCV, dict(P))
    c["scene_stride3"] = (sweep(scene, 3, np.random.default_rng(5), pad_to=5003), inst, masks, cars, CAM, TCV, dict(P))
    c["scene_nocap"] = (c["scene"][0], inst, masks, cars, CAM, TCV, dict(P, max_pts=2048, max_bg=1000))
    c["nine"] = (c["scene"][0], inst, masks, [cars[i % 3] for i in range(9)], CAM, TCV, dict(P, max_pts=100))
    c["n_det0"] = (c["scene"][0], inst, masks, [], CAM, TCV, dict(P))
    c["n_masks0"] = (c["scene"][0], inst, [], cars[:1], CAM, TCV, dict(P))
    c["max_bg0"] = (c["scene"][0], inst, masks, cars[:2], CAM, TCV, dict(P, max_bg=0))
    # two detections (the same car, one shifted a little) sharing one mask
    c["shared_mask"] = (c["scene"][0], inst, masks, [cars[0], dict(cars[0], trans=(8.1, 0.25, -1.0))], CAM, TCV, dict(P))
    # the label is listed twice: only entry 0 is ever matched; entry 1's box is never used
    c["dup_label"] = (c["scene"][0], inst, [(10, None), (10, (0, 0, 30, 30)), (11, None)], cars[:2], CAM, TCV, dict(P))
    # a given box away from the mask: the matched label is absent from the box's grid
    c["absent_from_grid"] = (c["scene"][0], inst, [(10, (2, 2, 30, 20)), (11, (100, 30, 400, 500))], cars[:2], CAM,
                             TCV, dict(P))
    area = int((inst == 10).sum())
    c["area_eq"] = (c["scene"][0], inst, masks, cars[:1], CAM, TCV, dict(min_mask_area=area))
    c["area_plus1"] = (c["scene"][0], inst, masks, cars[:1], CAM, TCV, dict(min_mask_area=area - 1))

    # ---- sweep sizes at the chunk and workgroup boundaries: the car's points first, then padding
    car = cars[0]
    inst1 = blank()
    paint_rect(inst1, box_points(car, 400, np.random.default_rng(2)), 3)
    for n in (0, 1, 63, 64, 65, 257):
        p = box_points(car, min(n, 40), np.random.default_rng(100 + n))
        c[f"n_velo{n}"] = (sweep([p], 4 if n % 2 else 3, None, pad_to=n), inst1, [(3, None)], [car], CAM, TCV, dict(P))

    # ---- crop sizes against max_pts (clutter is near but outside the box)
    for name, n_in, mp in (("crop1", 1, 250), ("crop_eq", 250, 250), ("crop_plus1", 251, 250), ("crop1080", 1080, 250),
                           ("crop0", 0, 250)):
        parts = [box_points(car, n_in, np.random.default_rng(7)), above_points(car, 130, np.random.default_rng(8))]
        c[name] = (sweep(parts, 4, np.random.default_rng(9)), inst1, [(3, None)], [car], CAM, TCV, dict(P, max_pts=mp))

    # ---- points exactly on a box face, on the cube face, NaN: theta = 0 keeps the arithmetic exact
    # (x_1 = p_z - o_z with o_z = -0.25, e_1 = 0.75; hi_y = 0.5 + 3); the truck (l = 12) reaches
    # past the cube along y, so the cube cuts it
    truck = det(8.0, 0.5, z=-1.0, w=2.5, l=12.0, h=1.5, theta=0.0)
    on_face = np.array([[8.0, 0.5, 0.5], [8.0, 0.5, 0.5 - 2.0 ** -23],                          # x_1 == e_1 / just inside
                        [8.0, 0.5, -1.0], [8.0, 0.5, np.nextafter(f32(-1.0), f32(0))],          # x_1 == -e_1 / just inside
                        [8.0, 3.5, 0.0], [8.0, np.nextafter(f32(3.5), f32(0)), 0.0],            # p_y == hi_y / just inside
                        [8.0, -2.5, 0.0], [8.0, np.nextafter(f32(-2.5), f32(0)), 0.0],          # p_y == lo_y / just inside
                        [8.0, 5.0, 0.0], [8.0, -4.0, 0.0],                                      # in the box, cut by the cube
                        [np.nan, 0.5, 0.0], [8.0, np.nan, 0.0], [8.0, 0.5, np.nan],             # NaN: in nothing
                        [8.0, 0.5, 0.0]], f32)
    inst2 = blank()
    inst2[:, :] = 4
    c["faces"] = (sweep([on_face], 4), inst2, [(4, None)], [truck], CAM, TCV, dict(P))

    # ---- association counts
    d, p, inst3 = counted_rows(3, 3, 2)
    c["tie"] = (sweep([p], 3), inst3, [(6, None), (5, None)], [d], CAM, TCV, dict(min_mask_area=2))
    d, p, inst3 = counted_rows(4, 0, 4)
    c["half"] = (sweep([p], 3), inst3, [(5, None)], [d], CAM, TCV, dict(min_mask_area=2))
    d, p, inst3 = counted_rows(5, 0, 4)
    c["half_plus1"] = (sweep([p], 3), inst3, [(5, None)], [d], CAM, TCV, dict(min_mask_area=2))

    # ---- rows outside the image, rows behind the image plane, a detection behind the camera
    side = det(5.0, 4.6, theta=0.1)                            # straddles the left image border
    ps = box_points(side, 300, np.random.default_rng(3))
    inst4 = blank()
    paint_rect(inst4, ps, 8)
    c["fov"] = (sweep([ps], 4), inst4, [(8, None)], [side], CAM, TCV, dict(P))
    close = det(0.9, 0.3, l=4.4, theta=math.pi / 2)            # its length axis along velo x, through the image plane
    pc = box_points(close, 300, np.random.default_rng(4))
    inst5 = blank()
    inst5[:, :] = 9
    c["behind_rows"] = (sweep([pc], 4), inst5, [(9, None)], [close], CAM, TCV, dict(P))
    back = det(-8.0, 0.5)
    c["behind"] = (sweep([box_points(back, 100, np.random.default_rng(6)), pts[0]], 4), inst, masks, [back, cars[0]],
                   CAM, TCV, dict(P))

    # ---- odd image sizes: rows of ten 64-pixel chunks plus one pixel; rows shorter than a wave and
    # more rows than one workgroup's four
    for w, h in ((641, 5), (63, 70)):
        io, co = odd_image(w, h)
        c[f"image{w}x{h}"] = (c["scene"][0], io, [(2, None), (1, (3, 1, w - 4, h - 2)), (7, None)], cars, co, TCV,
                              dict(min_mask_area=20, downsample=1, expand=2, max_pts=100, max_bg=64))
    return c


CASE_NAMES = ["scene", "scene_stride3", "scene_nocap", "nine", "n_det0", "n_masks0", "max_bg0", "shared_mask", "dup_label",
              "absent_from_grid", "area_eq", "area_plus1", "n_velo0", "n_velo1", "n_velo63", "n_velo64", "n_velo65",
              "n_velo257", "crop1", "crop_eq", "crop_plus1", "crop1080", "crop0", "faces", "tie", "half", "half_plus1",
              "fov", "behind_rows", "behind", "image641x5", "image63x70"]


def golden_inputs():
    """The fixture's inputs as the entry points take them, and the file."""
    z = np.load(F24)
    w, h = int(z["cam"][0]), int(z["cam"][1])
    cam = dict(width=w, height=h, fx=float(z["cam"][2]), fy=float(z["cam"][3]), cx=float(z["cam"][4]), cy=float(z["cam"][5]))
    masks = np.unpackbits(z["masks"], axis=-1, count=w).astype(bool)
    inst = np.full((h, w), -1, np.int32)
    for lab, m in zip(z["labels"], masks):
        assert np.all(inst[m] == -1)                                       # one label per pixel
        inst[m] = lab
    mlist = [(int(lab), tuple(int(v) for v in b.astype(np.int32))) for lab, b in zip(z["labels"], z["bboxes"])]
    dets = [dict(trans=tuple(r[:3]), size=tuple(r[3:6]), theta=r[6]) for r in z["dets"]]
    names = ("max_pts", "max_bg", "downsample", "expand", "min_mask_area", "radius", "box_margin")
    params = {k: (float(v) if k in ("radius", "box_margin") else int(v)) for k, v in zip(names, z["params"])}
    return z, (z["velo"], inst, mlist, dets, cam, z["t_cam_velo"], params)


def run(entry, velo, inst, masks, dets, cam, tcv, params, ctx=None):
    """Call ``dsr_lidar_inputs_host`` (entry "host") or ``dsr_lidar_inputs`` ("device", with a
    context) with sentinel-filled arrays; returns (rc, pts, rays, dobs, records)."""
    lib = L.load_library()
    cam = U.frame_camera(cam)
    p = U.lidar_params(**params)
    velo, inst, tcv = U.lidar_sweep(velo, inst, cam, tcv)
    n = len(dets)
    ld, keep = U.lidar_dets(dets)
    ml = U.lidar_masks(masks)
    pts = np.full((max(n, 1), p.max_pts, 3), SENTINEL, np.float32)
    rays = np.full((max(n, 1), p.max_pts + p.max_bg, 3), SENTINEL, np.float32)
    dobs = np.full((max(n, 1), p.max_pts), SENTINEL, np.float32)
    out = (L.LidarDetOut * max(n, 1))()
    args = (cam, p, L.fptr(tcv), L.fptr(velo), velo.shape[0], velo.shape[1], L.iptr(inst), len(masks), ml, n, ld,
            L.fptr(pts), L.fptr(rays), L.fptr(dobs), out)
    if entry == "host":
        rc = lib.dsr_lidar_inputs_host(*args)
    else:
        rc = lib.dsr_lidar_inputs(ctx.handle, *args)
    return rc, pts, rays, dobs, [U.lidar_record(out[i]) for i in range(n)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_matches_oracle(velo, inst, masks, dets, cam, tcv, params, result):
    """Arrays bitwise on every counted row, rows beyond the counts untouched, records whole."""
    rc, pts, rays, dobs, recs = result
    assert rc == 0
    before = LO.SUSPECTS
    for i, d in enumerate(dets):
        opts, orays, odobs, orec = LO.ingest(velo, inst, masks, d, cam, tcv, **params)
        assert dict(recs[i]) == orec, (i, recs[i], orec)
        n, m = orec["n_pts"], orec["n_pts"] + orec["n_bg"]
        assert np.array_equal(bits(pts[i, :n]), bits(opts)), i
        assert np.array_equal(bits(rays[i, :m]), bits(orays)), i
        assert np.array_equal(bits(dobs[i, :n]), bits(odobs)), i
        assert np.all(pts[i, n:] == SENTINEL) and np.all(rays[i, m:] == SENTINEL) and np.all(dobs[i, n:] == SENTINEL), i
    if len(dets) < pts.shape[0]:
        assert np.all(pts == SENTINEL) and np.all(rays == SENTINEL) and np.all(dobs == SENTINEL)
    assert LO.SUSPECTS == before, "an emulated fmaf of the oracle sat on a float32 rounding boundary"


def assert_same(a, b):
    """Two ``run`` results agree bitwise (arrays in full, sentinel rows included) and in records."""
    assert a[0] == b[0] == 0
    for x, y in zip(a[1:4], b[1:4]):
        assert np.array_equal(bits(x), bits(y))
    assert a[4] == b[4]
