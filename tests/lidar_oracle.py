"""The LiDAR-ingest rule restated in numpy / python floats: fp64 preparation
with one rounding per stored value, float32 crop and rows with exact fused multiply-adds, integer
``sel`` and counts.  Written forwards from the rule, not from the C++; the lidar tests compare
``dsr_lidar_inputs_host`` (and through it the device kernels) with it bitwise.

``fmaf`` is emulated through fp64: the product of two float32 is exact in fp64, the sum is rounded
to fp64 and then to float32.  The two roundings differ from the single one only when the fp64 sum
was itself rounded and landed exactly half-way between two float32 values; ``SUSPECTS`` counts
those, and the tests assert it stays 0 on their fixtures."""
from __future__ import annotations

import math

import numpy as np

import frame_oracle as FO

OK, BEHIND, NO_POINTS, NO_MATCH, SMALL_MASK = 0, 1, 2, 3, 4
DEFAULTS = dict(max_pts=250, max_bg=200, downsample=4, expand=5, min_mask_area=1000, radius=3.0, box_margin=1.1)
MAX_MASKS = 256
f32 = np.float32

SUSPECTS = 0      # fp64 sums that sit on a float32 rounding boundary (see the module docstring)


def fmaf(a, b, c):
    """float32 fma(a, b, c) of float32 arrays, one rounding."""
    global SUSPECTS
    a, b, c = (np.asarray(x, np.float32).astype(np.float64) for x in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        ab = a * b                                    # exact: 24 x 24 bits
        r = ab + c
        t = r - ab
        err = (ab - (r - t)) + (c - t)                # the fp64 sum's rounding error, exactly (TwoSum)
    r1, e1 = np.atleast_1d(r), np.atleast_1d(err)
    half_way = (r1.view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)
    SUSPECTS += int((np.isfinite(r1) & half_way & (e1 != 0)).sum())
    with np.errstate(over="ignore"):
        return r.astype(np.float32)


def affine(M, p):
    """Row k: fmaf(M_k0, p_x, fmaf(M_k1, p_y, fmaf(M_k2, p_z, M_k3))) for points p (n, 3); M (3, 4) float32."""
    return np.stack([fmaf(M[k, 0], p[:, 0], fmaf(M[k, 1], p[:, 1], fmaf(M[k, 2], p[:, 2], np.full(p.shape[0], M[k, 3], f32))))
                     for k in range(3)], 1)


def prepare(det, t_cam_velo, P):
    """The host preparation of one detection ``{trans, size, theta}``: python floats are fp64, every
    operation rounds on its own, every stored value is rounded to float32 once."""
    x, y, z = (float(f32(v)) for v in det["trans"])
    w, l, h = (float(f32(v)) for v in det["size"])
    th = float(f32(det["theta"]))
    C = np.asarray(t_cam_velo, np.float32).reshape(4, 4).astype(np.float64)
    m, rad = float(f32(P["box_margin"])), float(f32(P["radius"]))
    c, s = math.cos(th), math.sin(th)
    R = [[c, 0.0, -s], [-s, 0.0, -c], [0.0, 1.0, 0.0]]
    hh = h / 2.0
    o = [x, y, z + hh]
    A = np.array([[R[j][i] for j in range(3)] for i in range(3)], np.float64).astype(f32)
    t = np.array([-(c * o[0] - s * o[1]), -o[2], s * o[0] + c * o[1]], np.float64).astype(f32)
    lo = np.array([x - rad, y - rad, z - rad], np.float64).astype(f32)
    hi = np.array([x + rad, y + rad, z + rad], np.float64).astype(f32)
    sigma = (m * l) / 2.0
    e = np.array([(m * w) / 2.0, hh, sigma], np.float64).astype(f32)
    T = np.zeros((4, 4), np.float64)
    for i in range(3):
        for j in range(3):
            acc = 0.0
            for k in range(3):
                acc = acc + float(C[i, k]) * (sigma * R[k][j])
            T[i, j] = acc
        acc = 0.0
        for k in range(3):
            acc = acc + float(C[i, k]) * o[k]
        T[i, 3] = acc + float(C[i, 3])
    T[3, 3] = 1.0
    return dict(A=np.concatenate([A, t[:, None]], 1), lo=lo, hi=hi, e=e, t_cam_obj=T.astype(f32))


def crop_rows(p, L, P):
    """(near flags, n_crop, sweep indices of the kept rows in row order) of points p (n, 3) float32."""
    with np.errstate(invalid="ignore"):
        near = np.all((L["lo"][None, :] < p) & (p < L["hi"][None, :]), 1)
        x = affine(L["A"], p)
        inside = near & np.all((-L["e"][None, :] < x) & (x < L["e"][None, :]), 1)
    crop = np.nonzero(inside)[0]
    n_crop = int(crop.shape[0])
    pick = crop[np.asarray(FO.sel(P["max_pts"], n_crop), np.int64)] if n_crop else crop
    return near, n_crop, pick


def ingest(velo, instance, masks, det, cam, t_cam_velo, **params):
    """One detection -> (pts, rays, dobs, record): pts / dobs have the record's n_pts rows, rays
    n_pts + n_bg.  ``masks``: list of ``(label, bbox or None)``."""
    P = dict(DEFAULTS, **params)
    H, W = instance.shape
    L = prepare(det, t_cam_velo, P)
    C = np.asarray(t_cam_velo, np.float32).reshape(4, 4)
    p = np.ascontiguousarray(velo[:, :3], np.float32)
    near, n_crop, pick = crop_rows(p, L, P)
    n_pts = int(pick.shape[0])
    q = affine(C[:3], p[pick]) if n_pts else np.zeros((0, 3), f32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        fg = np.stack([q[:, 0] / q[:, 2], q[:, 1] / q[:, 2], np.ones(n_pts, f32)], 1).astype(f32)
        uf = fmaf(f32(cam["fx"]), fg[:, 0], np.full(n_pts, cam["cx"], f32))
        vf = fmaf(f32(cam["fy"]), fg[:, 1], np.full(n_pts, cam["cy"], f32))
        fov = (q[:, 2] > 0) & (uf > 0) & (uf < f32(W)) & (vf > 0) & (vf < f32(H))
    n_proj = int(fov.sum())
    labels = instance[vf[fov].astype(np.int32), uf[fov].astype(np.int32)]
    hits = [0] * len(masks)
    for lab in labels.tolist():
        for j, (mlab, _) in enumerate(masks):
            if mlab == lab:
                hits[j] += 1
                break
    best = hits.index(max(hits)) if hits else -1
    n_hits = hits[best] if hits else 0
    matched = best >= 0 and 2 * n_hits > n_proj
    T = L["t_cam_obj"]
    rec = dict(status=OK, n_near=int(near.sum()), n_crop=n_crop, n_pts=n_pts, n_proj=n_proj,
               mask=best if matched else -1, n_hits=n_hits, n_mask_px=0, n_bg=0, box=(0, 0, -1, -1), grid_h=0,
               grid_w=0, t_cam_obj=tuple(float(v) for v in T.reshape(16)))
    bg = np.zeros((0, 3), f32)
    status = BEHIND if T[2, 3] <= 0 else NO_POINTS if n_crop == 0 else NO_MATCH if not matched else OK
    if matched:
        label, bbox = masks[best]
        # the frame rule's box, grid and background rays for this label (a depth image valid everywhere
        # keeps its status on the mask alone)
        _, frays, _, frec = FO.ingest(np.ones((H, W), f32), instance, dict(label=label, bbox=bbox), cam,
                                      max_pts=1, max_bg=P["max_bg"], downsample=P["downsample"], expand=P["expand"],
                                      min_mask_area=P["min_mask_area"])
        rec.update(n_mask_px=frec["n_mask"], box=frec["box"], grid_h=frec["grid_h"], grid_w=frec["grid_w"])
        if status == OK and frec["n_mask"] <= P["min_mask_area"]:
            status = SMALL_MASK
        if status == OK:
            bg = frays[1:]
            rec["n_bg"] = int(bg.shape[0])
    rec["status"] = status
    return q.astype(f32), np.concatenate([fg, bg], 0), q[:, 2].astype(f32), rec


def ingest_all(velo, instance, masks, dets, cam, t_cam_velo, **params):
    return [ingest(velo, instance, masks, d, cam, t_cam_velo, **params) for d in dets]
