"""The frame-ingest rule restated in numpy: integer ``sel``, float32 operations
in the stated order.  Written from the rule, not from the C++; the frame tests compare
``dsr_frame_inputs_host`` (and through it the device kernels) with it bitwise."""
from __future__ import annotations

import numpy as np

OK, NO_MASK, SMALL_MASK, NO_DEPTH = 0, 1, 2, 3
DEFAULTS = dict(max_pts=250, max_bg=200, downsample=4, expand=5, min_mask_area=1000, near=0.01, far=np.inf)


def sel(n, N):
    """Indices sel(i, n, N), i = 0..n-1 (python integers: exact); the identity unless N > n."""
    if N <= n:
        return list(range(N))
    if n == 1:
        return [0]
    return [(i * (N - 1)) // (n - 1) for i in range(n)]


def rays_of(u, v, cam):
    """float32 rays ((u - cx) / fx, (v - cy) / fy, 1), one rounded operation each."""
    f32 = np.float32
    rx = (u.astype(f32) - f32(cam["cx"])) / f32(cam["fx"])
    ry = (v.astype(f32) - f32(cam["cy"])) / f32(cam["fy"])
    return np.stack([rx, ry, np.ones_like(rx)], 1).astype(f32)


def ingest(depth, instance, det, cam, **params):
    """One detection ``{label, bbox=None}`` -> (pts, rays, dobs, record)."""
    P = dict(DEFAULTS, **params)
    H, W = instance.shape
    label = det["label"]
    mask = instance == label
    z = depth.astype(np.float32)
    with np.errstate(invalid="ignore"):
        valid = mask & (z == z) & (z > np.float32(P["near"])) & (z < np.float32(P["far"]))
    n_mask, n_valid = int(mask.sum()), int(valid.sum())
    status = NO_MASK if n_mask == 0 else SMALL_MASK if n_mask <= P["min_mask_area"] else \
        NO_DEPTH if n_valid == 0 else OK
    # box
    bbox = det.get("bbox")
    box = None
    if bbox is not None and bbox[2] >= bbox[0]:
        l, t, r, b = max(bbox[0], 0), max(bbox[1], 0), min(bbox[2], W - 1), min(bbox[3], H - 1)
        if l <= r and t <= b:
            box = (l, t, r, b)
    elif n_mask:
        vs, us = np.nonzero(mask)
        box = (int(us.min()), int(vs.min()), int(us.max()), int(vs.max()))
    gh = gw = 0
    if box is not None:
        l, t, r, b = box
        e = P["expand"]
        l = l - e if l > e else 0
        t = t - e if t > e else 0
        r = r + e if r < W - 1 - e else W - 1
        b = b + e if b < H - 1 - e else H - 1
        box = (l, t, r, b)
        gh, gw = (b - t + 1) // P["downsample"], (r - l + 1) // P["downsample"]
    rec = dict(status=status, n_mask=n_mask, n_valid=n_valid, n_pts=0, n_bg=0,
               box=box if box is not None else (0, 0, -1, -1), grid_h=gh, grid_w=gw)
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), np.zeros(0, np.float32), rec)
    if status != OK:
        return empty
    # foreground
    vv, uu = np.nonzero(valid)                      # row-major order
    pick = np.asarray(sel(P["max_pts"], n_valid), np.int64)
    u, v = uu[pick], vv[pick]
    fg = rays_of(u, v, cam)
    zz = z[v, u]
    pts = np.stack([fg[:, 0] * zz, fg[:, 1] * zz, zz], 1).astype(np.float32)
    # background
    bg = np.zeros((0, 3), np.float32)
    if gh > 0 and gw > 0 and P["max_bg"] > 0:
        l, t, r, b = box
        rows = t + np.asarray(sel(gh, b - t + 1), np.int64)
        cols = l + np.asarray(sel(gw, r - l + 1), np.int64)
        gv, gu = np.meshgrid(rows, cols, indexing="ij")
        gv, gu = gv.reshape(-1), gu.reshape(-1)
        keep = instance[gv, gu] != label
        gv, gu = gv[keep], gu[keep]
        pick = np.asarray(sel(P["max_bg"], gv.shape[0]), np.int64)
        if pick.size:
            bg = rays_of(gu[pick], gv[pick], cam)
    rec["n_pts"], rec["n_bg"] = pts.shape[0], bg.shape[0]
    return pts, np.concatenate([fg, bg], 0), zz.astype(np.float32), rec


def ingest_all(depth, instance, dets, cam, **params):
    return [ingest(depth, instance, d, cam, **params) for d in dets]
