"""The association rule of ``dsr_scene_associate_*`` (include/dsr.h) restated in
numpy: the world transform with exact fused multiply-adds (``lidar_oracle.fmaf``), the strided
layout of the detections in the scene's point buffer, the vote over the candidate records of a
scene query (``scene_oracle.query``'s, or ``SceneSdf.peek``'s) and the pick.  Written forwards from
the rule, not from the C++.  Shared by tests/test_assoc_cpu.py and tests/test_gpu_assoc.py."""
from __future__ import annotations

import numpy as np

import lidar_oracle as LO

MATCHED, NEW, NO_POINTS = 0, 1, 2
DEFAULTS = dict(inlier_tol=0.05, min_hits=20, min_pct=50)
f32 = np.float32


def world(t_world_cam, rows):
    """w_k = fmaf(B_k0, q_x, fmaf(B_k1, q_y, fmaf(B_k2, q_z, b_k))) in float32; None: the rows as they are."""
    rows = np.ascontiguousarray(rows, f32).reshape(-1, 3)
    if t_world_cam is None or rows.shape[0] == 0:
        return rows.copy()
    return LO.affine(np.asarray(t_world_cam, f32).reshape(4, 4)[:3], rows)


def strided(rows, max_pts, t_world_cam=None):
    """Row k of detection j at scene point j * max_pts + k, NaN beyond the detection's count:
    (pts (n_det * max_pts, 3) float32, n_rows (n_det,) int32)."""
    pts = np.full((len(rows), max_pts, 3), np.nan, f32)
    n_rows = np.zeros(len(rows), np.int32)
    for j, r in enumerate(rows):
        w = world(t_world_cam, r)
        assert w.shape[0] <= max_pts
        pts[j, :w.shape[0]] = w
        n_rows[j] = w.shape[0]
    return pts.reshape(-1, 3), n_rows


def vote(cands, n_det, max_pts, inlier_tol=DEFAULTS["inlier_tol"]):
    """``cands``: per object (idx, f) — its candidates' scene-point indices and decoded values.
    Returns n_in, n_hit, n_neg (n_det, n_obj) int32: the detection of a candidate is idx //
    max_pts, a hit has |f| <= inlier_tol, a neg f < -inlier_tol (a NaN f is neither); a float32 f is
    compared in float32."""
    n_obj = len(cands)
    tabs = np.zeros((3, n_det, n_obj), np.int32)
    for i, (idx, f) in enumerate(cands):
        idx = np.asarray(idx, np.int64)
        f = np.asarray(f)
        tol = f32(inlier_tol) if f.dtype == f32 else float(f32(inlier_tol))
        d = idx // max_pts
        with np.errstate(invalid="ignore"):
            hit, neg = np.abs(f) <= tol, f < -tol
        for k, m in enumerate((np.ones(idx.shape, bool), hit, neg)):
            tabs[k, :, i] = np.bincount(d[m], minlength=n_det)[:n_det]
    return tabs[0], tabs[1], tabs[2]


def pick(n_in, n_hit, n_neg, n_rows, inlier_tol=DEFAULTS["inlier_tol"], min_hits=DEFAULTS["min_hits"],
         min_pct=DEFAULTS["min_pct"]):
    """The records: the best object is the first with the largest n_hit, the runner-up the first of
    the others with the largest n_hit; MATCHED iff n_hit >= min_hits and 100 n_hit > min_pct n_pts."""
    out = []
    n_det = len(n_rows)
    n_in, n_hit, n_neg = (np.asarray(t, np.int64) for t in (n_in, n_hit, n_neg))
    assert n_in.shape == n_hit.shape == n_neg.shape and n_hit.ndim == 2 and n_hit.shape[0] == n_det
    for j in range(n_det):
        n = int(n_rows[j])
        hits = [int(x) for x in n_hit[j]]
        best = second = -1
        if hits:
            best = hits.index(max(hits))
            rest = [(h, i) for i, h in enumerate(hits) if i != best]
            if rest:
                top = max(h for h, _ in rest)
                second = min(i for h, i in rest if h == top)
        bh = hits[best] if best >= 0 else 0
        matched = n > 0 and best >= 0 and bh >= min_hits and 100 * bh > min_pct * n
        out.append(dict(status=NO_POINTS if n == 0 else MATCHED if matched else NEW, n_pts=n,
                        obj=best if matched else -1, n_hit=bh,
                        n_in=int(n_in[j][best]) if best >= 0 else 0, n_neg=int(n_neg[j][best]) if best >= 0 else 0,
                        second=second, second_hit=hits[second] if second >= 0 else 0,
                        ingest_status=0, n_mask=0, n_valid=0))
    return out
