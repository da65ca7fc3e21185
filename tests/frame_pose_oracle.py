"""The cuboid start-pose rule restated in numpy and Python floats on top of
``frame_oracle.ingest``: fp64 on the fp32 rows, one rounded operation at a time, sums as 256
strided partials added in index order.  Written from the rule, not from the C++; the frame-pose
tests compare ``dsr_frame_poses_host`` (and through it the device kernels) with it bitwise."""
from __future__ import annotations

import math

import numpy as np

import frame_oracle as FO

GIVEN, CUBOID, CUBOID_FLIPPED = 0, 1, 2
OK, NOT_ASKED, NO_INPUT, FEW_POINTS, DEGENERATE = 0, 1, 2, 3, 4
DEFAULTS = dict(outlier_radius=1.0, lo_pct=5, hi_pct=95, box_margin=1.2, scale_factor=0.40, min_points=50,
                up=(0.0, -1.0, 0.0))
LANES = 256


def strided_sum(terms, use=None):
    """Σ terms[i] over the points with use[i]: partial j adds points j, j+256, ... in order from 0,
    then the partials are added in index order.  (Adding +0.0 for a skipped point changes nothing.)"""
    t = np.asarray(terms, np.float64)
    if use is not None:
        t = np.where(use, t, 0.0)
    pad = (-t.shape[0]) % LANES
    t = np.concatenate([t, np.zeros(pad)]).reshape(-1, LANES)
    part = np.zeros(LANES)
    for row in t:
        part = part + row
    s = 0.0
    for x in part.tolist():
        s = s + x
    return s


def jacobi(C):
    """10 cyclic sweeps over (0,1), (0,2), (1,2) from V = I, in the statement order of §3.5c."""
    A = [[float(C[i][j]) for j in range(3)] for i in range(3)]
    V = [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]

    def rot(c, s, a, b):
        return c * a - s * b, s * a + c * b

    for _ in range(10):
        for p, q in ((0, 1), (0, 2), (1, 2)):
            apq = A[p][q]
            if apq == 0.0:
                continue
            theta = (A[q][q] - A[p][p]) / (2.0 * apq)
            t = 1.0 / (abs(theta) + math.sqrt(theta * theta + 1.0))
            if theta < 0.0:
                t = -t
            c = 1.0 / math.sqrt(t * t + 1.0)
            s = t * c
            for k in range(3):
                A[k][p], A[k][q] = rot(c, s, A[k][p], A[k][q])
            for k in range(3):
                A[p][k], A[q][k] = rot(c, s, A[p][k], A[q][k])
            for k in range(3):
                V[k][p], V[k][q] = rot(c, s, V[k][p], V[k][q])
    d = [A[0][0], A[1][1], A[2][2]]
    idx = [0, 1, 2]
    for i in range(1, 3):                          # ascending, ties by index
        j = i
        while j > 0 and d[idx[j - 1]] > d[idx[j]]:
            idx[j - 1], idx[j] = idx[j], idx[j - 1]
            j -= 1
    return [d[k] for k in idx], [[V[r][k] for r in range(3)] for k in idx]


def axes(v, up):
    """Eigenvectors v0, v1, v2 -> R (3x3 nested lists)."""
    v0, v1, v2 = [list(x) for x in v]
    big = 0
    for r in (1, 2):
        if abs(v2[r]) > abs(v2[big]):
            big = r
    if v2[big] < 0.0:
        v2 = [-x for x in v2]
    R = [[v1[r], v0[r], -v2[r]] for r in range(3)]
    det = (R[0][0] * (R[1][1] * R[2][2] - R[1][2] * R[2][1]) - R[0][1] * (R[1][0] * R[2][2] - R[1][2] * R[2][0])
           + R[0][2] * (R[1][0] * R[2][1] - R[1][1] * R[2][0]))
    if det < 0.0:
        for r in range(3):
            R[r][0] = -R[r][0]
    u = [float(np.float32(x)) for x in up]
    if u[0] * R[0][1] + u[1] * R[1][1] + u[2] * R[2][1] < 0.0:
        for r in range(3):
            R[r][0], R[r][1] = -R[r][0], -R[r][1]
    return R


def blank(status, n_in):
    return dict(status=status, n_in=n_in, n_near=0, n_kept=0, dims=np.zeros(3), eig=np.zeros(3),
                t_cam_obj=np.eye(4, dtype=np.float32))


def pose(pts, rays, dobs, n_bg, flipped, **pose_params):
    """The rule on one detection's ingested rows -> (pts, rays, dobs, record); empty arrays and the
    identity unless the status is OK."""
    Q = dict(DEFAULTS, **pose_params)
    f32 = np.float32
    none = (np.zeros((0, 3), f32), np.zeros((0, 3), f32), np.zeros(0, f32))
    n_in = pts.shape[0]
    rec = blank(FEW_POINTS, n_in)
    P = pts.astype(np.float64)
    m0 = [strided_sum(P[:, k]) / float(n_in) for k in range(3)]
    radius = float(f32(Q["outlier_radius"]))
    dx, dy, dz = P[:, 0] - m0[0], P[:, 1] - m0[1], P[:, 2] - m0[2]
    near = (dx * dx + dy * dy) + dz * dz <= radius * radius
    n_near = int(near.sum())
    rec["n_near"] = n_near
    if n_in < Q["min_points"] or n_near < Q["min_points"]:
        return none + (rec,)
    m1 = [strided_sum(P[:, k], near) / float(n_near) for k in range(3)]
    D = [P[:, k] - m1[k] for k in range(3)]
    C = [[0.0] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(i, 3):
            C[i][j] = C[j][i] = strided_sum(D[i] * D[j], near)
    eig, v = jacobi(C)
    rec["eig"] = np.asarray(eig, np.float64)
    R = axes(v, Q["up"])
    Pn = P[near]
    q = [((R[0][a] * Pn[:, 0] + R[1][a] * Pn[:, 1]) + R[2][a] * Pn[:, 2]) + 0.0 for a in range(3)]
    lo, hi = (n_near * Q["lo_pct"]) // 100, (n_near * Q["hi_pct"]) // 100
    qs = [np.sort(x) for x in q]
    qlo, qhi = [float(x[lo]) for x in qs], [float(x[hi]) for x in qs]
    with np.errstate(all="ignore"):
        dims = [qhi[a] - qlo[a] for a in range(3)]
        co = [(qhi[a] + qlo[a]) / 2.0 for a in range(3)]
        cc = [(R[k][0] * co[0] + R[k][1] * co[1]) + R[k][2] * co[2] for k in range(3)]
    rec["dims"] = np.asarray(dims, np.float64)
    everything = eig + dims + co + cc + [x for row in R for x in row]
    if dims[2] == 0.0 or not all(math.isfinite(x) for x in everything):
        rec["status"] = DEGENERATE
        return none + (rec,)
    margin = float(f32(Q["box_margin"]))
    with np.errstate(all="ignore"):
        half = [(margin * dims[a]) / 2.0 for a in range(3)]
        outlier = np.zeros(n_near, bool)
        for a in range(3):
            outlier |= np.abs(q[a] - co[a]) > half[a]
    kept = np.nonzero(near)[0][~outlier]
    rec["n_kept"] = int(kept.shape[0])
    if rec["n_kept"] < Q["min_points"]:
        return none + (rec,)
    rec["status"] = OK
    T = np.eye(4, dtype=f32)
    sl = float(f32(Q["scale_factor"])) * dims[2]
    for k in range(3):
        for j in range(3):
            T[k, j] = f32(sl * R[k][j])
        T[k, 3] = f32(cc[k])
    if flipped:
        T[:3, 0], T[:3, 2] = -T[:3, 0], -T[:3, 2]
    rec["t_cam_obj"] = T
    return pts[kept], np.concatenate([rays[kept], rays[n_in:n_in + n_bg]], 0), dobs[kept], rec


def poses(depth, instance, dets, modes, cam, pose_params=None, **params):
    """Per detection (pts, rays, dobs, ingest record, pose record)."""
    out = []
    for det, mode in zip(dets, modes):
        pts, rays, dobs, rec = FO.ingest(depth, instance, det, cam, **params)
        if mode == GIVEN:
            prec = blank(NOT_ASKED, rec["n_pts"])
            prec["t_cam_obj"] = np.asarray(det["t_cam_obj"], np.float32).reshape(4, 4)
        elif rec["status"] != FO.OK:
            prec = blank(NO_INPUT, 0)
        else:
            pts, rays, dobs, prec = pose(pts, rays, dobs, rec["n_bg"], mode == CUBOID_FLIPPED, **(pose_params or {}))
        out.append((pts, rays, dobs, rec, prec))
    return out
