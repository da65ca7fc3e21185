"""The start pose of a detection tracked from a sweep (DESIGN.md §3.5e,
``dsr_lidar_track_prep_host``) restated in python floats, beside ``lidar_oracle.prepare``: python
floats are fp64, every operation rounds on its own, every stored value is rounded to float32 once.
Written forwards from the rule, not from the C++."""
from __future__ import annotations

import math

import numpy as np

f32 = np.float32


def track_prep(det, t_cam_velo, box_margin):
    """One detection ``{trans, size = (w, l, h), theta}`` -> (t_co_se3 (4, 4) float32, det_scale
    float32): t_co_se3 = t_cam_velo [R | o] with R = [[c,0,-s],[-s,0,-c],[0,1,0]], o = (x, y, z +
    h/2), each entry the left-to-right sum over k; det_scale = m l / 2."""
    x, y, z = (float(f32(v)) for v in det["trans"])
    w, l, h = (float(f32(v)) for v in det["size"])
    th = float(f32(det["theta"]))
    C = np.asarray(t_cam_velo, np.float32).reshape(4, 4).astype(np.float64)
    m = float(f32(box_margin))
    c, s = math.cos(th), math.sin(th)
    R = [[c, 0.0, -s], [-s, 0.0, -c], [0.0, 1.0, 0.0]]
    o = [x, y, z + h / 2.0]
    T = np.zeros((4, 4), np.float64)
    for i in range(3):
        for j in range(3):
            acc = 0.0
            for k in range(3):
                acc = acc + float(C[i, k]) * R[k][j]
            T[i, j] = acc
        acc = 0.0
        for k in range(3):
            acc = acc + float(C[i, k]) * o[k]
        T[i, 3] = acc + float(C[i, 3])
    T[3, 3] = 1.0
    return T.astype(f32), f32((m * l) / 2.0)


def t_cam_obj_terms(det, t_cam_velo, box_margin):
    """Sum over k of |t_cam_velo[i, k] sigma R[k, j]| for the rotation block of the rule's
    t_cam_obj (fp64): the size of what a re-ordered fp32 evaluation of an entry adds up."""
    l = float(f32(det["size"][1]))
    th = float(f32(det["theta"]))
    C = np.abs(np.asarray(t_cam_velo, np.float32).reshape(4, 4).astype(np.float64))
    sigma = (float(f32(box_margin)) * l) / 2.0
    c, s = abs(math.cos(th)), abs(math.sin(th))
    R = np.array([[c, 0.0, s], [s, 0.0, c], [0.0, 1.0, 0.0]])
    return C[:3, :3] @ (sigma * R)
