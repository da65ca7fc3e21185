"""The sphere tracer of ``dsr_renderer_render`` (include/dsr.h) restated in numpy
over any ``sdf(points (n,3)) -> values (n,)`` callable: the pose and rectangle rule, the ray
set-up, the signed march and the nearest-hit composite.  Shared by tests/test_render_cpu.py and
tests/test_gpu_render.py.

The restatement runs in the dtype it is given (float64 by default): it states the algorithm, not
the device's rounding, so it is compared to the device through bounds, never bitwise.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

OK, OFFSCREEN, SKIP_NEAR = 0, 1, 2
DEFAULTS = dict(hit_eps=1e-4, max_steps=48, damp=1.0, near=0.01)


@dataclass
class Camera:
    width: int
    height: int
    fx: float
    fy: float
    cx: float
    cy: float

    def f32(self):
        """the camera as the C ABI carries it (float32 intrinsics), in float64"""
        return Camera(self.width, self.height, *(float(np.float32(v)) for v in (self.fx, self.fy, self.cx, self.cy)))


def pose(t_cam_obj):
    """(T_oc (4,4) f64 rounded once to f32, c (3,), rho) of the float32 pose the C ABI carries:
    T_oc = inverse(t_cam_obj) in float64, the ball's centre c = t[:3,3], radius rho = det(R)^(1/3).
    None for a last row that is not 0 0 0 1 or a determinant <= 0."""
    t = np.asarray(t_cam_obj, np.float32).astype(np.float64).reshape(4, 4)
    if not np.array_equal(t[3], [0.0, 0.0, 0.0, 1.0]):
        return None
    m = t[:3, :3]
    c00 = m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]
    c01 = m[1, 2] * m[2, 0] - m[1, 0] * m[2, 2]
    c02 = m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]
    det = m[0, 0] * c00 + m[0, 1] * c01 + m[0, 2] * c02
    if not (det > 0.0) or not np.isfinite(det):
        return None
    inv = np.array([[c00, m[0, 2] * m[2, 1] - m[0, 1] * m[2, 2], m[0, 1] * m[1, 2] - m[0, 2] * m[1, 1]],
                    [c01, m[0, 0] * m[2, 2] - m[0, 2] * m[2, 0], m[0, 2] * m[1, 0] - m[0, 0] * m[1, 2]],
                    [c02, m[0, 1] * m[2, 0] - m[0, 0] * m[2, 1], m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]]]) / det
    toc = np.eye(4)
    toc[:3, :3] = inv
    toc[:3, 3] = -(inv @ t[:3, 3])
    toc = toc.astype(np.float32).astype(np.float64)
    return toc, t[:3, 3].copy(), float(np.cbrt(det))


def rectangle(cam, near, c, rho):
    """(status, (u_min, v_min, u_max, v_max)) — the conservative box of the ball's projection."""
    cam = cam.f32()
    empty = (0, 0, -1, -1)
    z0, z1 = c[2] - rho, c[2] + rho
    if not (z0 >= near):
        return SKIP_NEAR, empty
    lo, hi = [], []
    for a, (f, pp, size) in enumerate(((cam.fx, cam.cx, cam.width), (cam.fy, cam.cy, cam.height))):
        x0, x1 = c[a] - rho, c[a] + rho
        q = (x0 / z0, x0 / z1, x1 / z0, x1 / z1)
        l, h = np.floor(pp + f * min(q)), np.ceil(pp + f * max(q))
        if l > size - 1 or h < 0:
            return OFFSCREEN, empty
        lo.append(int(max(l, 0.0)))
        hi.append(int(min(h, size - 1.0)))
    return OK, (lo[0], lo[1], hi[0], hi[1])


def layout(cam, near, poses):
    """dsr_render_layout: rect (n,4) int32 and status (n,) int32."""
    near = float(np.float32(near)) if near > 0 else float(np.float32(0.01))
    rect = np.zeros((len(poses), 4), np.int32)
    status = np.zeros(len(poses), np.int32)
    for i, t in enumerate(poses):
        _, c, rho = pose(t)
        status[i], rect[i] = rectangle(cam, near, c, rho)
    return rect, status


@dataclass
class ObjectTrace:
    status: int
    rect: tuple
    u: np.ndarray = None          # (n_rays,) pixel columns / rows of the rectangle, row-major
    v: np.ndarray = None
    d: np.ndarray = None          # (n_rays,3) object-frame ray directions
    o: np.ndarray = None          # (3,) object-frame ray origin
    toc: np.ndarray = None
    ball: np.ndarray = None       # (n_rays,) bool: enters the unit ball
    hit: np.ndarray = None        # (n_rays,) bool
    lam: np.ndarray = None        # (n_rays,) depth of the hit (valid where hit)
    unconverged: np.ndarray = None
    steps: np.ndarray = None      # (n_rays,) decoder evaluations of the ray
    live_per_step: list = None


def trace_object(sdf, cam, t_cam_obj, dtype=np.float64, **params):
    """One object's rays through §3.6b's set-up and march."""
    P = dict(DEFAULTS, **{k: v for k, v in params.items() if v})
    dt = np.dtype(dtype).type
    cam32 = cam.f32()
    toc, c, rho = pose(t_cam_obj)
    status, rect = rectangle(cam, float(np.float32(P["near"])), c, rho)
    tr = ObjectTrace(status, rect, toc=toc)
    if status != OK:
        return tr
    u0, v0, u1, v1 = rect
    vv, uu = np.meshgrid(np.arange(v0, v1 + 1), np.arange(u0, u1 + 1), indexing="ij")
    u, v = uu.reshape(-1), vv.reshape(-1)
    r = np.stack([(u.astype(dt) - dt(cam32.cx)) / dt(cam32.fx), (v.astype(dt) - dt(cam32.cy)) / dt(cam32.fy),
                  np.ones(u.shape[0], dt)], axis=1)
    R, o = toc[:3, :3].astype(dt), toc[:3, 3].astype(dt)
    d = r @ R.T
    a = (d * d).sum(1)
    b = d @ o
    cc = o @ o - dt(1)
    disc = b * b - a * cc
    ball = disc > 0
    sq = np.sqrt(np.where(ball, disc, 0))
    lam0, lam1 = (-b - sq) / a, (-b + sq) / a
    lam = lam0.copy()
    live = ball.copy()
    hit = np.zeros_like(ball)
    steps = np.zeros(u.shape[0], np.int64)
    nd = np.sqrt(a)
    hit_eps, damp = dt(np.float32(P["hit_eps"])), dt(np.float32(P["damp"]))
    live_per_step = []
    for _ in range(int(P["max_steps"])):
        idx = np.nonzero(live)[0]
        live_per_step.append(idx.size)
        if idx.size == 0:
            break
        y = np.asarray(sdf((o + lam[idx, None] * d[idx]).astype(dt)), dt)
        steps[idx] += 1
        h = np.abs(y) < hit_eps
        hit[idx[h]] = True
        live[idx[h]] = False
        m = idx[~h]
        ln = lam[m] + damp * y[~h] / nd[m]
        lam[m] = ln
        live[m] = (ln >= lam0[m]) & (ln <= lam1[m])
    tr.u, tr.v, tr.d, tr.o = u, v, d, o
    tr.ball, tr.hit, tr.lam, tr.unconverged, tr.steps = ball, hit, lam, live.copy(), steps
    tr.live_per_step = live_per_step
    return tr


def render(sdfs, cam, poses, dtype=np.float64, **params):
    """The composite of several objects: depth (H,W) (0 = nothing hit), instance (H,W) int32 (-1 =
    nothing hit; the nearest hit wins, ties go to the lower index) and the per-object traces."""
    depth = np.zeros((cam.height, cam.width), dtype)
    inst = np.full((cam.height, cam.width), -1, np.int32)
    traces = []
    for i, (sdf, t) in enumerate(zip(sdfs, poses)):
        tr = trace_object(sdf, cam, t, dtype, **params)
        traces.append(tr)
        if tr.status != OK:
            continue
        for k in np.nonzero(tr.hit)[0]:
            u, v = tr.u[k], tr.v[k]
            if inst[v, u] < 0 or tr.lam[k] < depth[v, u]:
                depth[v, u] = tr.lam[k]
                inst[v, u] = i
    return depth, inst, traces


def decoder_sdf(dec, code):
    """sdf callable of an oracle Decoder (oracle/dsr_oracle.py) at one latent code"""
    z = np.asarray(code, dec.dtype)

    def f(x):
        x = np.asarray(x, dec.dtype)
        return dec.forward(np.concatenate([np.broadcast_to(z, (x.shape[0], z.shape[0])), x], axis=1))
    return f
