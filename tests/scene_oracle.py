"""The scene query of ``dsr_scene_query`` (include/dsr.h) restated in numpy over
any ``sdf(points (n,3)) -> values (n,)`` callable: the pose rule, the in-ball binning, the nearest
composite, the per-object sums and the world-frame gradient.  Shared by tests/test_scene_cpu.py and
tests/test_gpu_scene.py, with the test scene both use.

The restatement runs in float64 on the float32 inputs the C ABI carries: it states the algorithm,
not the device's rounding, so it is compared to the device through bounds, never bitwise.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

import render_oracle as RO


def pose(t_world_obj):
    """(A (3,3), t (3,), s) of the float32 pose the C ABI carries, as float64 values: T_ow =
    inverse(t_world_obj) in float64 (adjugate / determinant) rounded once to float32, s =
    det(R)^(1/3) rounded once.  None for a non-finite entry, a last row that is not 0 0 0 1 or a
    determinant <= 0."""
    t = np.asarray(t_world_obj, np.float32).reshape(4, 4)
    if not np.all(np.isfinite(t)):
        return None
    p = RO.pose(t)
    if p is None:
        return None
    tow, _, rho = p
    return tow[:3, :3].copy(), tow[:3, 3].copy(), float(np.float32(rho))


def transform(t_world_obj, pts_world):
    """x = A p + t in float64, and the per-coordinate magnitude 1 + sum_j |A_kj p_j| + |t_k| that
    bounds a float32 evaluation's error (x 1e-6)."""
    A, t, _ = pose(t_world_obj)
    p = np.asarray(pts_world, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        x = p @ A.T + t
        mag = 1.0 + np.abs(p) @ np.abs(A).T + np.abs(t)
    return x, mag


def bin_object(t_world_obj, pts_world):
    """(idx, x (len(idx),3), s, r2 (n,)): the points with r2 = |x|^2 < 1, in point order.  A point
    with a non-finite coordinate is in no ball."""
    x, _ = transform(t_world_obj, pts_world)
    with np.errstate(invalid="ignore", over="ignore"):
        r2 = (x * x).sum(1)
    ok = np.isfinite(np.asarray(pts_world, np.float64)).all(1)
    r2 = np.where(ok, r2, np.inf)
    idx = np.nonzero(r2 < 1.0)[0].astype(np.int32)
    return idx, x[idx], pose(t_world_obj)[2], r2


@dataclass
class ObjectRecord:
    idx: np.ndarray                 # candidates' point indices, in point order
    x: np.ndarray                   # their object-frame coordinates
    f: np.ndarray                   # their decoded values
    s: float
    r2: np.ndarray                  # (n,) squared norm of every point in the object's frame
    n_win: int = 0

    @property
    def n_in(self):
        return int(self.idx.size)

    @property
    def n_neg(self):
        return int((self.f < 0).sum())

    @property
    def n_nan(self):
        return int(np.isnan(self.f).sum())

    @property
    def sum_sdf(self):
        return float(self.f[~np.isnan(self.f)].sum())

    @property
    def sum_abs(self):
        return float(np.abs(self.f[~np.isnan(self.f)]).sum())


@dataclass
class Result:
    dist: np.ndarray
    obj: np.ndarray
    grad: np.ndarray
    objects: list = field(default_factory=list)
    d_all: np.ndarray = None        # (n_obj, n) s f, +inf outside the ball or where f is NaN


def query(sdfs, poses, pts_world, grads=None):
    """The composite of several objects: dist (n,) (+inf in no ball), obj (n,) int32 (-1 in no ball;
    the smallest s f wins, ties go to the lower index), grad (n,3) = s A^T g = R g at the winners
    (``grads``: per object a callable points -> df/dx (n,3); zeros without it) and the records."""
    pts = np.asarray(pts_world, np.float32)
    n = pts.shape[0]
    d_all = np.full((len(poses), n), np.inf)
    recs = []
    for i, (sdf, t) in enumerate(zip(sdfs, poses)):
        idx, x, s, r2 = bin_object(t, pts)
        f = np.asarray(sdf(x), np.float64) if idx.size else np.zeros(0)
        recs.append(ObjectRecord(idx, x, f, s, r2))
        d = s * f
        d_all[i, idx] = np.where(np.isnan(d), np.inf, d)
    dist = np.full(n, np.inf)
    obj = np.full(n, -1, np.int32)
    if len(poses):
        win = d_all.argmin(0)                      # the first minimum: ties go to the lower index
        best = d_all[win, np.arange(n)]
        # a candidate always wins over no candidate, also at +inf
        has = np.zeros(n, bool)
        for i, r in enumerate(recs):
            ok = np.zeros(n, bool)
            ok[r.idx[~np.isnan(r.f)]] = True
            has |= ok
        dist = np.where(has, best, np.inf)
        obj = np.where(has, win, -1).astype(np.int32)
    grad = np.zeros((n, 3))
    for i, r in enumerate(recs):
        mine = obj[r.idx] == i
        r.n_win = int(mine.sum())
        if grads is not None and mine.any():
            A, _, s = pose(poses[i])
            g = np.asarray(grads[i](r.x[mine]), np.float64)
            grad[r.idx[mine]] = s * (g @ A)        # row-wise s A^T g
    return Result(dist, obj, grad, recs, d_all)


def decoder_sdf(dec, code):
    """sdf callable of an oracle Decoder (oracle/dsr_oracle.py) at one latent code"""
    return RO.decoder_sdf(dec, code)


def decoder_grad(dec, code):
    """df/dx callable of an oracle Decoder at one latent code"""
    z = np.asarray(code, dec.dtype)

    def g(x):
        x = np.asarray(x, dec.dtype)
        _, j = dec.forward_jac(np.concatenate([np.broadcast_to(z, (x.shape[0], z.shape[0])), x], axis=1))
        return j[:, -3:]
    return g


# ---- the test scene (tests/test_scene_cpu.py, tests/test_gpu_scene.py) --------------------------
SCALES = (2.0, 1.5, 1.0, 2.5)
CENTRES = ((0.0, 0.0, 0.0), (2.2, 0.3, -0.4), (-1.1, 1.6, 0.5), (0.8, -2.0, 1.0))
CODE_SCALES = (0.0, 0.1, 0.3, 0.3)
COUNTS = {1500: (480, 194, 56, 598), 400: (141, 53, 17, 152)}


def rotation(i):
    """the rotation of the unit quaternion default_rng(40 + i).standard_normal(4) (w, x, y, z)"""
    q = np.random.default_rng(40 + i).standard_normal(4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def scene_pose(i, scale=None, centre=None):
    T = np.eye(4)
    T[:3, :3] = (SCALES[i] if scale is None else scale) * rotation(i)
    T[:3, 3] = CENTRES[i] if centre is None else centre
    return T.astype(np.float32)


def scene_code(i, n=64):
    return (CODE_SCALES[i % 4] * np.random.default_rng(100 + i).standard_normal(n)).astype(np.float32)


def scene_objects(n=4, code_len=64):
    return [(scene_pose(i), scene_code(i, code_len)) for i in range(n)]


def scene_points(n):
    return np.random.default_rng(7).uniform((-2, -3, -1.5), (3.2, 2.6, 2), (n, 3)).astype(np.float32)
