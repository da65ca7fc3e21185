"""The association test scene (tests/test_assoc_cpu.py, tests/test_gpu_assoc.py), built on the CPU
alone: the four objects of ``scene_oracle.scene_objects()`` and six detections of world rows at
``max_pts = 65`` — points projected onto an object's zero level with the float64 oracle decoder,
mixed with the scene's uniform points — with what the float64 restatement says about them."""
from __future__ import annotations

import numpy as np

import assoc_oracle as AO
import scene_oracle as SO

MAX_PTS = 65
N_DET, N_OBJ = 6, 4
COUNTS = (116, 44, 53, 94)                     # candidates per object
N_HIT = ((65, 0, 0, 0), (0, 0, 0, 41), (1, 0, 0, 0), (0, 0, 0, 0), (0, 33, 32, 0), (0, 0, 21, 0))
N_IN = ((65, 6, 0, 31), (15, 2, 0, 50), (8, 3, 0, 8), (0, 0, 0, 0), (15, 33, 32, 5), (13, 0, 21, 0))
N_ROWS = (65, 65, 30, 0, 65, 21)
#: (status, obj, second, second_hit) at the defaults
DECISIONS = ((AO.MATCHED, 0, 1, 0), (AO.MATCHED, 3, 0, 0), (AO.NEW, -1, 1, 0), (AO.NO_POINTS, -1, 1, 0),
             (AO.MATCHED, 1, 2, 32), (AO.MATCHED, 2, 0, 0))
F_TOL = 2e-5                                   # the exact kernel against fp64 on f (tests/test_gpu_scene.py)
_CACHE = {}


def surface(dec64, i, n, seed):
    """n world points on object i's zero level: 4n points uniform in [-0.6, 0.6]^3, four Newton
    steps x -= f g / max(|g|^2, 1e-6) with the float64 decoder, the first n with |f| < 2e-3 and
    |x|^2 < 0.8, mapped by scene_pose(i) in float64 and rounded to float32."""
    z = SO.scene_code(i)
    sdf, grad = SO.decoder_sdf(dec64, z), SO.decoder_grad(dec64, z)
    x = np.random.default_rng(seed).uniform(-0.6, 0.6, (4 * n, 3))
    for _ in range(4):
        f = np.asarray(sdf(x), np.float64)
        g = np.asarray(grad(x), np.float64)
        x = x - f[:, None] * g / np.maximum((g * g).sum(1), 1e-6)[:, None]
    f = np.asarray(sdf(x), np.float64)
    keep = np.nonzero((np.abs(f) < 2e-3) & ((x * x).sum(1) < 0.8))[0][:n]
    assert keep.shape[0] == n, (i, n, seed, keep.shape[0])
    T = SO.scene_pose(i).astype(np.float64)
    return (x[keep] @ T[:3, :3].T + T[:3, 3]).astype(np.float32)


def detections(dec64):
    """the six detections' world rows"""
    if "rows" not in _CACHE:
        rnd = SO.scene_points(400)
        _CACHE["rows"] = [surface(dec64, 0, 65, 1),
                          np.concatenate([surface(dec64, 3, 40, 2), rnd[:25]]),
                          rnd[100:130].copy(),
                          np.zeros((0, 3), np.float32),
                          np.concatenate([surface(dec64, 1, 33, 3), surface(dec64, 2, 32, 4)]),
                          surface(dec64, 2, 21, 5)]
    return [r.copy() for r in _CACHE["rows"]]


def oracle(dec64):
    """(strided points, n_rows, the float64 scene query on them, (n_in, n_hit, n_neg)): computed once"""
    if "oracle" not in _CACHE:
        objs = SO.scene_objects()
        pts, n_rows = AO.strided(detections(dec64), MAX_PTS)
        ref = SO.query([SO.decoder_sdf(dec64, z) for _, z in objs], [t for t, _ in objs], pts)
        tabs = AO.vote([(r.idx, r.f) for r in ref.objects], N_DET, MAX_PTS)
        _CACHE["oracle"] = (pts, n_rows, ref, tabs)
    return _CACHE["oracle"]


def assert_conditions(dec64):
    """what makes exact equality with the GPU legitimate; a changed recipe fails here"""
    pts, n_rows, ref, (n_in, n_hit, n_neg) = oracle(dec64)
    assert tuple(int(n) for n in n_rows) == N_ROWS
    assert tuple(r.n_in for r in ref.objects) == COUNTS
    assert np.array_equal(n_hit, np.asarray(N_HIT)) and np.array_equal(n_in, np.asarray(N_IN))
    f = np.concatenate([r.f for r in ref.objects])
    tol = float(np.float32(AO.DEFAULTS["inlier_tol"]))
    margin_f = np.abs(np.abs(f) - tol).min()
    r2 = np.stack([r.r2 for r in ref.objects])
    margin_r = np.abs(r2[np.isfinite(r2)] - 1.0).min()
    print(f"smallest ||f| - tol| {margin_f:.3e}, smallest |r^2 - 1| {margin_r:.3e}")
    assert margin_f > 5e-3 and margin_r > 4e-4          # far above F_TOL: no membership, no class can flip
    # object 0's two tiles hold four detections' candidates; two objects stay under one tile
    assert len(set((ref.objects[0].idx // MAX_PTS).tolist())) >= 4
    assert sum(c < 64 for c in COUNTS) == 2
    recs = AO.pick(n_in, n_hit, n_neg, n_rows)
    assert tuple((r["status"], r["obj"], r["second"], r["second_hit"]) for r in recs) == DECISIONS
    assert AO.pick(n_in, n_hit, n_neg, n_rows, min_hits=22)[5]["status"] == AO.NEW
    return recs
