"""Scene SDF queries (SceneSdf.query) against what a caller could do before them:
a per-object loop of host binning (numpy, float32) plus sdf_eval(code_i, X_i), composited on the
host — on the same build, same points.

Workload: the suite's synthetic decoder (seed 1234), 16 scale-2 objects on a 4 x 4 grid (spacing 3,
so neighbouring unit balls overlap; z = 0.5 (i % 3 - 1)), codes 0.1 N(0,1) with seeds 100..115,
65,536 world points uniform in the bounding box of the balls (seed 7).  With --grad the loop decodes
every object's winners a second time through sdf_eval(..., with_jac=True) and rotates the gradient
on the host.  Both sides are warmed up, then timed in alternation, --reps rounds; the figures are
medians.  Wall clock is a host clock around calls that end in a device synchronise (copies to the
host included); the query's device-event times come from dsr_scene_stats.  No pass/fail threshold.

Usage (GPU box): python tools/scene_bench.py [--reps 15] [--out profiles/scene.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--out", default=None)
ap.add_argument("--points", type=int, default=65536)
ap.add_argument("--objects", type=int, default=16)
a = ap.parse_args()

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.abspath(os.path.join(REPO, "dsp-slam-rgbd_amd")))
import synthetic as S  # noqa: E402
from deep_sdf.workspace import decoder_from_state  # noqa: E402
from reconstruct.optimizer import SceneSdf, sdf_eval  # noqa: E402

dec = decoder_from_state(S.make_decoder(1234), S.DEFAULT_SPECS)
N, P, SCALE = a.objects, a.points, 2.0
objs = []
for i in range(N):
    T = S.make_object(7 + i, n_pts=8, scale=SCALE, tz=15, perturb=0).t_true.copy()
    T[:3, 3] = (3.0 * (i % 4), 3.0 * ((i // 4) % 4), 0.5 * (i % 3 - 1) + 6.0 * (i // 16))
    objs.append((T.astype(np.float32), (0.1 * np.random.default_rng(100 + i).standard_normal(64)).astype(np.float32)))
cen = np.array([t[:3, 3] for t, _ in objs], np.float64)
lo, hi = cen.min(0) - SCALE, cen.max(0) + SCALE
pts = np.random.default_rng(7).uniform(lo, hi, (P, 3)).astype(np.float32)
scene = SceneSdf(dec, N, P)
scene.set_objects(objs)
inv = []
for t, _ in objs:                                      # the loop's poses, inverted once like the scene's
    ti = np.linalg.inv(t.astype(np.float64))
    s = float(np.cbrt(np.linalg.det(t[:3, :3].astype(np.float64))))
    inv.append((ti[:3, :3].astype(np.float32), ti[:3, 3].astype(np.float32), np.float32(s)))


def loop(grad):
    dist = np.full(P, np.inf, np.float32)
    who = np.full(P, -1, np.int32)
    kept = []
    for i, ((A, t, s), (_, z)) in enumerate(zip(inv, objs)):
        x = pts @ A.T + t
        idx = np.nonzero((x * x).sum(1) < 1.0)[0]
        if idx.size == 0:
            kept.append((idx, x[:0]))
            continue
        xi = np.ascontiguousarray(x[idx])
        d = s * sdf_eval(dec, z, xi)
        better = d < dist[idx]
        dist[idx[better]] = d[better]
        who[idx[better]] = i
        kept.append((idx, xi))
    g = None
    if grad:
        g = np.zeros((P, 3), np.float32)
        for i, ((A, t, s), (_, z)) in enumerate(zip(inv, objs)):
            idx, xi = kept[i]
            mine = who[idx] == i
            if mine.any():
                _, j = sdf_eval(dec, z, np.ascontiguousarray(xi[mine]), with_jac=True)
                g[idx[mine]] = s * (j[:, -3:] @ A)
    return dist, who, g


def med(v):
    return float(np.median(v))


res = {"tool": "tools/scene_bench.py", "objects": N, "points": P, "reps": a.reps,
       "box": {"lo": [float(v) for v in lo], "hi": [float(v) for v in hi]}}
for grad in (False, True):
    modes = {"query": lambda: scene.query(pts, grad=grad), "loop": lambda: loop(grad)}
    first = {}
    for name, fn in modes.items():                     # warm-up (first launches, buffers) + check
        for _ in range(2):
            out = fn()
        first[name] = out
    q, (ld, lw, lg) = first["query"], first["loop"]
    # the loop bins with numpy's matmul, not the fused rule: membership may differ at a ball's rim
    agree = float((q["obj"] == lw).mean())
    both = (q["obj"] == lw) & (lw >= 0)
    worst = float(np.abs(q["dist"][both] - ld[both]).max())
    wall = {k: [] for k in modes}
    dev = {k: [] for k in ("bin_ms", "decode_ms", "resolve_ms", "grad_ms")}
    for _ in range(a.reps):
        for name, fn in modes.items():                 # alternating order
            t0 = time.perf_counter()
            fn()
            wall[name].append(1e3 * (time.perf_counter() - t0))
            if name == "query":
                st = scene.stats()
                for k in dev:
                    dev[k].append(st[k])
    r = {name: {"wall_ms_median": med(wall[name]), "wall_ms_min": float(min(wall[name])),
                "wall_ms_max": float(max(wall[name]))} for name in modes}
    r["query"].update({k: med(v) for k, v in dev.items()})
    r["query"].update({k: st[k] for k in ("n_passes", "pairs", "decoded", "winners")})
    r["same_winner_share"] = agree
    r["worst_dist_difference"] = worst
    res["grad" if grad else "value"] = r
res["unmeasured"] = ["other point counts", "other object counts", "multi-pass calls (k * n_pts above the pair buffers)"]
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(res, fo, indent=1)
        fo.write("\n")
print(json.dumps({"query_ms": res["value"]["query"]["wall_ms_median"], "loop_ms": res["value"]["loop"]["wall_ms_median"],
                  "query_grad_ms": res["grad"]["query"]["wall_ms_median"],
                  "loop_grad_ms": res["grad"]["loop"]["wall_ms_median"],
                  "decoded": res["value"]["query"]["decoded"], "winners": res["value"]["query"]["winners"],
                  "decode_ms": res["value"]["query"]["decode_ms"]}))
