"""Data association in one device call (SceneSdf.associate_frame) against what a
caller could do before it, on the same build and the same frame: utils.frame_inputs (the ingest
rule on the host, with max_bg = 0: no background rays are picked), a numpy transform of the rows to the world, SceneSdf.query on the strided
points, SceneSdf.peek per object and the vote and the pick counted in numpy.

Workload: the suite's synthetic decoder (seed 1234); a 640 x 480 frame (fx = fy = 500) rendered by
SdfRenderer from 8 scale-2 objects on a 4 x 2 grid 15 m in front of the camera (codes 0.1 N(0,1),
seeds 100..107), every object one detection of max_pts = 250 rows; a 32-object map: those 8 moved to
the world by t_world_cam plus 24 more on the same grid 6, 12 and 18 m further back.  Both sides are
warmed up, then timed in alternation, --reps rounds; the figures are medians of a host clock around
calls that end in a device synchronise.  No pass/fail threshold: the tool reports what it measures.

Usage (GPU box): python tools/assoc_bench.py [--reps 15] [--out profiles/assoc_frame.json]
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
a = ap.parse_args()

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.abspath(os.path.join(REPO, "dsp-slam-rgbd_amd")))
import synthetic as S  # noqa: E402
from deep_sdf.workspace import decoder_from_state  # noqa: E402
from reconstruct import utils as U  # noqa: E402
from reconstruct.optimizer import SceneSdf, SdfRenderer  # noqa: E402

W, H, N_DET, N_OBJ, MAX_PTS = 640, 480, 8, 32, 250
CAM = dict(width=W, height=H, fx=500.0, fy=500.0, cx=319.5, cy=239.5)
TOL, MIN_HITS, MIN_PCT = np.float32(0.05), 20, 50
dec = decoder_from_state(S.make_decoder(1234), S.DEFAULT_SPECS)
cam_objs = []
for i in range(N_OBJ):
    T = S.make_object(7 + i, n_pts=8, scale=2.0, tz=15, perturb=0).t_true.copy()
    T[:3, 3] = (4.6 * (i % 4 - 1.5), 4.6 * ((i // 4) % 2 - 0.5), 15.0 + 6.0 * (i // 8))
    cam_objs.append((T.astype(np.float32), (0.1 * np.random.default_rng(100 + i).standard_normal(64)).astype(np.float32)))
ren = SdfRenderer(dec, W, H, CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"])
img = ren.render(cam_objs[:N_DET])
ren.close()
depth, inst = img["depth"].copy(), img["instance"].copy()
labels = list(range(N_DET))
c, s = np.cos(0.3), np.sin(0.3)
t_world_cam = np.array([[c, 0, s, 2.0], [0, 1, 0, -1.0], [-s, 0, c, 0.5], [0, 0, 0, 1]], np.float64)
twc32 = t_world_cam.astype(np.float32)
objs = [((t_world_cam @ t.astype(np.float64)).astype(np.float32), z) for t, z in cam_objs]
scene = SceneSdf(dec, N_OBJ, N_DET * MAX_PTS)
scene.set_objects(objs)
dets = [dict(label=k, t_cam_obj=np.eye(4, dtype=np.float32)) for k in labels]


def device():
    return scene.associate_frame(depth, inst, labels, CAM, twc32, max_pts=MAX_PTS)


def yardstick():
    rows, recs = U.frame_inputs(depth, inst, dets, CAM, max_pts=MAX_PTS, max_bg=0)     # points only, as the device call
    pts = np.full((N_DET, MAX_PTS, 3), np.nan, np.float32)
    for j, o in enumerate(rows):
        pts[j, :o[1].shape[0]] = o[1] @ twc32[:3, :3].T + twc32[:3, 3]
    scene.query(pts.reshape(-1, 3))
    n_in, n_hit, n_neg = (np.zeros((N_DET, N_OBJ), np.int32) for _ in range(3))
    for i in range(N_OBJ):
        idx, _, f = scene.peek(i)
        d = idx // MAX_PTS
        n_in[:, i] = np.bincount(d, minlength=N_DET)
        n_hit[:, i] = np.bincount(d[np.abs(f) <= TOL], minlength=N_DET)
        n_neg[:, i] = np.bincount(d[f < -TOL], minlength=N_DET)
    best = n_hit.argmax(1)
    n_pts = np.asarray([r.n_pts for r in recs])
    hit = n_hit[np.arange(N_DET), best]
    matched = (hit >= MIN_HITS) & (100 * hit > MIN_PCT * n_pts)
    return dict(n_in=n_in, n_hit=n_hit, n_neg=n_neg, obj=np.where(matched, best, -1))


def med(v):
    return float(np.median(v))


modes = {"device": device, "yardstick": yardstick}
first = {}
for name, fn in modes.items():                     # warm-up (first launches, buffers) + check
    for _ in range(2):
        out = fn()
    first[name] = out
dv, ys = first["device"], first["yardstick"]
# the yardstick transforms with numpy's matmul, not the fused rule: a candidate at a ball's rim may differ
same = {k: bool(np.array_equal(dv[k], ys[k])) for k in ("n_in", "n_hit", "n_neg")}
same["obj"] = [r.obj for r in dv["records"]] == ys["obj"].tolist()
wall = {k: [] for k in modes}
for _ in range(a.reps):
    for name, fn in modes.items():                 # alternating order
        t0 = time.perf_counter()
        fn()
        wall[name].append(1e3 * (time.perf_counter() - t0))
device()
st = scene.stats()
res = {"tool": "tools/assoc_bench.py", "frame": [W, H], "detections": N_DET, "max_pts": MAX_PTS, "objects": N_OBJ,
       "reps": a.reps, "rows": [r.n_pts for r in dv["records"]], "matched": [r.obj for r in dv["records"]],
       "decoded": int(st["decoded"]), "n_passes": int(st["n_passes"]), "same_as_yardstick": same}
for name in modes:
    res[name] = {"wall_ms_median": med(wall[name]), "wall_ms_min": float(min(wall[name])),
                 "wall_ms_max": float(max(wall[name]))}
res["unmeasured"] = ["other image sizes", "other detection and object counts", "the host-rows form (associate_points)"]
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(res, fo, indent=1)
        fo.write("\n")
print(json.dumps({"device_ms": res["device"]["wall_ms_median"], "yardstick_ms": res["yardstick"]["wall_ms_median"],
                  "decoded": res["decoded"], "matched": res["matched"], "same_as_yardstick": same}))
