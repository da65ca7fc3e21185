"""The resident object tracker (dsr_tracker_*) against the one-shot pose-only entry
points on the same build and machine: N tracked objects x 250 points (num_lidar_max) at 5 and 7
pose-only iterations, N = 8 and 32, one 120 k-point sweep with 8 detections, and one 640 x 480
rendered frame of 8 objects.

  loop:     Optimizer.estimate_pose_cam_obj once per object (the reference's call pattern,
            LocalMapping_util.cc:103-110)
  batch:    Optimizer.estimate_pose_cam_obj_batch (dsr_pose_only_batch)
  tracker:  Optimizer.track_objects' two halves on its resident ObjectTracker: call_ms until
            track() returns, done_ms until result() returns
  sweep:    the ingest rows on the device, then the batch (dsr_lidar_inputs, then
            estimate_pose_cam_obj_batch on the rows it copies back) against
            Optimizer.track_lidar_frame
  frame:    a depth image + instance image at 7 iterations, max_pts = 250.  rows_then_track: the
            rows on the host (utils.frame_inputs: a W x H scan per detection), then the resident
            tracker's track() from those rows — what a caller does without the new entry point;
            track_frame: ObjectTracker.track_frame (the rows are built on the device).  call_ms
            until the call returns, done_ms until result() returns the poses.

Host clock; every "done" figure ends in a stream synchronise (the blocking entry points and
result() all do).  All legs are warmed up, then timed in alternation; medians of --reps rounds with
min and max.  The tracker's poses are compared bitwise with the batch's first and the outcome is
reported.  No pass/fail threshold.

Usage (GPU box): python tools/track_bench.py [--reps 15] [--out profiles/track_bench.json]
                 python tools/track_bench.py --legs frame --frame-out profiles/track_frame.json
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--out", default=None)
ap.add_argument("--points", type=int, default=250)
ap.add_argument("--sweep-points", type=int, default=120000)
ap.add_argument("--legs", default="rows,sweep,frame", help="comma-separated: rows, sweep, frame")
ap.add_argument("--frame-out", default=None, help="the frame leg's JSON (profiles/track_frame.json)")
a = ap.parse_args()
LEGS = set(a.legs.split(","))

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.abspath(os.path.join(REPO, "dsp-slam-rgbd_amd")))
import synthetic as S  # noqa: E402
from deep_sdf.workspace import decoder_from_state  # noqa: E402
from reconstruct import _libdsr as L  # noqa: E402
from reconstruct import utils as U  # noqa: E402
from reconstruct.optimizer import Optimizer, SdfRenderer  # noqa: E402

dec = decoder_from_state(S.make_decoder(1234), S.DEFAULT_SPECS)


def optimizer(iters):
    optim = dict(S.KITTI_OPTIM, pose_only_optim={"num_iterations": iters, "learning_rate": 1.0})
    return Optimizer(dec, U.ForceKeyErrorDict(data_type="KITTI", optimizer=optim))


def objects(n):
    out = []
    for i in range(n):
        ob = S.kitti_object(300 + i, n_pts=a.points)
        T = ob.t_cam_obj.copy()
        s = float(np.cbrt(np.linalg.det(T[:3, :3].astype(np.float64))))
        T[:3, :3] /= s
        out.append((T, s, ob.pts, (0.02 * np.random.default_rng(i).standard_normal(64)).astype(np.float32)))
    return out


def bits(x):
    return np.ascontiguousarray(np.asarray(x), np.float32).view(np.uint32)


def stats(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def timed(legs, reps):
    """legs: name -> callable returning a dict of named times (ms); warmed up, then alternating."""
    for fn in legs.values():
        for _ in range(3):
            fn()
    t = {}
    for _ in range(reps):
        for name, fn in legs.items():
            for k, v in fn().items():
                t.setdefault(name, {}).setdefault(k, []).append(v)
    return {name: {k: stats(v) for k, v in d.items()} for name, d in t.items()}


res = {"tool": "tools/track_bench.py", "points": a.points, "reps": a.reps, "rows": []}
for iters in (5, 7) if "rows" in LEGS else ():
    opt = optimizer(iters)
    for n in (8, 32):
        obs = objects(n)
        ref = opt.estimate_pose_cam_obj_batch(obs)
        poses, recs = opt.track_objects(obs)
        tr = opt._tracker

        def loop():
            t0 = time.perf_counter()
            for ob in obs:
                opt.estimate_pose_cam_obj(*ob)
            return {"done_ms": 1e3 * (time.perf_counter() - t0)}

        def batch():
            t0 = time.perf_counter()
            opt.estimate_pose_cam_obj_batch(obs)
            return {"done_ms": 1e3 * (time.perf_counter() - t0)}

        def tracker():
            t0 = time.perf_counter()
            tr.track(obs)
            t1 = time.perf_counter()
            tr.result()
            return {"call_ms": 1e3 * (t1 - t0), "done_ms": 1e3 * (time.perf_counter() - t0)}

        row = {"objects": n, "iterations": iters, "identical_poses": bool(np.array_equal(bits(poses), bits(ref))),
               "n_inliers": [int(r.n_inliers) for r in recs]}
        row.update(timed({"loop": loop, "batch": batch, "tracker": tracker}, a.reps))
        res["rows"].append(row)
        print(json.dumps({k: (v if not isinstance(v, dict) else {q: round(x["median"], 4) for q, x in v.items()})
                          for k, v in row.items() if k != "n_inliers"}), flush=True)

# ---- the sweep leg: tools/lidar_bench.py's scene without its image
N = 8
tcv = np.array([[0, -1, 0, 0.0], [0, 0, -1, -0.08], [1, 0, 0, -0.27], [0, 0, 0, 1]], np.float32)
rng = np.random.default_rng(7)
dets, parts = [], []
for i in range(N):
    row_, col = divmod(i, 4)
    x, y, z = 14.0 + 16.0 * row_ + 0.3 * col, (-7.5, -2.5, 2.5, 7.5)[col] * (1.0 + 0.2 * row_), -1.7 + 3.5 * (row_ % 2)
    w, l, h, th = 1.6 + 0.02 * i, 3.9 + 0.05 * i, 1.5, (0.05, -0.08)[i % 2]
    dets.append(dict(trans=(x, y, z), size=(w, l, h), theta=th,
                     code=(0.02 * np.random.default_rng(100 + i).standard_normal(64)).astype(np.float32)))
    c, s = math.cos(th), math.sin(th)
    R = np.array([[c, 0, -s], [-s, 0, -c], [0, 1, 0]])
    local = rng.uniform(-0.95, 0.95, (max(6000 - 500 * i, 2500), 3)) * np.array([w / 2, h / 2, l / 2])
    parts.append((local @ R.T + np.array([x, y, z + h / 2])).astype(np.float32))
n_fill = max(a.sweep_points - sum(p.shape[0] for p in parts), 0)
r, phi = rng.uniform(3, 60, n_fill), rng.uniform(-math.pi, math.pi, n_fill)
ground = np.stack([r * np.cos(phi), r * np.sin(phi), rng.normal(-1.72, 0.02, n_fill)], 1).astype(np.float32)
xyz = np.concatenate(parts + [ground], 0)
xyz = xyz[rng.permutation(xyz.shape[0])]
velo = np.ascontiguousarray(np.concatenate([xyz, rng.random((xyz.shape[0], 1)).astype(np.float32)], 1))
cam = dict(width=64, height=16, fx=50.0, fy=50.0, cx=31.5, cy=7.5)       # the rows do not depend on the image
inst = np.full((cam["height"], cam["width"]), -1, np.int32)
params = dict(max_pts=a.points)
t_se3, det_scale = U.lidar_track_prep(dets, tcv)
lib = L.load_library()
lcam, lpar = U.frame_camera(cam), U.lidar_params(max_bg=0, **params)
velo_c, inst_c, tcv16 = U.lidar_sweep(velo, inst, lcam, tcv)
ldets, keep_d = U.lidar_dets(dets)
lmasks = U.lidar_masks([])
sweep_rows = []
for iters in (5, 7) if "sweep" in LEGS else ():
    opt = optimizer(iters)
    ctx = opt._ctx
    pts = np.zeros((N, a.points, 3), np.float32)
    rays = np.zeros((N, a.points, 3), np.float32)
    dobs = np.zeros((N, a.points), np.float32)
    out = (L.LidarDetOut * N)()

    def rows_then_batch():
        t0 = time.perf_counter()
        ctx.check(lib.dsr_lidar_inputs(ctx.handle, lcam, lpar, L.fptr(tcv16), L.fptr(velo_c), velo_c.shape[0],
                                       velo_c.shape[1], L.iptr(inst_c), 0, lmasks, N, ldets, L.fptr(pts), L.fptr(rays),
                                       L.fptr(dobs), out), "dsr_lidar_inputs")
        t1 = time.perf_counter()
        poses = opt.estimate_pose_cam_obj_batch([(t_se3[i], float(det_scale[i]), pts[i, :out[i].n_pts], dets[i]["code"])
                                                 for i in range(N)])
        rows_then_batch.poses = poses
        return {"rows_ms": 1e3 * (t1 - t0), "done_ms": 1e3 * (time.perf_counter() - t0)}

    def track_sweep():
        t0 = time.perf_counter()
        poses, recs = opt.track_lidar_frame(velo, tcv, dets, [float(s_) for s_ in det_scale], **params)
        track_sweep.poses, track_sweep.recs = poses, recs
        return {"done_ms": 1e3 * (time.perf_counter() - t0)}

    rows_then_batch()
    track_sweep()
    row = {"objects": N, "iterations": iters, "n_velo": int(velo.shape[0]),
           "identical_poses": bool(np.array_equal(bits(track_sweep.poses), bits(rows_then_batch.poses))),
           "n_pts": [int(r.n_pts) for r in track_sweep.recs], "n_crop": [int(r.n_crop) for r in track_sweep.recs]}
    row.update(timed({"rows_then_batch": rows_then_batch, "track_lidar_frame": track_sweep}, a.reps))
    sweep_rows.append(row)
    print(json.dumps({k: (v if not isinstance(v, dict) else {q: round(x["median"], 4) for q, x in v.items()})
                      for k, v in row.items() if k not in ("n_pts", "n_crop")}), flush=True)
res["sweep"] = sweep_rows


# ---- the frame leg: 8 rendered objects at 640 x 480
def frame_leg():
    FW, FH, iters = 640, 480, 7
    fcam = dict(width=FW, height=FH, fx=525.0, fy=525.0, cx=319.5, cy=239.5)
    fparams = dict(max_pts=a.points)
    codes = [(0.02 * np.random.default_rng(100 + i).standard_normal(64)).astype(np.float32) for i in range(N)]
    sim3, starts, scales = [], [], []
    for i in range(N):
        T = S.make_object(7 + i, n_pts=8, scale=2.0, tz=12, perturb=0).t_true.astype(np.float32)
        T[:3, 3] = ((-4.5, -1.5, 1.5, 4.5)[i % 4], (-1.6, 1.6)[i // 4], 12.0 + 0.25 * i)
        sc = float(np.cbrt(np.linalg.det(T[:3, :3].astype(np.float64))))
        T0 = T.copy()
        T0[:3, :3] /= np.float32(sc)
        T0[:3, 3] += np.float32(0.05)
        sim3.append(T)
        starts.append(T0)
        scales.append(sc)
    ren = SdfRenderer(dec, FW, FH, fcam["fx"], fcam["fy"], fcam["cx"], fcam["cy"])
    img = ren.render([(sim3[i], codes[i]) for i in range(N)])
    ren.close()
    depth, inst = img["depth"], img["instance"]
    opt = optimizer(iters)
    tr = opt._tracker_for(N, a.points)
    host_dets = [dict(label=i, t_cam_obj=starts[i]) for i in range(N)]
    fdets = [dict(label=i, code=codes[i]) for i in range(N)]
    priors = [(scales[i], starts[i]) for i in range(N)]
    got = {}

    def rows_then_track():
        t0 = time.perf_counter()
        objs, _ = U.frame_inputs(depth, inst, host_dets, fcam, **fparams)
        t1 = time.perf_counter()
        tr.track([(starts[i], scales[i], objs[i][1], codes[i]) for i in range(N)])
        t2 = time.perf_counter()
        got["rows"] = tr.result()
        return {"rows_ms": 1e3 * (t1 - t0), "call_ms": 1e3 * (t2 - t0), "done_ms": 1e3 * (time.perf_counter() - t0)}

    def track_frame():
        t0 = time.perf_counter()
        tr.track_frame(depth, inst, fdets, priors, fcam, fparams)
        t1 = time.perf_counter()
        got["frame"] = tr.result()
        return {"call_ms": 1e3 * (t1 - t0), "done_ms": 1e3 * (time.perf_counter() - t0)}

    rows_then_track()
    track_frame()
    recs = got["frame"][1]
    row = {"objects": N, "iterations": iters, "width": FW, "height": FH, "max_pts": a.points,
           "identical_poses": bool(np.array_equal(bits(got["frame"][0]), bits(got["rows"][0]))),
           "n_pts": [int(r.n_pts) for r in recs], "n_valid": [int(r.n_crop) for r in recs],
           "n_inliers": [int(r.n_inliers) for r in recs]}
    row.update(timed({"rows_then_track": rows_then_track, "track_frame": track_frame}, a.reps))
    print(json.dumps({k: (v if not isinstance(v, dict) else {q: round(x["median"], 4) for q, x in v.items()})
                      for k, v in row.items() if k not in ("n_pts", "n_valid", "n_inliers")}), flush=True)
    return row


if "frame" in LEGS:
    res["frame"] = frame_leg()
    if a.frame_out:
        os.makedirs(os.path.dirname(os.path.abspath(a.frame_out)), exist_ok=True)
        with open(a.frame_out, "w") as fo:
            json.dump({"tool": "tools/track_bench.py --legs frame", "reps": a.reps, "frame": res["frame"]}, fo, indent=1)
            fo.write("\n")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(res, fo, indent=1)
        fo.write("\n")
