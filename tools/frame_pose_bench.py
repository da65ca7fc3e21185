"""Cuboid start poses on the device (dsr_batch_refill_frame_poses) against the plain
frame refill and against the host route, on the same build and machine: a 640 x 480 frame of 8
rendered objects (tools/frame_bench.py's scene), max_pts 2048, one capacity batch of 8 slots.

  (a) poses:  dsr_batch_refill_frame_poses(depth, instance, detections, all modes cuboid)
  (b) given:  dsr_batch_refill_frame with given poses — (a) minus (b) is what k_frame_pose and
              k_frame_compact add
  (c) host:   reconstruct.utils.frame_poses (dsr_frame_poses_host) + Optimizer._object_in per object
              + dsr_batch_refill

Per leg and keyframe: call_ms, the host-side time until the refill call returns (leg (c)'s includes
building the arrays and poses); done_ms, a host clock from the start of the refill to the end of a
stream synchronise after it (uploads and kernels finished) — a host-clock window, not a kernel
time; keyframe_ms, refill + run + download of the whole GN run.  All legs are warmed up, then
timed in alternation; medians of --reps rounds.  Legs (a) and (c) are compared first (bitwise
equal records after a run).  No pass/fail threshold.

Usage (GPU box): python tools/frame_pose_bench.py [--reps 15] [--out profiles/frame_pose.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--out", default=None)
ap.add_argument("--width", type=int, default=640)
ap.add_argument("--height", type=int, default=480)
ap.add_argument("--objects", type=int, default=8)
ap.add_argument("--max-pts", type=int, default=2048)
ap.add_argument("--max-bg", type=int, default=200)
ap.add_argument("--radius", type=float, default=2.0, help="outlier_radius: the rendered objects' size")
a = ap.parse_args()

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.abspath(os.path.join(REPO, "dsp-slam-rgbd_amd")))
import synthetic as S  # noqa: E402
from deep_sdf.workspace import decoder_from_state  # noqa: E402
from reconstruct import _libdsr as L  # noqa: E402
from reconstruct import utils as U  # noqa: E402
from reconstruct.optimizer import Optimizer, SdfRenderer  # noqa: E402

dec = decoder_from_state(S.make_decoder(1234), S.DEFAULT_SPECS)
W, H, N = a.width, a.height, a.objects
f = 520.0 * W / 640.0
cam = dict(width=W, height=H, fx=f, fy=f, cx=(W - 1) / 2.0, cy=(H - 1) / 2.0)
ren = SdfRenderer(dec, W, H, f, f, cam["cx"], cam["cy"])
objs = []
for i in range(N):
    T = S.make_object(7 + i, n_pts=8, scale=2, tz=15, perturb=0).t_true.copy()
    col, row = i % 4, (i // 4) % 2
    T[:3, 3] = (-4.5 + 3.0 * col, -2.0 + 4.0 * row, 11.0 + i)
    objs.append((T.astype(np.float32), (0.1 * np.random.default_rng(100 + i).standard_normal(64)).astype(np.float32)))
img = ren.render(objs)
ren.close()
depth, inst = img["depth"], img["instance"]
given = [dict(label=i, t_cam_obj=objs[i][0]) for i in range(N)]
poseless = [dict(label=i, t_cam_obj=None) for i in range(N)]
params = dict(max_pts=a.max_pts, max_bg=a.max_bg)
pose_params = dict(outlier_radius=a.radius)

opt = Optimizer(dec, U.ForceKeyErrorDict(data_type="Redwood", optimizer=S.REDWOOD_OPTIM))
ctx, lib = opt._ctx, opt._ctx.lib
h = C.c_void_p()
ctx.check(lib.dsr_batch_create_capacity(ctx.handle, dec.handle, C.byref(opt.params), N, a.max_pts, a.max_pts + a.max_bg,
                                        0, C.byref(h)), "dsr_batch_create_capacity")
fcam, fpar, fpose = U.frame_camera(cam), U.frame_params(**params), U.frame_pose_params(pose_params)
fgiven, keep_g = U.frame_dets(given)
fposeless, keep_p = U.frame_dets([U._with_pose(d) for d in poseless])
modes = U.frame_pose_modes(poseless)
outs = (L.ObjectOut * N)()


def refill_poses():
    ctx.check(lib.dsr_batch_refill_frame_poses(h, fcam, fpar, fpose, L.fptr(depth), L.iptr(inst), N, fposeless,
                                               L.iptr(modes)), "dsr_batch_refill_frame_poses")


def refill_given():
    ctx.check(lib.dsr_batch_refill_frame(h, fcam, fpar, L.fptr(depth), L.iptr(inst), N, fgiven), "dsr_batch_refill_frame")


def refill_host():
    objects, _, _ = U.frame_poses(depth, inst, poseless, cam, pose_params, **params)
    keep = []
    ins = (L.ObjectIn * N)()
    for i, ob in enumerate(objects):
        ins[i] = opt._object_in(*ob, keep)
    ctx.check(lib.dsr_batch_refill(h, N, ins), "dsr_batch_refill")


def sync():
    ctx.check(lib.dsr_batch_download(h, outs), "dsr_batch_download")


def run():
    ctx.check(lib.dsr_batch_run(h), "dsr_batch_run")
    sync()
    return bytes(outs)


paths = {"poses": refill_poses, "given": refill_given, "host": refill_host}
first = {}
for name, fn in paths.items():                          # warm-up (buffer growth, first launches) + check
    for _ in range(2):
        fn()
        first[name] = run()
assert first["poses"] == first["host"], "the device and host routes gave different reconstructions"
precs = (L.FramePoseOut * N)()
refill_poses()
ctx.check(lib.dsr_batch_frame_pose_info(h, precs), "dsr_batch_frame_pose_info")
t = {k: {"call_ms": [], "done_ms": [], "keyframe_ms": []} for k in paths}
for _ in range(a.reps):
    for name, fn in paths.items():                      # alternating order
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        sync()
        t2 = time.perf_counter()
        t[name]["call_ms"].append(1e3 * (t1 - t0))
        t[name]["done_ms"].append(1e3 * (t2 - t0))
        t0 = time.perf_counter()
        fn()
        run()
        t[name]["keyframe_ms"].append(1e3 * (time.perf_counter() - t0))
lib.dsr_batch_destroy(h)

res = {"tool": "tools/frame_pose_bench.py", "width": W, "height": H, "objects": N, "max_pts": a.max_pts,
       "max_bg": a.max_bg, "outlier_radius": a.radius, "reps": a.reps, "gn_iterations": int(opt.params.num_iterations),
       "status": [int(r.status) for r in precs], "n_in": [int(r.n_in) for r in precs],
       "n_near": [int(r.n_near) for r in precs], "n_kept": [int(r.n_kept) for r in precs],
       "note": "done_ms is a host-clock window ending in a stream synchronise, not a kernel time"}
for name in paths:
    res[name] = {}
    for k, v in t[name].items():
        res[name][k + "_median"] = float(np.median(v))
        res[name][k + "_min"] = float(min(v))
        res[name][k + "_max"] = float(max(v))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(res, fo, indent=1)
        fo.write("\n")
print(json.dumps({p: {k: round(res[p][k + "_median"], 4) for k in ("call_ms", "done_ms", "keyframe_ms")} for p in paths}
                 | {"n_kept": res["n_kept"], "n_in": res["n_in"], "status": res["status"]}))
