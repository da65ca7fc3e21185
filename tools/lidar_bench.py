"""LiDAR keyframe ingest (dsr_batch_refill_lidar) against the host path on the same
build and machine: a 1242 x 375 image, a synthetic sweep of about 120 k points (8 boxes of a few
thousand points each over ground and clutter), 8 detections, max_pts 2048, into one capacity batch
of 8 slots (max_rays 2248).

  device path: dsr_batch_refill_lidar(sweep, instance, masks, detections)
  host path:   reconstruct.utils.lidar_inputs (dsr_lidar_inputs_host) + Optimizer._object_in per
               object + dsr_batch_refill

Per path and keyframe: call_ms, the host-side time until the refill call returns (the host path's
includes building the arrays); done_ms, a host clock from the start of the refill to the end of a
stream synchronise after it (dsr_batch_download of the not-yet-run batch: uploads and kernels
finished), so done_ms - call_ms is the device time the host did not wait for; keyframe_ms, refill +
run + download of the whole GN run.  Both paths are warmed up, then timed in alternation; medians of
--reps rounds.  The two fills are compared first (the object records after a run and the ingest
records) and the outcome is reported.  No pass/fail threshold.

Usage (GPU box): python tools/lidar_bench.py [--reps 15] [--out profiles/lidar_ingest.json]
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--out", default=None)
ap.add_argument("--width", type=int, default=1242)
ap.add_argument("--height", type=int, default=375)
ap.add_argument("--objects", type=int, default=8)
ap.add_argument("--points", type=int, default=120000)
ap.add_argument("--max-pts", type=int, default=2048)
ap.add_argument("--max-bg", type=int, default=200)
a = ap.parse_args()

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.abspath(os.path.join(REPO, "dsp-slam-rgbd_amd")))
import synthetic as S  # noqa: E402
from deep_sdf.workspace import decoder_from_state  # noqa: E402
from reconstruct import _libdsr as L  # noqa: E402
from reconstruct import utils as U  # noqa: E402
from reconstruct.optimizer import Optimizer  # noqa: E402

W, H, N = a.width, a.height, a.objects
cam = dict(width=W, height=H, fx=721.5, fy=721.5, cx=609.5, cy=172.75)
# velodyne (x ahead, y left, z up) -> camera (x right, y down, z ahead), a KITTI-like offset
tcv = np.array([[0, -1, 0, 0.0], [0, 0, -1, -0.08], [1, 0, 0, -0.27], [0, 0, 0, 1]], np.float32)
rng = np.random.default_rng(7)
dets, parts = [], []
# cars seen side-on, none hiding another: rows of four, 14 m ahead on the ground, 30 m ahead on an overpass, ...
for i in range(N):
    row, col = divmod(i, 4)
    x, y, z = 14.0 + 16.0 * row + 0.3 * col, (-7.5, -2.5, 2.5, 7.5)[col] * (1.0 + 0.2 * row), -1.7 + 3.5 * (row % 2)
    w, l, h, th = 1.6 + 0.02 * i, 3.9 + 0.05 * i, 1.5, (0.05, -0.08)[i % 2]
    dets.append(dict(trans=(x, y, z), size=(w, l, h), theta=th,
                     code=(0.1 * np.random.default_rng(100 + i).standard_normal(64)).astype(np.float32)))
    c, s = math.cos(th), math.sin(th)
    R = np.array([[c, 0, -s], [-s, 0, -c], [0, 1, 0]])
    local = rng.uniform(-0.95, 0.95, (max(6000 - 500 * i, 2500), 3)) * np.array([w / 2, h / 2, l / 2])
    parts.append((local @ R.T + np.array([x, y, z + h / 2])).astype(np.float32))
n_fill = max(a.points - sum(p.shape[0] for p in parts), 0)
r, phi = rng.uniform(3, 60, n_fill), rng.uniform(-math.pi, math.pi, n_fill)
ground = np.stack([r * np.cos(phi), r * np.sin(phi), rng.normal(-1.72, 0.02, n_fill)], 1).astype(np.float32)
ground[::7, 2] += rng.uniform(0, 3, ground[::7].shape[0]).astype(np.float32)          # walls, poles, bushes
xyz = np.concatenate(parts + [ground], 0)
xyz = xyz[rng.permutation(xyz.shape[0])]
velo = np.ascontiguousarray(np.concatenate([xyz, rng.random((xyz.shape[0], 1)).astype(np.float32)], 1))   # KITTI's stride 4
inst = np.full((H, W), -1, np.int32)
masks = []
for i in reversed(range(N)):                             # far cars first, nearer ones painted over them
    q = parts[i].astype(np.float64) @ tcv[:3, :3].astype(np.float64).T + tcv[:3, 3]
    u, v = cam["fx"] * q[:, 0] / q[:, 2] + cam["cx"], cam["fy"] * q[:, 1] / q[:, 2] + cam["cy"]
    l, rr = max(int(u.min()) - 2, 0), min(int(u.max()) + 2, W - 1)
    t, b = max(int(v.min()) - 2, 0), min(int(v.max()) + 2, H - 1)
    inst[t:b + 1, l:rr + 1] = 50 + i
    masks.append(dict(label=50 + i, bbox=(l - 3, t - 2, rr + 3, b + 2)))
masks += [dict(label=90 + k) for k in range(4)]          # detections of other things
inst[5:60, 20:200] = np.where(inst[5:60, 20:200] < 0, 90, inst[5:60, 20:200])
params = dict(max_pts=a.max_pts, max_bg=a.max_bg)

dec = decoder_from_state(S.make_decoder(1234), S.DEFAULT_SPECS)
opt = Optimizer(dec, U.ForceKeyErrorDict(data_type="KITTI", optimizer=S.KITTI_OPTIM))
ctx, lib = opt._ctx, opt._ctx.lib
h = C.c_void_p()
ctx.check(lib.dsr_batch_create_capacity(ctx.handle, dec.handle, C.byref(opt.params), N, a.max_pts, a.max_pts + a.max_bg,
                                        0, C.byref(h)), "dsr_batch_create_capacity")
lcam, lpar = U.frame_camera(cam), U.lidar_params(**params)
velo, inst, tcv16 = U.lidar_sweep(velo, inst, lcam, tcv)
ldets, keep_d = U.lidar_dets(dets)
lmasks = U.lidar_masks(masks)
outs = (L.ObjectOut * N)()
host_records = []


def refill_device():
    ctx.check(lib.dsr_batch_refill_lidar(h, lcam, lpar, L.fptr(tcv16), L.fptr(velo), velo.shape[0], velo.shape[1],
                                         L.iptr(inst), len(masks), lmasks, N, ldets), "dsr_batch_refill_lidar")


def refill_host():
    objects, records = U.lidar_inputs(velo, inst, masks, dets, cam, tcv, **params)
    host_records[:] = records
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


paths = {"device": refill_device, "host": refill_host}
first = {}
for name, fn in paths.items():                          # warm-up (buffer growth, first launches) + check
    for _ in range(2):
        fn()
        first[name] = run()
recs = (L.LidarDetOut * N)()
refill_device()
ctx.check(lib.dsr_batch_lidar_info(h, recs), "dsr_batch_lidar_info")
recs = [U.lidar_record(x) for x in recs]
same_objects, same_records = first["device"] == first["host"], recs == host_records
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

res = {"tool": "tools/lidar_bench.py", "width": W, "height": H, "objects": N, "n_velo": int(velo.shape[0]),
       "stride": int(velo.shape[1]), "n_masks": len(masks), "max_pts": a.max_pts, "max_bg": a.max_bg, "reps": a.reps,
       "gn_iterations": int(opt.params.num_iterations), "identical_object_records": bool(same_objects),
       "identical_ingest_records": bool(same_records)}
for k in ("status", "n_near", "n_crop", "n_pts", "n_proj", "mask", "n_hits", "n_mask_px", "n_bg"):
    res[k] = [int(r[k]) for r in recs]
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
                 | {"n_pts": res["n_pts"], "status": res["status"], "identical_object_records": res["identical_object_records"],
                    "identical_ingest_records": res["identical_ingest_records"]}))
