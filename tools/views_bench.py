"""Tied against independent: 8 objects x 3 views (KITTI-size views: 2048 points, 2248 rays, 10 GN
iterations) through Optimizer.reconstruct_objects_views on this tree's library, and the same 24
views as 24 independent objects through Optimizer.reconstruct_objects on a build of the parent
commit.  The tied batch does the same per-view work and 8 solves instead of 24, so the two are
expected to be equal within the run-to-run spread.

The legs alternate, each in a fresh child process (one library per process); every leg times
--calls whole calls (batch creation, upload, run, download) after one warm-up and reports their
median; the result is the median over the --reps legs of a kind and their spread (max - min).

Usage (GPU box): python tools/views_bench.py --parent-lib PATH [--reps 4] [--calls 5] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(REPO, "dsp-slam-rgbd_amd"))
sys.path.insert(0, REPO)

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", help="libdsr.so of the parent commit (the independent leg)")
ap.add_argument("--objects", type=int, default=8)
ap.add_argument("--views", type=int, default=3)
ap.add_argument("--reps", type=int, default=4)
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--out")
ap.add_argument("--leg", choices=["views", "independent"], help="(child process) time one leg")
a = ap.parse_args()


def leg():
    import ctypes as C

    import synthetic as S
    from deep_sdf.workspace import decoder_from_state
    from reconstruct import _libdsr as L
    from reconstruct.optimizer import Optimizer
    from reconstruct.utils import ForceKeyErrorDict

    dec = decoder_from_state(S.make_decoder(1234), S.DEFAULT_SPECS)
    opt = Optimizer(dec, ForceKeyErrorDict(data_type="KITTI", optimizer=S.KITTI_OPTIM))
    obs = [S.make_object_views(1000 + i, a.views, n_pts=2048, n_bg=200, scale=2.0, tz=15.0, upright=True)
           for i in range(a.objects)]
    if a.leg == "views":
        objs = [(ob.t_cam_obj, ob.views, None) for ob in obs]
        call = lambda: opt.reconstruct_objects_views(objs)  # noqa: E731
    else:       # every view an object of its own, started from the same pose seen from its camera
        objs = [((np.asarray(t, np.float64) @ ob.t_cam_obj.astype(np.float64)).astype(np.float32), p, r, d, None)
                for ob in obs for (t, p, r, d) in ob.views]
        call = lambda: opt.reconstruct_objects(objs)  # noqa: E731
    res = call()
    ts = []
    for _ in range(a.calls):
        t0 = time.perf_counter()
        res = call()
        ts.append(time.perf_counter() - t0)
    print(json.dumps(dict(leg=a.leg, n=len(objs), good=sum(bool(r["is_good"]) for r in res),
                          median_ms=1e3 * float(np.median(ts)), min_ms=1e3 * min(ts),
                          abi=int(C.CDLL(L.lib_path()).dsr_abi_version()))))


if a.leg:
    leg()
    sys.exit(0)
if not a.parent_lib or not os.path.isfile(a.parent_lib):
    sys.exit("--parent-lib: a libdsr.so built from the parent commit is needed")
runs = {"views": [], "independent": []}
for rep in range(a.reps):
    for kind in ("independent", "views"):
        env = dict(os.environ)
        if kind == "independent":
            env["DSR_LIB"] = os.path.abspath(a.parent_lib)
        else:
            env.pop("DSR_LIB", None)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", kind, "--objects", str(a.objects),
                            "--views", str(a.views), "--calls", str(a.calls)], env=env, capture_output=True,
                           text=True, timeout=170)
        if p.returncode != 0:
            sys.exit(f"{kind} leg failed ({p.returncode}):\n{p.stderr[-2000:]}")
        r = json.loads(p.stdout.strip().splitlines()[-1])
        runs[kind].append(r)
        print(f"rep {rep} {kind}: median {r['median_ms']:.2f} ms, good {r['good']}/{r['n']}", flush=True)
out = dict(objects=a.objects, views=a.views, reps=a.reps, calls=a.calls)
for kind, rs in runs.items():
    m = [r["median_ms"] for r in rs]
    out[kind] = dict(median_ms=float(np.median(m)), spread_ms=max(m) - min(m), legs_ms=m,
                     good=rs[-1]["good"], n=rs[-1]["n"])
print(json.dumps(out))
if a.out:
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
