"""Sphere-traced images (SdfRenderer.render): 640 x 480, 8 synthetic objects, and,
for scale, the meshes of the same 8 codes (MeshExtractor.extract_meshes_from_codes, 64^3) on the
same build.

Objects: the suite's synthetic decoder (seed 1234), codes 0.1 N(0,1) with seeds 100..107, scale-2
poses in two rows of four at depths 11..18 with neighbouring rectangles overlapping; fx = fy = 520.
All three calls are warmed up, then timed in alternation, --reps rounds; the figures are medians.  Wall
clock is a host clock around calls that end in a device synchronise (copies to the host included);
the renderer's device-event times come from dsr_render_stats.  No pass/fail threshold.

Usage (GPU box): python tools/render_bench.py [--reps 15] [--out profiles/render.json]
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
ap.add_argument("--width", type=int, default=640)
ap.add_argument("--height", type=int, default=480)
ap.add_argument("--objects", type=int, default=8)
a = ap.parse_args()

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.abspath(os.path.join(REPO, "dsp-slam-rgbd_amd")))
import synthetic as S  # noqa: E402
from deep_sdf.workspace import decoder_from_state  # noqa: E402
from reconstruct.optimizer import MeshExtractor, SdfRenderer  # noqa: E402

dec = decoder_from_state(S.make_decoder(1234), S.DEFAULT_SPECS)
W, H, N = a.width, a.height, a.objects
f = 520.0 * W / 640.0
ren = SdfRenderer(dec, W, H, f, f, (W - 1) / 2.0, (H - 1) / 2.0)
mex = MeshExtractor(dec, 64, 64)
codes = [(0.1 * np.random.default_rng(100 + i).standard_normal(64)).astype(np.float32) for i in range(N)]
objs = []
for i in range(N):
    T = S.make_object(7 + i, n_pts=8, scale=2, tz=15, perturb=0).t_true.copy()
    col, row = i % 4, (i // 4) % 2
    T[:3, 3] = (-4.5 + 3.0 * col, -2.0 + 4.0 * row, 11.0 + i)
    objs.append((T.astype(np.float32), codes[i]))


def med(v):
    return float(np.median(v))


modes = {"render": lambda: ren.render(objs), "render_normals": lambda: ren.render(objs, normals=True),
         "meshes": lambda: mex.extract_meshes_from_codes(codes)}
first = {}
for name, fn in modes.items():                         # warm-up (first launches, buffer growth) + check
    for _ in range(2):
        out = fn()
    first[name] = out
assert first["render"]["depth"].tobytes() == first["render_normals"]["depth"].tobytes()
wall = {k: [] for k in modes}
dev = {k: {"setup_ms": [], "march_ms": [], "resolve_ms": []} for k in ("render", "render_normals")}
st = {}
for _ in range(a.reps):
    for name, fn in modes.items():                     # alternating order
        t0 = time.perf_counter()
        fn()
        wall[name].append(1e3 * (time.perf_counter() - t0))
        if name in dev:
            st[name] = ren.stats()
            for k in dev[name]:
                dev[name][k].append(st[name][k])

img = first["render"]
res = {"tool": "tools/render_bench.py", "width": W, "height": H, "objects": N, "reps": a.reps,
       "rays": int(sum(o["n_rays"] for o in img["objects"])), "ball": int(sum(o["n_ball"] for o in img["objects"])),
       "hit": int(sum(o["n_hit"] for o in img["objects"])),
       "unconverged": int(sum(o["n_unconverged"] for o in img["objects"])),
       "visible": int((img["instance"] >= 0).sum()),
       "mesh_vertices": int(sum(m.vertices.shape[0] for m in first["meshes"]))}
for name in modes:
    r = {"wall_ms_median": med(wall[name]), "wall_ms_min": float(min(wall[name])), "wall_ms_max": float(max(wall[name]))}
    if name in dev:
        r.update({k: med(v) for k, v in dev[name].items()})
        r.update({k: st[name][k] for k in ("n_passes", "steps_run", "decoded", "max_live_last")})
    res[name] = r
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fo:
        json.dump(res, fo, indent=1)
        fo.write("\n")
print(json.dumps({"ms": res["render"]["wall_ms_median"], "decoded": res["render"]["decoded"],
                  "steps_run": res["render"]["steps_run"], "march_ms": res["render"]["march_ms"],
                  "normals_ms": res["render_normals"]["wall_ms_median"],
                  "meshes_ms": res["meshes"]["wall_ms_median"], "rays": res["rays"], "hit": res["hit"]}))
