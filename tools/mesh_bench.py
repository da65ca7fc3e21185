"""Mesh extraction: a per-code loop (MeshExtractor.extract_mesh_from_code) against one batch call
(extract_meshes_from_codes), with and without the sign pass (DSR_MESH_LITE=0).

Cases: 1, 8 and 16 codes at 32^3 and 64^3, 4 codes at 128^3; codes 0.1 N(0,1) with fixed seeds on
the suite's synthetic decoder.  Every mode of a case is warmed up, then the modes are timed in
alternation, --reps rounds; the figure is the median.  Wall clock is a host clock around calls that
end in a device synchronise (copies to the host included); the batch call's device-event times
(lite pass, exact passes + mark / merge, marching cubes) come from dsr_mesher_stats.  The per-code
entry point exposes no device events, so its figure is wall clock only.

On a tree without the batch call (--pkg PATH/dsp-slam-rgbd_amd of an older checkout) only the
per-code loop runs; --merge FILE adds that result to this one as its "parent" block.

Usage (GPU box): python tools/mesh_bench.py [--reps 15] [--out profiles/mesh_batch.json]
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
ap.add_argument("--pkg", default=None, help="package directory (dsp-slam-rgbd_amd) to measure")
ap.add_argument("--merge", default=None, help="result file of another tree, stored as 'parent'")
ap.add_argument("--cases", default="1x32,8x32,16x32,1x64,8x64,16x64,4x128")
a = ap.parse_args()

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
PKG = os.path.abspath(a.pkg or os.path.join(REPO, "dsp-slam-rgbd_amd"))
sys.path.insert(0, PKG)
import synthetic as S  # noqa: E402
from deep_sdf.workspace import decoder_from_state  # noqa: E402
from reconstruct.optimizer import MeshExtractor  # noqa: E402

HAS_BATCH = hasattr(MeshExtractor, "extract_meshes_from_codes")
dec = decoder_from_state(S.make_decoder(1234), S.DEFAULT_SPECS)


def med(v):
    return float(np.median(v))


def run_case(n, d):
    mex = MeshExtractor(dec, 64, d)
    codes = [(0.1 * np.random.default_rng(100 + i).standard_normal(64)).astype(np.float32) for i in range(n)]

    def loop():
        return [mex.extract_mesh_from_code(c) for c in codes]

    def batch(sign):
        os.environ["DSR_MESH_LITE"] = "1" if sign else "0"
        try:
            return mex.extract_meshes_from_codes(codes)
        finally:
            del os.environ["DSR_MESH_LITE"]

    modes = {"loop": loop}
    if HAS_BATCH:
        modes["batch_sign"] = lambda: batch(True)
        modes["batch_exact"] = lambda: batch(False)
    ref = None
    for name, fn in modes.items():                     # warm-up (first launches, buffer growth) + check
        for _ in range(2):
            out = fn()
        if ref is None:
            ref = out
        for x, y in zip(ref, out):
            assert x.vertices.tobytes() == y.vertices.tobytes() and x.faces.tobytes() == y.faces.tobytes(), name
    wall = {k: [] for k in modes}
    dev = {k: {"lite_ms": [], "exact_ms": [], "mc_ms": []} for k in modes if k != "loop"}
    st = {}
    reps = max(3, a.reps // 3) if d >= 128 else a.reps
    for _ in range(reps):
        for name, fn in modes.items():                 # alternating order
            t0 = time.perf_counter()
            fn()
            wall[name].append(1e3 * (time.perf_counter() - t0))
            if name != "loop":
                st[name] = mex.stats()
                for k in dev[name]:
                    dev[name][k].append(st[name][k])
    res = {"codes": n, "vol_dim": d, "reps": reps, "vertices": int(sum(m.vertices.shape[0] for m in ref)),
           "faces": int(sum(m.faces.shape[0] for m in ref))}
    for name in modes:
        r = {"wall_ms_median": med(wall[name]), "wall_ms_min": float(min(wall[name])),
             "wall_ms_max": float(max(wall[name]))}
        if name != "loop":
            s = st[name]
            r.update({k: med(v) for k, v in dev[name].items()})
            r["device_ms"] = r["lite_ms"] + r["exact_ms"] + r["mc_ms"]
            r.update({k: s[k] for k in ("n_passes", "slots", "sign_pass", "all_tiles", "exact_tiles", "audit_tiles",
                                        "redo_tiles", "violations", "redone_codes", "lite_broken_blocks")})
            r["max_lite_err"] = s["max_lite_err"]
            r["decoded_tile_share"] = s["exact_tiles"] / s["all_tiles"]
        res[name] = r
    del mex
    return res


out = {"tool": "tools/mesh_bench.py", "has_batch": HAS_BATCH, "package": os.path.relpath(PKG, REPO), "cases": []}
for case in a.cases.split(","):
    n, d = (int(x) for x in case.split("x"))
    r = run_case(n, d)
    out["cases"].append(r)
    line = f"{n:2d} codes at {d}^3: loop {r['loop']['wall_ms_median']:.2f} ms"
    if HAS_BATCH:
        bs, be = r["batch_sign"], r["batch_exact"]
        line += (f" | batch sign {bs['wall_ms_median']:.2f} ms (device {bs['device_ms']:.2f}: lite {bs['lite_ms']:.2f}"
                 f" exact {bs['exact_ms']:.2f} mc {bs['mc_ms']:.2f}; decoded tiles {bs['decoded_tile_share']:.3f})"
                 f" | batch exact {be['wall_ms_median']:.2f} ms (device {be['device_ms']:.2f})")
    print(line, flush=True)
if a.merge:
    out["parent"] = json.load(open(a.merge))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
print(json.dumps({"cases": len(out["cases"]), "has_batch": HAS_BATCH}))
