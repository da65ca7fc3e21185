"""Signature of one batch run and of every decoder-query entry point, for bitwise A/B of two
library builds.

Usage (GPU box): DSR_LIB=<path to libdsr.so> python tools/batch_sig.py out.npz
                 python tools/batch_sig.py --compare a.npz b.npz
A layout-only change (LDS swizzles, schedules) or a host-side refactor must leave every array
bitwise equal.  The batch arrays (rec, cnt) and the 5000-point query (y, j) are signed on the
default decoder, and so are the two other creation paths at their smallest shapes, 2 iterations each:
  cap_1 / cap_2   a 2-slot capacity batch (dsr_batch_create_capacity: 70 points, 270 rays per slot)
                  refilled with one object and run, then with two and run again
  tied            dsr_reconstruct_views, 2 objects x 2 views at 70 points (a tied batch)
The small queries below run on it ("def") and on a LayerNorm decoder ("ln", the Jacobian kernel's
workspace path), at the smallest shapes that take every host path:
  sdf / jac     dsr_sdf_eval with the Jacobian, 70 points (two 64-point tiles, one partial)
  pose          dsr_pose_only_batch, 2 objects x 70 points, 6 iterations (the iteration-4 filter)
  mesh1_* / meshb_*   dsr_mesher_run / dsr_mesher_run_batch, 8^3 grid, 2 codes
  depth / inst / nrm / robj   dsr_renderer_render, 2 objects, 32x24, normals
  dist / obj / grad / sobj    dsr_scene_query, 2 objects x 200 points, gradient
  info          dsr_decoder_info without probe_ms
"""
import copy
import ctypes as C
import os
import sys

import numpy as np

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(REPO, "dsp-slam-rgbd_amd"))
sys.path.insert(0, REPO)

if sys.argv[1] == "--compare":
    a, b = np.load(sys.argv[2]), np.load(sys.argv[3])
    bad = [k for k in a.files if not np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8))]
    bad += [k for k in b.files if k not in a.files]
    print("bitwise equal" if not bad else f"DIFFERS: {bad}")
    sys.exit(1 if bad else 0)

import synthetic as S  # noqa: E402
from deep_sdf.workspace import decoder_from_state  # noqa: E402
from reconstruct import _libdsr as L  # noqa: E402

# an A/B against an older build (ABI 10: this script uses only entry points and record layouts
# both ABIs share) — accept the library's own ABI number
L.ABI_VERSION = C.CDLL(L.lib_path()).dsr_abi_version()
from reconstruct.optimizer import MeshExtractor, Optimizer, SceneSdf, SdfRenderer, sdf_eval  # noqa: E402
from reconstruct.utils import ForceKeyErrorDict  # noqa: E402
import bench  # noqa: E402

dec = decoder_from_state(S.make_decoder(1234), S.DEFAULT_SPECS)
lib, ctx = dec.ctx.lib, dec.ctx
n = 16
batch, keep = bench.make_batch(dec, L.optim_params(S.KITTI_OPTIM), n, 1000)
outs = (L.ObjectOut * n)()
ctx.check(lib.dsr_batch_run(batch), "run")
ctx.check(lib.dsr_batch_download(batch, outs), "dl")
st = L.Stats()
ctx.check(lib.dsr_batch_stats(batch, C.byref(st)), "stats")


def records(outs):
    return np.array([list(o.t_cam_obj) + list(o.code) + [o.loss, o.is_good, o.iters_done] for o in outs], np.float32)


rec = records(outs)
cnt = np.array([st.fwd_points, st.refine_points, st.jac_points], np.int64)
rng = np.random.default_rng(0)
z = (0.3 * rng.standard_normal(64)).astype(np.float32)
x = rng.uniform(-0.9, 0.9, (5000, 3)).astype(np.float32)
y, j = sdf_eval(dec, z, x, with_jac=True)
sig = dict(rec=rec, cnt=cnt, y=y, j=j)


def creation_paths(d):
    """The capacity and the tied creation path on decoder ``d``: {name: out-records}."""
    optim = dict(S.KITTI_OPTIM, joint_optim=dict(S.KITTI_OPTIM["joint_optim"], num_iterations=2))
    opt = Optimizer(d, ForceKeyErrorDict(data_type="KITTI", optimizer=optim))
    objs = [S.kitti_object(30 + i, n_pts=70) for i in range(2)]       # 70 points, 70 + 200 rays
    keep = []
    ins = (L.ObjectIn * 2)()
    for i, ob in enumerate(objs):
        ins[i] = opt._object_in(ob.t_cam_obj, ob.pts, ob.rays, ob.depth, None, keep)
    out = {}
    h = C.c_void_p()
    ctx.check(lib.dsr_batch_create_capacity(ctx.handle, d.handle, C.byref(opt.params), 2, 70, 270, 0, C.byref(h)),
              "create_capacity")
    try:
        for fill in (1, 2):
            o = (L.ObjectOut * fill)()
            ctx.check(lib.dsr_batch_refill(h, fill, ins), "refill")
            ctx.check(lib.dsr_batch_run(h), "run")
            ctx.check(lib.dsr_batch_download(h, o), "dl")
            out["cap_%d" % fill] = records(o)
            assert all(x.is_good and x.iters_done == 2 for x in o), "capacity batch: an object failed early"
    finally:
        lib.dsr_batch_destroy(h)
    views = [S.make_object_views(40 + i, n_views=2, n_pts=70) for i in range(2)]
    res = opt.reconstruct_objects_views([(v.t_cam_obj, v.views, None) for v in views])
    assert all(r["is_good"] and r["fail_view"] == -1 and r["iters_done"] == 2 for r in res), "tied batch: a view failed"
    zero = np.zeros(16, np.float32)                  # (a failed object's result has no pose and no code)
    out["tied"] = np.array([list(zero if r["t_cam_obj"] is None else r["t_cam_obj"].reshape(-1)) +
                            list(np.tile(zero, 4) if r["code"] is None else r["code"]) +
                            [r["loss"], r["is_good"], r["iters_done"], r["fail_view"]] for r in res], np.float32)
    return out


sig.update(creation_paths(dec))


def pose(tx, tz, s=1.0):
    t = np.eye(4, dtype=np.float32)
    t[:3, :3] *= s
    t[0, 3], t[2, 3] = tx, tz
    return t


def queries(d, tag):
    """The converted entry points on decoder ``d``: {name_tag: array}."""
    r = np.random.default_rng(7)
    codes = [(0.1 * r.standard_normal(64)).astype(np.float32) for _ in range(2)]
    out = {}
    out["sdf"], out["jac"] = sdf_eval(d, codes[0], r.uniform(-0.9, 0.9, (70, 3)).astype(np.float32), with_jac=True)
    opt = Optimizer(d, ForceKeyErrorDict(data_type="KITTI", optimizer=dict(
        S.KITTI_OPTIM, pose_only_optim={"num_iterations": 6, "learning_rate": 1.0})))
    cases = []
    for i in range(2):
        ob = S.kitti_object(20 + i, n_pts=70)
        T = ob.t_cam_obj.copy()
        s = float(np.cbrt(np.linalg.det(T[:3, :3].astype(np.float64))))
        T[:3, :3] /= s
        cases.append((T, s, ob.pts, codes[i]))
    out["pose"] = np.stack(opt.estimate_pose_cam_obj_batch(cases))
    mesher = MeshExtractor(d, voxels_dim=8)
    singles = [mesher.extract_mesh_from_code(c) for c in codes]
    for k, m in enumerate(singles + mesher.extract_meshes_from_codes(codes)):
        name = ("mesh1_%d" % k) if k < 2 else ("meshb_%d" % (k - 2))
        out[name + "_v"], out[name + "_f"] = m.vertices, m.faces
    objs = [(pose(-0.5, 3.0), codes[0]), (pose(0.5, 3.5, 1.2), codes[1])]
    rnd = SdfRenderer(d, 32, 24, 30.0, 30.0, 16.0, 12.0)
    img = rnd.render(objs, normals=True)
    out["depth"], out["inst"], out["nrm"] = img.depth, img.instance, img.normals
    out["robj"] = np.array([[o.status, *o.rect, o.n_rays, o.n_ball, o.n_hit, o.n_unconverged, o.n_visible]
                            for o in img.objects], np.int64)
    rnd.close()
    scene = SceneSdf(d, 2, 200)
    scene.set_objects([(pose(0.0, 0.0), codes[0]), (pose(0.8, 0.0, 1.2), codes[1])])
    q = scene.query(r.uniform(-1.0, 1.8, (200, 3)).astype(np.float32) * np.float32([1, 0.6, 0.6]), grad=True)
    out["dist"], out["obj"], out["grad"] = q.dist, q.obj, q.grad
    out["sobj"] = np.array([[o.n_in, o.n_win, o.n_neg, o.n_nan, o.sum_sdf, o.sum_abs] for o in q.objects], np.float64)
    scene.close()
    out["info"] = np.array([float(v) for k, v in sorted(d.info.items()) if k != "probe_ms"], np.float64)
    return {k + "_" + tag: np.ascontiguousarray(v) for k, v in out.items()}


ln_specs = copy.deepcopy(S.DEFAULT_SPECS)
ln_specs["NetworkSpecs"]["weight_norm"] = False          # norm_layers [0..7]: LayerNorm after lin0..lin7
sig.update(queries(dec, "def"))
sig.update(queries(decoder_from_state(S.make_decoder(1234, ln_specs), ln_specs), "ln"))
np.savez(sys.argv[1], **sig)
print("saved", sys.argv[1], "loss[0]", rec[0, 80], "pts", cnt, "arrays", len(sig))
