"""The resident object tracker on the GPU (dsr_tracker_*): Optimizer.track_objects
and track_lidar_frame against Optimizer.estimate_pose_cam_obj_batch (dsr_pose_only_batch, which
stays as it was) — host rows at 5 and 7 pose-only iterations with the iteration-4 inlier filter
dropping some, none and all of an object's points, one handle reused over calls of different
sizes, the argument errors, the asynchronous use, a rendered sweep cropped on the device, and a
LayerNorm and a CodeLength-32 decoder.  Every equality is bitwise on the float32 bits (a NaN pose
is the same NaN on both sides); the one tolerance is the existing golden bound of F7."""
from __future__ import annotations

import numpy as np
import pytest

import lidar_cases as LC
import synthetic as S
from conftest import golden, make_cfg

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 300, 700)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def _opt(dec, iters, code_len=64):
    from reconstruct.optimizer import Optimizer

    optim = dict(S.KITTI_OPTIM, code_len=code_len, pose_only_optim={"num_iterations": iters, "learning_rate": 1.0})
    return Optimizer(dec, make_cfg(optim, "KITTI"))


def _se3(ob):
    T = ob.t_cam_obj.copy()
    s = float(np.cbrt(np.linalg.det(T[:3, :3].astype(np.float64))))
    T[:3, :3] /= s
    return T, s


def _sized(n, code_len=64):
    """A synthetic object's first n points at its perturbed pose, code 0 (the decoder's sphere)."""
    ob = S.kitti_object(40 + n % 37, n_pts=max(n, 1))
    T, s = _se3(ob)
    return (T, s, ob.pts[:n].copy(), np.zeros(code_len, np.float32))


def _cases():
    """[F7 golden, the SIZES objects, 40 of 300 points 0.3 object units off the surface, the all-3.0
    code that leaves no inlier]; the indices of the last two."""
    f = golden("f7_secondary.npz")
    cases = [(f["t_se3"], float(f["scale"]), f["pts"], f["code"])]
    cases += [_sized(n) for n in SIZES]
    ob = S.kitti_object(12, n_pts=300)
    T, s = _se3(ob)
    pts = ob.pts.copy()
    c = ob.t_true[:3, 3]
    r = pts[:40] - c
    pts[:40] += (0.3 * s) * r / np.linalg.norm(r, axis=1, keepdims=True)
    cases.append((T, s, pts, np.zeros(64, np.float32)))
    ob = S.kitti_object(11)
    T, s = _se3(ob)
    cases.append((T, s, ob.pts[:300].copy(), np.full(64, 3.0, np.float32)))
    return cases, len(cases) - 2, len(cases) - 1


@pytest.fixture(scope="module")
def reference(gpu_decoder):
    """iters -> (cases, estimate_pose_cam_obj_batch(cases)): computed once, never changed."""
    cases, _, _ = _cases()
    return {it: (cases, _opt(gpu_decoder, it).estimate_pose_cam_obj_batch(cases)) for it in (5, 7)}


# ------------------------------------------------------------------ 1. host rows against the yardstick
@pytest.mark.parametrize("iters", [5, 7])
def test_host_rows_equal_pose_only_batch(gpu_decoder, reference, iters):
    from reconstruct import _libdsr as L

    cases, ref = reference[iters]
    _, i_out, i_none = _cases()
    poses, recs = _opt(gpu_decoder, iters).track_objects(cases)
    print("records", [(r.status, r.n_pts, r.n_inliers) for r in recs])
    assert same(poses, ref)
    assert [r.n_pts for r in recs] == [c[2].shape[0] for c in cases]
    assert all(r.n_near == 0 and r.n_crop == 0 for r in recs)
    empty = 1 + SIZES.index(0)
    assert recs[empty].status == L.TRACK_NO_POINTS and np.isnan(poses[empty]).all()
    if iters == 5:
        assert all(r.n_inliers == r.n_pts for r in recs)
        assert all(r.status == (L.TRACK_OK if r.n_pts else L.TRACK_NO_POINTS) for r in recs)
        f = golden("f7_secondary.npz")
        assert np.abs(poses[0] - f["pose_only_out"]).max() <= 2e-5 * np.abs(f["pose_only_out"]).max()
    else:
        assert 0 < recs[i_out].n_inliers < recs[i_out].n_pts and recs[i_out].status == L.TRACK_OK
        assert any(r.n_inliers == r.n_pts > 0 for r in recs)
        assert recs[i_none].status == L.TRACK_NO_INLIERS and recs[i_none].n_inliers == 0
        assert np.isnan(poses[i_none]).all() and np.isnan(ref[i_none]).all()
        assert sum(r.status == L.TRACK_NO_POINTS for r in recs) == 1


# ------------------------------------------------------------------ 2. handle reuse and argument errors
def test_one_handle_over_calls_of_different_sizes(gpu_decoder, reference):
    from reconstruct.tracker import ObjectTracker

    cases, _ = reference[7]
    opt = _opt(gpu_decoder, 7)
    ob = S.kitti_object(13, n_pts=700)
    other = _se3(ob) + (ob.pts.copy(), np.zeros(64, np.float32))
    none = (cases[-1][0], cases[-1][1], S.kitti_object(11).pts[:700].copy(), cases[-1][3])
    full = [cases[7], none, other]             # max_obj x max_pts exactly; the middle object loses every point
    calls = [[cases[7], cases[6], cases[-2]], [cases[2], cases[3]], [cases[-1], cases[7], cases[6]], full]
    tr = ObjectTracker(opt, 3, 700)
    try:
        for k, call in enumerate(calls):
            tr.track(call)
            got = tr.result()
            fresh = ObjectTracker(opt, tr.max_obj, tr.max_pts)
            fresh.track(call)
            want = fresh.result()
            fresh.close()
            assert same(got[0], want[0]) and got[1] == want[1], k
            assert same(got[0], opt.estimate_pose_cam_obj_batch(call)), k
    finally:
        tr.close()


def test_argument_errors_leave_the_handle_usable(gpu_decoder, reference):
    import ctypes as C

    from reconstruct import _libdsr as L
    from reconstruct import utils as U
    from reconstruct.tracker import ObjectTracker

    cases, ref = reference[7]
    opt = _opt(gpu_decoder, 7)
    ctx, lib = opt._ctx, opt._ctx.lib
    tr = ObjectTracker(opt, 2, 128)
    good = [cases[2], cases[5]]
    bad_scale = [(cases[2][0], s, cases[2][2], cases[2][3]) for s in (0.0, -1.0, float("nan"), float("inf"))]
    nan_pose = cases[2][0].copy()
    nan_pose[1, 3] = np.nan
    det = dict(trans=(9.0, 1.6, -2.2), size=(3.6, 3.6, 3.96), theta=0.2, code=np.zeros(64, np.float32))
    velo = np.zeros((5, 4), np.float32)
    try:
        with pytest.raises(L.DsrError):
            tr.track([])                                                   # n_obj outside 1 .. max_obj
        with pytest.raises(L.DsrError):
            tr.track([cases[2]] * 3)
        with pytest.raises(L.DsrError):
            tr.track([cases[6]])                                           # 300 points > max_pts
        for c in bad_scale:
            with pytest.raises(L.DsrError):
                tr.track([c])
        with pytest.raises(L.DsrError):
            tr.track([(nan_pose, 1.0, cases[2][2], cases[2][3])])
        assert lib.dsr_tracker_track(tr._handle(), 1, None) == -2          # null arguments
        assert lib.dsr_tracker_track(None, 1, None) == -2
        ins = (L.PoseIn * 1)()
        ins[0].scale = 1.0
        ins[0].t_co_se3[:] = np.eye(4, dtype=np.float32).reshape(-1).tolist()
        assert lib.dsr_tracker_track(tr._handle(), 1, ins) == -2           # null code
        assert lib.dsr_tracker_download(tr._handle(), None, None) == -2
        h = C.c_void_p()
        short = L.OptimParams.from_buffer_copy(opt.params)
        short.code_len = 32
        assert lib.dsr_tracker_create(ctx.handle, gpu_decoder.handle, C.byref(short), 2, 128, C.byref(h)) == -2
        assert lib.dsr_tracker_create(ctx.handle, gpu_decoder.handle, C.byref(opt.params), 0, 128, C.byref(h)) == -2
        assert lib.dsr_tracker_create(ctx.handle, gpu_decoder.handle, C.byref(opt.params), 2, 0, C.byref(h)) == -2
        # the sweep call: the ingest's errors for the fields that are read, the scale, the given pose
        for kw, pri in ((dict(max_pts=129), 1.0), (dict(max_pts=0), 1.0), (dict(radius=0.0), 1.0),
                        (dict(box_margin=float("inf")), 1.0), ({}, 0.0), ({}, float("nan")), ({}, (1.0, nan_pose))):
            with pytest.raises(L.DsrError):
                tr.track_lidar(velo, LC.TCV, [det], [pri], dict(dict(max_pts=64), **kw))
        with pytest.raises(L.DsrError):
            tr.track_lidar(velo, LC.TCV * 2.0, [det], [1.0], dict(max_pts=64))          # not rigid
        with pytest.raises(L.DsrError):
            tr.track_lidar(velo, LC.TCV, [dict(det, size=(3.6, -1.0, 3.96))], [1.0], dict(max_pts=64))
        with pytest.raises(L.DsrError):
            tr.track_lidar(velo, LC.TCV, [dict(det, code=None)], [1.0], dict(max_pts=64))   # null code
        with pytest.raises(L.DsrError):
            tr.track_lidar(velo, LC.TCV, [det] * 3, [1.0] * 3, dict(max_pts=64))
        with pytest.raises(L.DsrError):
            tr.track_lidar(velo, LC.TCV, [], [], dict(max_pts=64))                      # n_det outside 1 .. max_obj
        ld, keep = U.lidar_dets([det])
        pri = (L.TrackDet * 1)()
        pri[0].scale = 1.0
        p = U.lidar_params(max_pts=64)
        tcv = np.ascontiguousarray(LC.TCV.reshape(16))
        assert lib.dsr_tracker_track_lidar(tr._handle(), p, L.fptr(tcv), L.fptr(velo), 5, 2, 1, ld, pri) == -2   # stride
        assert lib.dsr_tracker_track_lidar(tr._handle(), p, L.fptr(tcv), None, 5, 4, 1, ld, pri) == -2         # null sweep
        assert lib.dsr_tracker_track_lidar(tr._handle(), p, L.fptr(tcv), L.fptr(velo), 5, 4, 1, ld, None) == -2
        assert lib.dsr_tracker_track_lidar(tr._handle(), None, L.fptr(tcv), L.fptr(velo), 5, 4, 1, ld, pri) == -2
        tr.track(good)
        poses, _ = tr.result()
        assert same(poses, [ref[2], ref[5]])
    finally:
        tr.close()


# ------------------------------------------------------------------ 3. asynchrony
def test_polling_and_back_to_back_calls(gpu_decoder, reference):
    from reconstruct.tracker import ObjectTracker

    cases, ref = reference[7]
    opt = _opt(gpu_decoder, 7)
    tr = ObjectTracker(opt, 4, 704)
    try:
        a, b = [cases[7], cases[8], cases[5]], [cases[4], cases[6], cases[-1], cases[1]]
        tr.track(a)
        polls = 0
        while not tr.query():
            polls += 1
        assert tr.query()
        poses, recs = tr.result()
        assert same(poses, [ref[7], ref[8], ref[5]])
        tr.track(a)                            # two calls, no result() between: the second's results
        tr.track(b)
        poses, recs = tr.result()
        assert len(poses) == 4 and same(poses, [ref[4], ref[6], ref[len(cases) - 1], ref[1]])
        assert [r.n_pts for r in recs] == [c[2].shape[0] for c in b]
    finally:
        tr.close()


# ------------------------------------------------------------------ 4. a sweep
RW, RH = 96, 72
RCAM = dict(width=RW, height=RH, fx=160.0, fy=160.0, cx=47.5, cy=35.5)
SWEEP_PARAMS = dict(max_pts=65)


def _det(i):
    y = (1.6, -1.6)[i]
    return dict(trans=(9.0 + 0.5 * i, y, -2.2), size=(3.6, 3.6, 3.96), theta=(0.2, -0.4)[i])


def _code(i):
    return ((0.0, 0.1)[i] * np.random.default_rng(100 + i).standard_normal(64)).astype(np.float32)


@pytest.fixture(scope="module")
def sweep(gpu_decoder):
    """Two objects rendered at 96 x 72, back-projected and moved into the velodyne frame (as the
    batch sweeps of test_gpu_lidar.py), plus 30 clutter points inside a third box; a fourth box
    holds nothing.  (sweep, detections with the map objects' codes)."""
    from reconstruct.optimizer import SdfRenderer

    truth = [_det(i) for i in range(2)]
    t_cam_obj = [np.asarray(LC.run("host", np.zeros((0, 3), np.float32), LC.blank(RCAM), [], [d], RCAM, LC.TCV,
                                   dict(max_pts=256))[4][0].t_cam_obj, np.float32).reshape(4, 4) for d in truth]
    ren = SdfRenderer(gpu_decoder, RW, RH, RCAM["fx"], RCAM["fy"], RCAM["cx"], RCAM["cy"])
    img = ren.render([(t_cam_obj[i], _code(i)) for i in range(2)])
    ren.close()
    depth, inst = img["depth"], img["instance"]
    v, u = np.nonzero((inst >= 0) & (depth > 0))
    z = depth[v, u].astype(np.float64)
    cam_pts = np.stack([(u - RCAM["cx"]) / RCAM["fx"] * z, (v - RCAM["cy"]) / RCAM["fy"] * z, z, np.ones_like(z)], 1)
    velo = (cam_pts @ np.linalg.inv(LC.TCV.astype(np.float64)).T)[:, :4].astype(np.float32)
    assert 1000 < velo.shape[0] < 7000
    sparse = LC.det(16.0, 6.0, theta=1.1)
    clutter = np.concatenate([LC.box_points(sparse, 30, np.random.default_rng(1)), np.ones((30, 1), np.float32)], 1)
    velo = np.ascontiguousarray(np.concatenate([velo, clutter], 0))
    dets = [dict(_det(0), trans=(9.05, 1.625, -2.2), code=_code(0)), dict(_det(1), trans=(9.55, -1.575, -2.2), code=_code(1)),
            dict(LC.det(20.0, -9.0, theta=-2.0), code=_code(0)), dict(sparse, code=_code(1))]
    return velo, dets


@pytest.mark.parametrize("iters", [5, 7])
def test_sweep_equals_pose_only_batch_on_the_ingest_rows(gpu_decoder, sweep, iters):
    from reconstruct import _libdsr as L
    from reconstruct import utils as U

    velo, dets = sweep
    opt = _opt(gpu_decoder, iters)
    t_se3, det_scale = U.lidar_track_prep(dets, LC.TCV)
    given = t_se3[1].copy()
    given[:3, 3] += np.float32(0.02)
    scales = [float(det_scale[0]), 1.05 * float(det_scale[1]), 1.7, float(det_scale[3])]
    priors = [scales[0], (scales[1], given), scales[2], scales[3]]
    start = [t_se3[0], given, t_se3[2], t_se3[3]]
    # the rows dsr_lidar_inputs copies back (the image plays no part in them)
    rc, pts, _, _, irecs = LC.run("device", velo, LC.blank(RCAM), [], dets, RCAM, LC.TCV, dict(SWEEP_PARAMS, max_bg=0),
                                  ctx=gpu_decoder.ctx)
    assert rc == 0
    ref = opt.estimate_pose_cam_obj_batch([(start[i], scales[i], pts[i, :irecs[i].n_pts], dets[i]["code"])
                                           for i in range(4)])
    poses, recs = opt.track_lidar_frame(velo, LC.TCV, dets, priors, **SWEEP_PARAMS)
    print("ingest", [(r.n_near, r.n_crop, r.n_pts) for r in irecs], "track", [(r.status, r.n_inliers) for r in recs])
    assert [(r.n_near, r.n_crop, r.n_pts) for r in recs] == [(r.n_near, r.n_crop, r.n_pts) for r in irecs]
    assert irecs[0].n_crop > 65 and irecs[1].n_crop > 65 and irecs[2].n_crop == 0 and 0 < irecs[3].n_crop < 65
    assert [r.n_pts for r in irecs] == [65, 65, 0, irecs[3].n_crop]
    assert same(poses, ref)
    assert recs[2].status == L.TRACK_NO_POINTS and np.isnan(poses[2]).all()
    assert np.isfinite(poses[0]).all() and np.isfinite(poses[1]).all()
    if iters == 5:
        assert all(r.n_inliers == r.n_pts for r in recs)


# ------------------------------------------------------------------ 5. decoder variants
@pytest.mark.parametrize("variant", ["ln", "code32"])
def test_decoder_variants(variant):
    """A LayerNorm decoder (the Jacobian kernel's lnw workspace) and a CodeLength-32 decoder (the
    code padded to the kernels' 64) through the 64-, 65- and 300-point cases at 7 iterations."""
    from deep_sdf.workspace import decoder_from_state
    from test_oracle_golden import _variant_specs

    specs = _variant_specs("ln") if variant == "ln" else dict(S.DEFAULT_SPECS, CodeLength=32)
    code_len = 32 if variant == "code32" else 64
    dec = decoder_from_state(S.make_decoder(1234, specs), specs)
    opt = _opt(dec, 7, code_len)
    rng = np.random.default_rng(8)
    cases = []
    for n in (64, 65, 300):
        T, s, pts, _ = _sized(n)
        cases.append((T, s, pts, (0.05 * rng.standard_normal(code_len)).astype(np.float32)))
    ref = opt.estimate_pose_cam_obj_batch(cases)
    poses, recs = opt.track_objects(cases)
    assert same(poses, ref)
    assert [r.n_pts for r in recs] == [64, 65, 300]
