"""The resident object tracker's depth-image source on the GPU (dsr_tracker_track_frame; DESIGN.md
§3.5e): Optimizer.track_frame / ObjectTracker.track_frame against the two yardsticks that existed
before it — Optimizer.estimate_pose_cam_obj_batch and Optimizer.track_objects on the rows
utils.frame_inputs (dsr_frame_inputs_host) builds from the same images.  The frame is rendered by
SdfRenderer at 100 x 75: a width that is no multiple of a wave's 64 pixels and a height that is no
multiple of the 4 rows a workgroup takes.  Every equality is bitwise on the float32 bits (a NaN
pose is the same NaN on both sides); there is no tolerance."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import synthetic as S
from conftest import make_cfg

pytestmark = pytest.mark.gpu

RW, RH = 100, 75
RCAM = dict(width=RW, height=RH, fx=165.0, fy=165.0, cx=49.5, cy=37.0)
CROP = dict(RCAM, width=64, height=48)                     # the frame's top-left 64 x 48 pixels
SUB = dict(max_pts=65, min_mask_area=10, far=100.0)        # sub-sampled: two Jacobian tiles, the second of one row
ALL = dict(max_pts=4096, min_mask_area=10, far=100.0)      # every valid pixel
LABELS = (0, 1, 7, 8, 9, 55, 0)                            # 55 is absent; label 0 twice, at two start poses
OBJ = (0, 1, 1, 1, 1, 0, 0)                                # the map object (scale, code, pose) of each detection


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))


def _opt(dec, iters, code_len=64):
    from reconstruct.optimizer import Optimizer

    optim = dict(S.KITTI_OPTIM, code_len=code_len, pose_only_optim={"num_iterations": iters, "learning_rate": 1.0})
    return Optimizer(dec, make_cfg(optim, "KITTI"))


def _codes(code_len=64):
    return [((0.0, 0.1)[i] * np.random.default_rng(100 + i).standard_normal(code_len)).astype(np.float32) for i in range(2)]


def _valid(depth, inst, label, p=SUB):
    return (inst == label) & (depth > 0.01) & (depth < p["far"])


@pytest.fixture(scope="module")
def frame(gpu_decoder):
    """(depth, instance, scales, start poses per detection of LABELS): two rendered objects, then
    label 7 = a 5 x 6 patch of object 1 (30 valid pixels), label 8 = a 3 x 3 patch of it (at most
    min_mask_area pixels), label 9 = a 4 x 4 patch without depth, and 40 pixels of object 0 pushed
    0.3 object scales away along their rays."""
    from reconstruct.optimizer import SdfRenderer

    sim3 = []
    for i, t in enumerate(((-2.6, 0.1, 15.0), (2.6, -0.2, 15.5))):
        T = S.make_object(7 + i, n_pts=8, scale=2.0, tz=15, perturb=0).t_true.copy()
        T[:3, 3] = t
        sim3.append(T.astype(np.float32))
    ren = SdfRenderer(gpu_decoder, RW, RH, RCAM["fx"], RCAM["fy"], RCAM["cx"], RCAM["cy"])
    img = ren.render([(sim3[i], _codes()[i]) for i in range(2)])
    ren.close()
    depth, inst = img["depth"].copy(), img["instance"].copy()
    scales, se3 = [], []
    for T in sim3:
        s = float(np.cbrt(np.linalg.det(T[:3, :3].astype(np.float64))))
        R = T.copy()
        R[:3, :3] /= np.float32(s)
        R[:3, 3] += np.float32(0.05)                        # the fit starts beside the rendered pose
        scales.append(s)
        se3.append(R)
    v1, u1 = np.nonzero(_valid(depth, inst, 1))
    cv, cu = int(np.median(v1)), int(np.median(u1))
    inst[cv:cv + 5, cu:cu + 6] = 7
    inst[cv - 9:cv - 6, cu - 2:cu + 1] = 8
    assert np.all(inst[0:4, 0:4] == -1)
    inst[0:4, 0:4] = 9
    depth[0:4, 0:4] = 0.0
    v0, u0 = np.nonzero(_valid(depth, inst, 0))
    pick = np.linspace(0, v0.shape[0] - 1, 40).astype(np.int64)
    rx, ry = (u0[pick] - RCAM["cx"]) / RCAM["fx"], (v0[pick] - RCAM["cy"]) / RCAM["fy"]
    depth[v0[pick], u0[pick]] += (0.3 * scales[0] / np.sqrt(rx * rx + ry * ry + 1.0)).astype(np.float32)
    # what the tests rely on
    assert _valid(depth, inst, 0).sum() > 65 and _valid(depth, inst, 1).sum() > 65
    assert _valid(depth, inst, 7).sum() == 30 == (inst == 7).sum()
    assert 0 < (inst == 8).sum() <= SUB["min_mask_area"]
    assert (inst == 9).sum() > SUB["min_mask_area"] and _valid(depth, inst, 9).sum() == 0
    assert not (inst == 55).any()
    other = se3[0].copy()
    other[:3, 3] -= np.float32(0.08)
    starts = [se3[o] for o in OBJ[:-1]] + [other]
    return depth, inst, scales, starts


def _call(frame, codes, labels=range(len(LABELS))):
    """(detections, priors) of track_frame for the detections `labels` indexes"""
    _, _, scales, starts = frame
    dets = [dict(label=LABELS[k], code=codes[OBJ[k]]) for k in labels]
    priors = [(scales[OBJ[k]], starts[k]) for k in labels]
    return dets, priors


def _rows(frame, codes, params, labels=range(len(LABELS)), cam=RCAM, window=None):
    """The yardsticks' input: (t_co_se3, scale, pts, code) per detection from the host twin's rows,
    and its records."""
    from reconstruct import utils as U

    depth, inst, scales, starts = frame
    if window:
        depth, inst = depth[window], inst[window]
    host = [dict(label=LABELS[k], t_cam_obj=np.eye(4, dtype=np.float32)) for k in labels]
    objs, recs = U.frame_inputs(depth, inst, host, cam, **params)
    return [(starts[k], scales[OBJ[k]], objs[j][1], codes[OBJ[k]]) for j, k in enumerate(labels)], recs


@pytest.fixture(scope="module")
def reference(gpu_decoder, frame):
    """(iters, max_pts) -> (rows, host records, estimate_pose_cam_obj_batch(rows)): computed once,
    never changed."""
    out = {}
    for iters in (5, 7):
        for p in (SUB, ALL):
            rows, recs = _rows(frame, _codes(), p)
            out[iters, p["max_pts"]] = (rows, recs, _opt(gpu_decoder, iters).estimate_pose_cam_obj_batch(rows))
    return out


def _assert_equals_yardsticks(opt, frame, codes, params, rows, hrecs, ref):
    from reconstruct import _libdsr as L

    depth, inst = frame[0], frame[1]
    dets, priors = _call(frame, codes)
    poses, recs = opt.track_frame(depth, inst, dets, priors, RCAM, **params)
    tposes, trecs = opt.track_objects(rows)
    print("host", [(r.status, r.n_mask, r.n_valid, r.n_pts) for r in hrecs])
    print("track", [(r.status, r.n_pts, r.n_inliers, r.n_near, r.n_crop) for r in recs])
    assert same(poses, ref)
    assert same(poses, tposes)
    key = lambda r: (r.status, r.n_pts, r.n_inliers)  # noqa: E731
    assert [key(r) for r in recs] == [key(r) for r in trecs]
    assert [(r.n_near, r.n_crop) for r in recs] == [(r.n_mask, r.n_valid) for r in hrecs]
    assert [r.n_pts for r in recs] == [r.n_pts for r in hrecs]
    for k in (3, 4, 5):                                     # a small mask, no valid depth, an absent label
        assert recs[k].status == L.TRACK_NO_POINTS and recs[k].n_pts == 0 and np.isnan(poses[k]).all()
    assert [hrecs[k].status for k in (3, 4, 5)] == [L.FRAME_SMALL_MASK, L.FRAME_NO_DEPTH, L.FRAME_NO_MASK]
    assert recs[2].n_pts == 30
    assert recs[0].n_pts == recs[6].n_pts == min(hrecs[0].n_valid, params["max_pts"]) > 64
    assert not same([poses[0]], [poses[6]])                 # one label, two start poses
    return poses, recs


# ------------------------------------------------------------------ 1. equality with the yardsticks
@pytest.mark.parametrize("params", [SUB, ALL], ids=["max_pts65", "max_pts4096"])
@pytest.mark.parametrize("iters", [5, 7])
def test_frame_equals_the_yardsticks_on_the_host_rows(gpu_decoder, frame, reference, iters, params):
    rows, hrecs, ref = reference[iters, params["max_pts"]]
    poses, recs = _assert_equals_yardsticks(_opt(gpu_decoder, iters), frame, _codes(), params, rows, hrecs, ref)
    if params is SUB:
        assert recs[0].n_pts == recs[1].n_pts == 65
    else:
        assert recs[0].n_pts == hrecs[0].n_valid and recs[1].n_pts == hrecs[1].n_valid
    if iters == 5:
        assert all(r.n_inliers == r.n_pts for r in recs)
    elif params is ALL:
        assert 0 < recs[0].n_inliers < recs[0].n_pts
        assert np.isfinite(poses[0]).all()


# ------------------------------------------------------------------ 2. one handle, every source, two image sizes
def test_one_handle_across_sources_and_image_sizes(gpu_decoder, frame, reference):
    from reconstruct.tracker import ObjectTracker

    depth, inst = frame[0], frame[1]
    opt = _opt(gpu_decoder, 7)
    rows = reference[7, 65][0]
    dets, priors = _call(frame, _codes())
    window = (slice(0, CROP["height"]), slice(0, CROP["width"]))
    crop = (np.ascontiguousarray(depth[window]), np.ascontiguousarray(inst[window]))
    assert _valid(crop[0], crop[1], 0).sum() > 65
    full = lambda t: t.track_frame(depth, inst, dets, priors, RCAM, SUB)  # noqa: E731
    small = lambda t: t.track_frame(crop[0], crop[1], dets[:4], priors[:4], CROP, SUB)  # noqa: E731
    host = lambda t: t.track([rows[1], rows[0], rows[2]])  # noqa: E731
    tr = ObjectTracker(opt, 8, 128)
    try:
        for k, call in enumerate((host, full, small, full, host)):
            call(tr)
            got = tr.result()
            fresh = ObjectTracker(opt, 8, 128)
            try:
                call(fresh)
                want = fresh.result()
            finally:
                fresh.close()
            assert same(got[0], want[0]) and got[1] == want[1], k
            if call is full:
                assert same(got[0], reference[7, 65][2]), k
            if call is small:
                srows, _ = _rows(frame, _codes(), SUB, range(4), CROP, window)
                assert same(got[0], opt.estimate_pose_cam_obj_batch(srows)), k
    finally:
        tr.close()


# ------------------------------------------------------------------ 3. argument errors
def test_argument_errors_leave_the_handle_usable(gpu_decoder, frame, reference):
    from reconstruct import _libdsr as L
    from reconstruct import utils as U
    from reconstruct.tracker import ObjectTracker

    depth, inst, scales, starts = frame
    opt = _opt(gpu_decoder, 7)
    lib = opt._ctx.lib
    codes = _codes()
    dets, priors = _call(frame, codes, (0, 1))
    nan_pose = starts[0].copy()
    nan_pose[1, 3] = np.nan
    tr = ObjectTracker(opt, 2, 128)
    try:
        go = lambda d=dets, p=priors, cam=RCAM, **kw: tr.track_frame(depth, inst, d, p, cam, dict(SUB, **kw))  # noqa: E731
        with pytest.raises(L.DsrError):
            go([], [])                                                      # n_det outside 1 .. max_obj
        with pytest.raises(L.DsrError):
            go(dets + dets[:1], priors + priors[:1])
        with pytest.raises(L.DsrError):
            go(max_pts=129)                                                 # above the tracker's
        with pytest.raises(L.DsrError):
            go(max_pts=0)
        for bad in (dict(RCAM, fx=0.0), dict(RCAM, fy=-1.0), dict(RCAM, fx=float("nan"))):
            with pytest.raises(L.DsrError):
                go(cam=bad)
        with pytest.raises(L.DsrError):
            go([dets[0], dict(dets[1], code=None)])                         # null code
        for s in (0.0, -1.0, float("nan"), float("inf")):
            with pytest.raises(L.DsrError):
                go(p=[priors[0], (s, starts[1])])
        with pytest.raises(L.DsrError):
            go(p=[(scales[0], nan_pose), priors[1]])
        with pytest.raises(ValueError):
            go(p=priors[:1])
        with pytest.raises(ValueError):
            go(p=[priors[0], scales[1]])                                    # a prior without a pose
        # raw ctypes: the null pointers, an image size, pose_given == 0
        cam, p = U.frame_camera(RCAM), U.frame_params(**SUB)
        fd = (L.FrameDet * 2)()
        pri = (L.TrackDet * 2)()
        for i in range(2):
            fd[i].label, fd[i].code = i, L.fptr(codes[i])
            pri[i].scale, pri[i].pose_given = scales[i], 1
            pri[i].t_co_se3[:] = starts[i].reshape(-1).tolist()
        good = [tr._handle(), cam, p, L.fptr(depth), L.iptr(inst), 2, fd, pri]
        for k in (0, 1, 2, 3, 4, 6, 7):
            args = list(good)
            args[k] = None
            assert lib.dsr_tracker_track_frame(*args) == -2, k
        for w, h in ((0, RH), (RW, 0), (-RW, RH)):
            assert lib.dsr_tracker_track_frame(*(good[:1] + [L.Camera(w, h, 165.0, 165.0, 49.5, 37.0)] + good[2:])) == -2
        pri[1].pose_given = 0
        assert lib.dsr_tracker_track_frame(*good) == -2
        assert b"pose" in lib.dsr_last_error(opt._ctx.handle)
        pri[1].pose_given = 1
        go()
        poses, _ = tr.result()
        assert lib.dsr_tracker_track_frame(*good) == 0                      # the raw arrays, now complete
        raw, _ = tr.result()
        ref = reference[7, 65][2]
        assert same(poses, ref[:2]) and same(raw, ref[:2])
    finally:
        tr.close()


# ------------------------------------------------------------------ 4. asynchrony
def test_polling_and_back_to_back_calls(gpu_decoder, frame, reference):
    from reconstruct.tracker import ObjectTracker

    depth, inst = frame[0], frame[1]
    ref = reference[7, 65][2]
    codes = _codes()
    tr = ObjectTracker(_opt(gpu_decoder, 7), 8, 128)
    try:
        a, b = _call(frame, codes), _call(frame, codes, (1, 6, 3, 0))
        tr.track_frame(depth, inst, a[0], a[1], RCAM, SUB)
        while not tr.query():
            pass
        assert tr.query()
        assert same(tr.result()[0], ref)
        tr.track_frame(depth, inst, a[0], a[1], RCAM, SUB)   # two calls, no result() between: the second's results
        tr.track_frame(depth, inst, b[0], b[1], RCAM, SUB)
        poses, recs = tr.result()
        assert len(poses) == 4 and same(poses, [ref[1], ref[6], ref[3], ref[0]])
        assert [r.n_pts for r in recs] == [65, 65, 0, 65]
    finally:
        tr.close()


# ------------------------------------------------------------------ 5. a CodeLength-32 decoder
@pytest.mark.parametrize("iters", [5, 7])
def test_code32_decoder(frame, iters):
    """The fixture's images with codes of length 32 (padded to the kernels' 64) through the
    max_pts = 65 case."""
    from deep_sdf.workspace import decoder_from_state

    specs = dict(S.DEFAULT_SPECS, CodeLength=32)
    dec = decoder_from_state(S.make_decoder(1234, specs), specs)
    opt = _opt(dec, iters, 32)
    codes = _codes(32)
    rows, hrecs = _rows(frame, codes, SUB)
    ref = opt.estimate_pose_cam_obj_batch(rows)
    _, recs = _assert_equals_yardsticks(opt, frame, codes, SUB, rows, hrecs, ref)
    if iters == 5:
        assert all(r.n_inliers == r.n_pts for r in recs)
