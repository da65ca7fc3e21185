"""Frame ingest on the GPU: the device kernels (dsr_frame_inputs) against the
host rule (dsr_frame_inputs_host) bitwise, a capacity batch refilled from a frame
(dsr_batch_refill_frame) against the same batch refilled from the host arrays, eager and as a
replayed hipGraph, and Optimizer.reconstruct_frame against reconstruct_keyframe(frame_inputs).
The frames of the batch tests are rendered by SdfRenderer at 96 x 72: the renderer produces what
the ingest consumes.  Every comparison is bitwise."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import frame_cases as FC
import synthetic as S
from conftest import make_cfg

pytestmark = pytest.mark.gpu

RW, RH = 96, 72
RCAM = dict(width=RW, height=RH, fx=160.0, fy=160.0, cx=47.5, cy=35.5)
PARAMS = dict(max_pts=256, max_bg=200, min_mask_area=50)


@pytest.fixture(scope="module")
def cases():
    return FC.cases()


def _opt(dec, iters=2):
    from reconstruct.optimizer import Optimizer

    optim = dict(S.REDWOOD_OPTIM, joint_optim=dict(S.REDWOOD_OPTIM["joint_optim"], num_iterations=iters))
    return Optimizer(dec, make_cfg(optim, "Redwood"))


# ------------------------------------------------------------------ kernels against the host rule
def _both(ctx, depth, inst, cam, dets, params):
    host = FC.run("host", depth, inst, cam, dets, params)
    dev = FC.run("device", depth, inst, cam, dets, params, ctx=ctx)
    FC.assert_same(dev, host)
    return host


CASE_NAMES = ["cap_hit", "cap_not_hit", "n1080", "borders", "boxes", "downsample1", "downsample1_cap", "gh1", "gh0",
              "max_bg0", "dup_label", "absent", "area_eq", "area_plus1", "no_depth", "one_pt", "n_det0", "nine"]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_device_equals_host_on_the_cpu_fixtures(gpu_decoder, cases, name):
    (depth, inst), cam, dets, params = cases[name]
    _, _, _, _, recs = _both(gpu_decoder.ctx, depth, inst, cam, dets, params)
    if name == "nine":
        assert len(recs) == 9
    if name == "n1080":
        assert len(recs) == 1 and recs[0].n_valid == 1080


def _odd_frame(w, h, seed):
    """Two labels in vertical / diagonal bands over a w x h image, with depth holes."""
    rng = np.random.default_rng(seed)
    v, u = np.mgrid[0:h, 0:w]
    inst = np.where((u + 2 * v) % 7 < 3, 1, np.where(u % 5 == 0, 2, -1)).astype(np.int32)
    depth = (1.5 + rng.random((h, w))).astype(np.float32)
    depth[rng.random((h, w)) < 0.1] = 0.0
    depth[rng.random((h, w)) < 0.05] = np.nan
    cam = dict(width=w, height=h, fx=0.9 * w, fy=1.1 * w, cx=0.5 * w - 0.25, cy=0.5 * h + 0.125)
    return depth, inst, cam


@pytest.mark.parametrize("w,h", [(641, 5), (63, 70)])
def test_device_equals_host_on_odd_image_sizes(gpu_decoder, w, h):
    """641 x 5: rows of ten 64-pixel chunks plus one pixel; 63 x 70: rows shorter than a wave,
    more rows than one workgroup's four."""
    depth, inst, cam = _odd_frame(w, h, 3)
    dets = [FC.det(1), FC.det(2), FC.det(1, (3, 1, w - 4, h - 2))]
    for params in (dict(max_pts=100, max_bg=64, min_mask_area=20, downsample=1, expand=2),
                   dict(max_pts=4096, max_bg=4096, min_mask_area=20, downsample=2, expand=0)):
        _, _, _, _, recs = _both(gpu_decoder.ctx, depth, inst, cam, dets, params)
        assert all(r.status == 0 and r.n_pts > 0 and r.n_bg > 0 for r in recs)


def test_device_equals_host_on_a_whole_image_mask(gpu_decoder):
    depth, _, cam = _odd_frame(130, 67, 4)
    inst = np.full((67, 130), 9, np.int32)
    for params in (dict(max_pts=300, min_mask_area=100), dict(max_pts=10000, min_mask_area=100, near=1.7, far=2.2)):
        _, _, _, _, recs = _both(gpu_decoder.ctx, depth, inst, cam, [FC.det(9)], params)
        assert recs[0].n_mask == 130 * 67 and recs[0].box == (0, 0, 129, 66) and recs[0].n_bg == 0
        assert recs[0].n_pts == min(recs[0].n_valid, params["max_pts"]) > 0


# ------------------------------------------------------------------ capacity batches
def _pose(i, t):
    T = S.make_object(7 + i, n_pts=8, scale=2.0, tz=15, perturb=0).t_true.copy()
    T[:3, 3] = t
    return T.astype(np.float32)


def _code(i):
    return ((0.0, 0.1)[i] * np.random.default_rng(100 + i).standard_normal(64)).astype(np.float32)


@pytest.fixture(scope="module")
def frames(gpu_decoder):
    """Two rendered frames of two objects: the second at other poses and with label 1 erased."""
    from reconstruct.optimizer import SdfRenderer

    ren = SdfRenderer(gpu_decoder, RW, RH, RCAM["fx"], RCAM["fy"], RCAM["cx"], RCAM["cy"])
    out = []
    for k, ts in enumerate((((-2.6, 0.1, 15.0), (2.6, -0.2, 15.5)), ((-1.9, 0.6, 14.0), (2.2, -0.5, 16.0)))):
        poses = [_pose(i, t) for i, t in enumerate(ts)]
        img = ren.render([(poses[i], _code(i)) for i in range(2)])
        assert all(o["n_visible"] > PARAMS["min_mask_area"] for o in img["objects"])
        inst = img["instance"].copy()
        if k == 1:
            inst[inst == 1] = -1
        starts = []
        for T in poses:                                       # the fit starts beside the rendered pose
            T0 = T.copy()
            T0[:3, 3] += np.float32(0.05)
            starts.append(T0)
        out.append((img["depth"], inst, starts))
    ren.close()
    return out


def _dets(starts, labels=(0, 1)):
    return [dict(label=lab, t_cam_obj=starts[min(lab, 1)], code=None, bbox=None) for lab in labels]


class Batch:
    def __init__(self, opt, max_obj, max_pts, max_rays, flags=0):
        self.opt, self.ctx, self.lib = opt, opt._ctx, opt._ctx.lib
        self.h = C.c_void_p()
        self.ctx.check(self.lib.dsr_batch_create_capacity(self.ctx.handle, opt.decoder.handle, C.byref(opt.params),
                                                          max_obj, max_pts, max_rays, flags, C.byref(self.h)), "create")

    def close(self):
        self.lib.dsr_batch_destroy(self.h)

    def run(self, n):
        from reconstruct import _libdsr as L

        self.ctx.check(self.lib.dsr_batch_run(self.h), "run")
        outs = (L.ObjectOut * n)()
        self.ctx.check(self.lib.dsr_batch_download(self.h, outs), "download")
        return outs

    def frame(self, depth, inst, dets, cam=RCAM, **params):
        """dsr_batch_refill_frame + run + download + dsr_batch_frame_info"""
        from reconstruct import _libdsr as L
        from reconstruct import utils as U

        fd, keep = U.frame_dets(dets)
        n = len(dets)
        self.ctx.check(self.lib.dsr_batch_refill_frame(self.h, U.frame_camera(cam), U.frame_params(**params),
                                                       L.fptr(depth), L.iptr(inst), n, fd), "refill_frame")
        outs = self.run(n)
        recs = (L.FrameDetOut * n)()
        self.ctx.check(self.lib.dsr_batch_frame_info(self.h, recs), "frame_info")
        return outs, [U.frame_record(r) for r in recs]

    def host(self, depth, inst, dets, cam=RCAM, **params):
        """dsr_frame_inputs_host arrays + dsr_batch_refill + run + download"""
        from reconstruct import _libdsr as L

        rc, pts, rays, dobs, recs = FC.run("host", depth, inst, cam, dets, params)
        assert rc == 0
        n = len(dets)
        ins = (L.ObjectIn * n)()
        for i, (d, r) in enumerate(zip(dets, recs)):
            ins[i].t_cam_obj[:] = np.asarray(d["t_cam_obj"], np.float32).reshape(16).tolist()
            ins[i].pts, ins[i].n_pts = L.fptr(pts[i]), r.n_pts
            ins[i].rays, ins[i].n_rays = L.fptr(rays[i]), r.n_pts + r.n_bg
            ins[i].depth, ins[i].n_depth = L.fptr(dobs[i]), r.n_pts
        self.ctx.check(self.lib.dsr_batch_refill(self.h, n, ins), "refill")
        return self.run(n), recs


def _bytes(outs):
    return bytes(outs)


def test_frame_refill_equals_host_refill(gpu_decoder, frames):
    depth, inst, starts = frames[0]
    b = Batch(_opt(gpu_decoder), 2, 256, 456)
    try:
        dets = _dets(starts)
        fo, frecs = b.frame(depth, inst, dets, **PARAMS)
        ho, hrecs = b.host(depth, inst, dets, **PARAMS)
        assert frecs == hrecs
        assert all(r.status == 0 and r.n_pts > 50 and r.n_bg > 20 for r in hrecs)
        assert _bytes(fo) == _bytes(ho)
        assert all(o.is_good for o in fo) and all(o.iters_done == 2 for o in fo)
    finally:
        b.close()


def test_frame_refills_replay_one_graph(gpu_decoder, frames):
    """Two different frames in succession through one DSR_BATCH_GRAPH batch: one capture, then
    replays, and the records of an eager batch."""
    from reconstruct import _libdsr as L

    opt = _opt(gpu_decoder)
    g, e = Batch(opt, 2, 256, 456, L.BATCH_GRAPH), Batch(opt, 2, 256, 456)
    try:
        for k, (depth, inst, starts) in enumerate(frames):
            dets = _dets(starts)
            go, grecs = g.frame(depth, inst, dets, **PARAMS)
            eo, erecs = e.frame(depth, inst, dets, **PARAMS)
            ho, hrecs = e.host(depth, inst, dets, **PARAMS)
            assert grecs == erecs == hrecs
            assert _bytes(go) == _bytes(eo) == _bytes(ho)
            assert [r.status for r in grecs] == ([0, 0] if k == 0 else [0, 1])
            assert go[0].is_good and bool(go[1].is_good) == (k == 0)
        st = L.Stats()
        opt._ctx.check(opt._ctx.lib.dsr_batch_stats(g.h, C.byref(st)), "stats")
        assert st.graph_captures == 1 and st.graph_replays >= 1, (st.graph_captures, st.graph_replays)
        opt._ctx.check(opt._ctx.lib.dsr_batch_stats(e.h, C.byref(st)), "stats")
        assert st.graph_captures == 0 and st.graph_replays == 0
    finally:
        g.close()
        e.close()


def test_a_missing_label_fails_like_an_empty_object(gpu_decoder, frames):
    depth, inst, starts = frames[0]
    opt = _opt(gpu_decoder)
    b = Batch(opt, 3, 256, 456)
    try:
        two, _ = b.frame(depth, inst, _dets(starts), **PARAMS)
        two = [bytes(o) for o in two]
        three, recs = b.frame(depth, inst, _dets(starts, (0, 5, 1)), **PARAMS)
        assert [r.status for r in recs] == [0, 1, 0] and recs[1].n_pts == recs[1].n_bg == 0
        assert bytes(three[0]) == two[0] and bytes(three[2]) == two[1]
        none = np.zeros((0, 3), np.float32)
        ref = opt.reconstruct_objects([(starts[1], none, none, np.zeros(0, np.float32))])[0]
        assert not three[1].is_good and not ref["is_good"]
        assert np.float32(three[1].loss) == np.float32(ref["loss"]) == 0.0
        from reconstruct import _libdsr as L
        assert L.FAIL_REASONS[three[1].fail_reason] == ref["fail_reason"]
    finally:
        b.close()


def test_capacity_errors(gpu_decoder, frames):
    from reconstruct import _libdsr as L
    from reconstruct import utils as U

    depth, inst, starts = frames[0]
    opt = _opt(gpu_decoder)
    ctx, lib = opt._ctx, opt._ctx.lib
    b = Batch(opt, 2, 256, 456)
    try:
        fd, keep = U.frame_dets(_dets(starts, (0, 1, 0)))
        cam = U.frame_camera(RCAM)

        def refill(n=2, cam=cam, depth=depth, inst=inst, **params):
            return lib.dsr_batch_refill_frame(b.h, cam, U.frame_params(**dict(PARAMS, **params)), L.fptr(depth),
                                              L.iptr(inst), n, fd)

        assert refill(max_pts=257) < 0
        assert b"max_pts" in lib.dsr_last_error(ctx.handle)
        assert refill(max_bg=201) < 0
        assert b"max_rays" in lib.dsr_last_error(ctx.handle)
        assert refill(n=3) < 0
        assert b"capacity" in lib.dsr_last_error(ctx.handle)
        assert refill(depth=None) < 0 and refill(inst=None) < 0
        assert refill(cam=U.frame_camera(dict(RCAM, width=0))) < 0 and refill(cam=U.frame_camera(dict(RCAM, fy=0.0))) < 0
        assert refill(max_pts=0) < 0 and refill(max_bg=-1) < 0 and refill(downsample=0) < 0 and refill(expand=-1) < 0
        recs = (L.FrameDetOut * 2)()
        assert lib.dsr_batch_frame_info(b.h, recs) < 0            # nothing filled yet
        assert refill() == 0
        assert lib.dsr_batch_frame_info(b.h, recs) == 0 and recs[0].status == 0
        b.host(depth, inst, _dets(starts), **PARAMS)              # a plain dsr_batch_refill
        assert lib.dsr_batch_frame_info(b.h, recs) < 0
        assert b"frame" in lib.dsr_last_error(ctx.handle)
        # an ordinary (non-capacity) batch is refused
        o = S.redwood_object(3, n_pts=64)
        ins = (L.ObjectIn * 1)()
        ins[0] = opt._object_in(o.t_cam_obj, o.pts, o.rays, o.depth, None, keep)
        h = C.c_void_p()
        ctx.check(lib.dsr_batch_create(ctx.handle, gpu_decoder.handle, C.byref(opt.params), 1, ins, C.byref(h)), "create")
        try:
            assert lib.dsr_batch_refill_frame(h, cam, U.frame_params(**PARAMS), L.fptr(depth), L.iptr(inst), 1, fd) < 0
            assert b"capacity" in lib.dsr_last_error(ctx.handle)
        finally:
            lib.dsr_batch_destroy(h)
    finally:
        b.close()


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x["is_good"] == y["is_good"] and np.float32(x["loss"]) == np.float32(y["loss"])
        assert x["iters_done"] == y["iters_done"] and x["fail_reason"] == y["fail_reason"]
        if x["is_good"]:
            assert np.array_equal(x["t_cam_obj"], y["t_cam_obj"]) and np.array_equal(x["code"], y["code"])


def test_reconstruct_frame_equals_keyframe_of_frame_inputs(gpu_decoder, frames):
    """Optimizer.reconstruct_frame in slot and graph modes (device ingest) and its oneshot fallback
    (host ingest) against reconstruct_keyframe(utils.frame_inputs(...)); detection 0 is not yet
    reconstructed, so its flipped hypothesis and the loss choice run."""
    from reconstruct import _libdsr as L
    from reconstruct import utils as U

    depth, inst, starts = frames[0]
    dets = [dict(label=0, t_cam_obj=starts[0], reconstructed=False),
            dict(label=1, t_cam_obj=starts[1], code=_code(1), reconstructed=True),
            dict(label=4, t_cam_obj=starts[1], reconstructed=False)]
    objects, records = U.frame_inputs(depth, inst, dets, RCAM, **PARAMS)
    kf = [ob + (d["reconstructed"],) for ob, d in zip(objects, dets)]
    results = {}
    for mode in ("slot", "graph", "oneshot"):
        opt = _opt(gpu_decoder)
        opt.keyframe_mode = mode
        got = opt.reconstruct_frame(depth, inst, dets, RCAM, **PARAMS)
        if mode != "oneshot":                                 # the frame went through a slot batch
            assert len(opt._slots) == 1
            recs = (L.FrameDetOut * 5)()
            assert opt._ctx.lib.dsr_batch_frame_info(opt._slots[0].handle, recs) == 0
            assert [r.status for r in recs] == [0, 0, 0, 1, 1]
        else:
            assert opt._slots == []
        ref = opt.reconstruct_keyframe(kf)
        _same(got, ref)
        assert [g["ingest"] for g in got] == records
        assert [g["is_good"] for g in got] == [True, True, False]
        results[mode] = got
        opt.close_slots()
    _same(results["slot"], results["oneshot"])
    _same(results["graph"], results["oneshot"])
