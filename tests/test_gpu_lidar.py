"""LiDAR keyframe ingest on the GPU: the device kernels (dsr_lidar_inputs) against
the host rule (dsr_lidar_inputs_host) bitwise on every synthetic case and on the golden frame's
inputs, a capacity batch refilled from a sweep (dsr_batch_refill_lidar) against the same batch
refilled from the host arrays, eager and as a replayed hipGraph, and
Optimizer.reconstruct_lidar_frame against reconstruct_keyframe(lidar_inputs).  The sweeps of the
batch tests are SdfRenderer images at 96 x 72 back-projected into the velodyne frame: the renderer
produces what a LiDAR would see of the objects.  Every comparison is bitwise."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import lidar_cases as LC
import synthetic as S
from conftest import make_cfg

pytestmark = pytest.mark.gpu

RW, RH = 96, 72
RCAM = dict(width=RW, height=RH, fx=160.0, fy=160.0, cx=47.5, cy=35.5)
PARAMS = dict(max_pts=256, max_bg=200, min_mask_area=50)
MASKS = [(0, None), (1, None)]


@pytest.fixture(scope="module")
def cases():
    return LC.cases()


def _opt(dec, iters=2):
    from reconstruct.optimizer import Optimizer

    optim = dict(S.REDWOOD_OPTIM, joint_optim=dict(S.REDWOOD_OPTIM["joint_optim"], num_iterations=iters))
    return Optimizer(dec, make_cfg(optim, "Redwood"))


# ------------------------------------------------------------------ kernels against the host rule
def _both(ctx, c):
    host = LC.run("host", *c)
    dev = LC.run("device", *c, ctx=ctx)
    LC.assert_same(dev, host)
    return host


@pytest.mark.parametrize("name", LC.CASE_NAMES)
def test_device_equals_host_on_the_cpu_fixtures(gpu_decoder, cases, name):
    recs = _both(gpu_decoder.ctx, cases[name])[4]
    if name == "nine":
        assert len(recs) == 9
    if name == "crop1080":
        assert recs[0].n_crop == 1080 and recs[0].n_pts == 250
    if name == "n_velo257":
        assert cases[name][0].shape[0] == 257 and recs[0].n_crop == 40


def test_device_equals_host_on_the_golden_frame(gpu_decoder):
    _, c = LC.golden_inputs()
    recs = _both(gpu_decoder.ctx, c)[4]
    assert [r.status for r in recs] == [0, 0, 4] and [r.n_pts for r in recs] == [250, 250, 161]


def test_device_equals_host_with_every_mask_slot_used(gpu_decoder, cases):
    """256 mask-list entries, the matching ones last: the whole LDS table and the linear search."""
    velo, inst, masks, dets, cam, tcv, params = cases["scene"]
    full = [(1000 + j, None) for j in range(256 - len(masks))] + list(masks)
    recs = _both(gpu_decoder.ctx, (velo, inst, full, dets, cam, tcv, params))[4]
    assert [r.mask for r in recs] == [253, 254, 255] and all(r.status == 0 for r in recs)


# ------------------------------------------------------------------ capacity batches
def _det(i, shift=0.0):
    """Two generous boxes (the widened box holds the whole unit ball of the object) side by side, 9 m ahead."""
    y = (1.6, -1.6)[i]
    return dict(trans=(9.0 + 0.5 * i + shift, y + 0.5 * shift, -2.2), size=(3.6, 3.6, 3.96), theta=(0.2, -0.4)[i], code=None)


def _code(i):
    return ((0.0, 0.1)[i] * np.random.default_rng(100 + i).standard_normal(64)).astype(np.float32)


def _pose_of(det):
    """The rule's t_cam_obj of a detection (the host entry point on an empty sweep)."""
    rec = LC.run("host", np.zeros((0, 3), np.float32), LC.blank(RCAM), [], [det], RCAM, LC.TCV, PARAMS)[4][0]
    return np.asarray(rec.t_cam_obj, np.float32).reshape(4, 4)


@pytest.fixture(scope="module")
def rendered(gpu_decoder):
    """Two rendered keyframes of two objects, each back-projected into a velodyne sweep: the second
    at other poses and with label 1 erased from the image.  The detections handed to the ingest sit
    5 cm beside the rendered poses.  Per keyframe (sweep, instance image, detections, depth image)."""
    from reconstruct.optimizer import SdfRenderer

    ren = SdfRenderer(gpu_decoder, RW, RH, RCAM["fx"], RCAM["fy"], RCAM["cx"], RCAM["cy"])
    inv = np.linalg.inv(LC.TCV.astype(np.float64))
    out = []
    for k, shift in enumerate((0.0, 0.4)):
        truth = [_det(i, shift) for i in range(2)]
        img = ren.render([(_pose_of(truth[i]), _code(i)) for i in range(2)])
        assert all(o["n_visible"] > PARAMS["min_mask_area"] for o in img["objects"])
        depth, inst = img["depth"], img["instance"].copy()
        v, u = np.nonzero((inst >= 0) & (depth > 0))
        z = depth[v, u].astype(np.float64)
        cam_pts = np.stack([(u - RCAM["cx"]) / RCAM["fx"] * z, (v - RCAM["cy"]) / RCAM["fy"] * z, z, np.ones_like(z)], 1)
        velo = np.ascontiguousarray((cam_pts @ inv.T)[:, :4].astype(np.float32))     # stride 4, the last column unread
        assert 1000 < velo.shape[0] < 7000
        if k == 1:
            inst[inst == 1] = -1
        out.append((velo, inst, [_det(i, shift + 0.05) for i in range(2)], depth))
    ren.close()
    return out


@pytest.fixture(scope="module")
def sweeps(rendered):
    """The keyframes of ``rendered`` as (sweep, instance image, detections)."""
    return [r[:3] for r in rendered]


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

    def lidar(self, velo, inst, dets, masks=MASKS, **params):
        """dsr_batch_refill_lidar + run + download + dsr_batch_lidar_info"""
        from reconstruct import _libdsr as L
        from reconstruct import utils as U

        cam = U.frame_camera(RCAM)
        velo, inst, tcv = U.lidar_sweep(velo, inst, cam, LC.TCV)
        ld, keep = U.lidar_dets(dets)
        n = len(dets)
        self.ctx.check(self.lib.dsr_batch_refill_lidar(self.h, cam, U.lidar_params(**params), L.fptr(tcv), L.fptr(velo),
                                                       velo.shape[0], velo.shape[1], L.iptr(inst), len(masks),
                                                       U.lidar_masks(masks), n, ld), "refill_lidar")
        outs = self.run(n)
        recs = (L.LidarDetOut * n)()
        self.ctx.check(self.lib.dsr_batch_lidar_info(self.h, recs), "lidar_info")
        return outs, [U.lidar_record(r) for r in recs]

    def host(self, velo, inst, dets, masks=MASKS, **params):
        """dsr_lidar_inputs_host arrays + dsr_batch_refill + run + download"""
        from reconstruct import _libdsr as L

        rc, pts, rays, dobs, recs = LC.run("host", velo, inst, masks, dets, RCAM, LC.TCV, params)
        assert rc == 0
        n = len(dets)
        ins = (L.ObjectIn * n)()
        for i, r in enumerate(recs):
            ok = r.status == 0
            ins[i].t_cam_obj[:] = list(r.t_cam_obj)
            ins[i].pts, ins[i].n_pts = L.fptr(pts[i]), r.n_pts if ok else 0
            ins[i].rays, ins[i].n_rays = L.fptr(rays[i]), r.n_pts + r.n_bg if ok else 0
            ins[i].depth, ins[i].n_depth = L.fptr(dobs[i]), r.n_pts if ok else 0
        self.ctx.check(self.lib.dsr_batch_refill(self.h, n, ins), "refill")
        return self.run(n), recs


def _bytes(outs):
    return bytes(outs)


def test_lidar_refill_equals_host_refill(gpu_decoder, sweeps):
    velo, inst, dets = sweeps[0]
    b = Batch(_opt(gpu_decoder), 2, 256, 456)
    try:
        lo, lrecs = b.lidar(velo, inst, dets, **PARAMS)
        ho, hrecs = b.host(velo, inst, dets, **PARAMS)
        assert lrecs == hrecs
        assert all(r.status == 0 and r.n_crop > 256 and r.n_pts == 256 and r.n_bg > 20 for r in hrecs), hrecs
        assert [r.mask for r in hrecs] == [0, 1]
        assert _bytes(lo) == _bytes(ho)
        assert all(o.iters_done >= 1 for o in lo)
    finally:
        b.close()


def test_lidar_refills_replay_one_graph(gpu_decoder, sweeps):
    """Two different sweeps in succession through one DSR_BATCH_GRAPH batch: one capture, then
    replays, and the outputs and records of an eager batch."""
    from reconstruct import _libdsr as L

    opt = _opt(gpu_decoder)
    g, e = Batch(opt, 2, 256, 456, L.BATCH_GRAPH), Batch(opt, 2, 256, 456)
    try:
        for k, (velo, inst, dets) in enumerate(sweeps):
            go, grecs = g.lidar(velo, inst, dets, **PARAMS)
            eo, erecs = e.lidar(velo, inst, dets, **PARAMS)
            ho, hrecs = e.host(velo, inst, dets, **PARAMS)
            assert grecs == erecs == hrecs
            assert _bytes(go) == _bytes(eo) == _bytes(ho)
            assert [r.status for r in grecs] == ([0, 0] if k == 0 else [0, 3])
        st = L.Stats()
        opt._ctx.check(opt._ctx.lib.dsr_batch_stats(g.h, C.byref(st)), "stats")
        assert st.graph_captures == 1 and st.graph_replays >= 1, (st.graph_captures, st.graph_replays)
        opt._ctx.check(opt._ctx.lib.dsr_batch_stats(e.h, C.byref(st)), "stats")
        assert st.graph_captures == 0 and st.graph_replays == 0
    finally:
        g.close()
        e.close()


def test_an_erased_mask_fails_like_an_empty_object(gpu_decoder, sweeps):
    """The second sweep's image has lost label 1: detection 1 is NO_MATCH, its rows and pose are
    still recorded, its object fails like an empty one, and its neighbour is what it is alone."""
    from reconstruct import _libdsr as L

    velo, inst, dets = sweeps[1]
    opt = _opt(gpu_decoder)
    b = Batch(opt, 2, 256, 456)
    try:
        one, _ = b.lidar(velo, inst, dets[:1], **PARAMS)
        one = bytes(one[0])
        two, recs = b.lidar(velo, inst, dets, **PARAMS)
        assert [r.status for r in recs] == [0, 3] and recs[1].mask == -1 and recs[1].n_pts == 256 and recs[1].n_bg == 0
        assert recs[1].n_proj > 0 and 2 * recs[1].n_hits <= recs[1].n_proj
        assert bytes(two[0]) == one
        none = np.zeros((0, 3), np.float32)
        start = np.asarray(recs[1].t_cam_obj, np.float32).reshape(4, 4)
        ref = opt.reconstruct_objects([(start, none, none, np.zeros(0, np.float32))])[0]
        assert not two[1].is_good and not ref["is_good"]
        assert np.float32(two[1].loss) == np.float32(ref["loss"]) == 0.0
        assert L.FAIL_REASONS[two[1].fail_reason] == ref["fail_reason"]
    finally:
        b.close()


def test_capacity_errors(gpu_decoder, sweeps):
    from reconstruct import _libdsr as L
    from reconstruct import utils as U

    velo, inst, dets = sweeps[0]
    opt = _opt(gpu_decoder)
    ctx, lib = opt._ctx, opt._ctx.lib
    b = Batch(opt, 2, 256, 456)
    try:
        cam = U.frame_camera(RCAM)
        velo, inst, tcv = U.lidar_sweep(velo, inst, cam, LC.TCV)
        ld, keep = U.lidar_dets(dets + dets[:1])
        ml = U.lidar_masks(MASKS)

        def refill(h=None, n=2, cam=cam, inst=inst, stride=velo.shape[1], tcv=tcv, n_masks=2, **params):
            return lib.dsr_batch_refill_lidar(h or b.h, cam, U.lidar_params(**dict(PARAMS, **params)), L.fptr(tcv),
                                              L.fptr(velo), velo.shape[0], stride, L.iptr(inst), n_masks, ml, n, ld)

        assert refill(max_pts=257) < 0
        assert b"max_pts" in lib.dsr_last_error(ctx.handle)
        assert refill(max_bg=201) < 0
        assert b"max_rays" in lib.dsr_last_error(ctx.handle)
        assert refill(n=3) < 0
        assert b"capacity" in lib.dsr_last_error(ctx.handle)
        assert refill(inst=None) < 0 and refill(stride=2) < 0 and refill(n_masks=257) < 0 and refill(radius=0.0) < 0
        bad = tcv.copy()
        bad[0] *= np.float32(1.5)
        assert refill(tcv=bad) < 0
        assert b"rigid" in lib.dsr_last_error(ctx.handle)
        assert refill(cam=U.frame_camera(dict(RCAM, width=0))) < 0 and refill(max_pts=0) < 0 and refill(downsample=0) < 0
        recs = (L.LidarDetOut * 2)()
        assert lib.dsr_batch_lidar_info(b.h, recs) < 0            # nothing filled yet
        assert refill() == 0
        assert lib.dsr_batch_lidar_info(b.h, recs) == 0 and recs[0].status == 0
        frecs = (L.FrameDetOut * 2)()
        assert lib.dsr_batch_frame_info(b.h, frecs) < 0           # the last fill was a sweep, not a frame
        b.host(velo, inst, dets, **PARAMS)                        # a plain dsr_batch_refill
        assert lib.dsr_batch_lidar_info(b.h, recs) < 0
        assert b"sweep" in lib.dsr_last_error(ctx.handle)
        # an ordinary (non-capacity) batch is refused
        o = S.redwood_object(3, n_pts=64)
        ins = (L.ObjectIn * 1)()
        ins[0] = opt._object_in(o.t_cam_obj, o.pts, o.rays, o.depth, None, keep)
        h = C.c_void_p()
        ctx.check(lib.dsr_batch_create(ctx.handle, gpu_decoder.handle, C.byref(opt.params), 1, ins, C.byref(h)), "create")
        try:
            assert refill(h=h, n=1) < 0
            assert b"capacity" in lib.dsr_last_error(ctx.handle)
        finally:
            lib.dsr_batch_destroy(h)
    finally:
        b.close()


def test_one_batch_takes_every_kind_of_fill(gpu_decoder, rendered):
    """One batch refilled from a frame, a sweep, a frame with poses, host arrays and a frame again:
    after each fill its downloaded out-records and its info records are those of a fresh batch given
    only that fill, and the info calls of the other kinds refuse.  The ingest block of two
    detections in a frame at 96 x 72 takes 2 x 27648 B of images and under 6 KB of tables and
    records (dsr_frame.hpp: frame_dev_bytes + frame_pose_dev_bytes), that of the sweep 16 B per
    point + 27648 B of image + 5120 B of masks + 7 KB of tables (dsr_lidar.hpp: lidar_dev_bytes), so
    above 1400 points the sweep's block is the larger: the second fill grows the block, and the
    third and fifth are laid out in a block left larger than they need."""
    from reconstruct import _libdsr as L
    from reconstruct import utils as U

    (velo, inst, ldets, depth), (_, inst1, _, depth1) = rendered
    assert velo.shape[0] > 1400
    opt = _opt(gpu_decoder)
    ctx, lib = opt._ctx, opt._ctx.lib
    cam = U.frame_camera(RCAM)
    given = [dict(label=i, t_cam_obj=_pose_of(ldets[i]), code=_code(i)) for i in range(2)]
    keep = []

    def frame(b, depth, inst):
        fd, k = U.frame_dets(given)
        keep.append(k)
        ctx.check(lib.dsr_batch_refill_frame(b.h, cam, U.frame_params(**PARAMS), L.fptr(depth), L.iptr(inst), 2, fd),
                  "refill_frame")
        return b.run(2)

    def sweep(b):
        v, i, tcv = U.lidar_sweep(velo, inst, cam, LC.TCV)
        ld, k = U.lidar_dets(ldets)
        keep.append(k)
        ctx.check(lib.dsr_batch_refill_lidar(b.h, cam, U.lidar_params(**PARAMS), L.fptr(tcv), L.fptr(v), v.shape[0],
                                             v.shape[1], L.iptr(i), len(MASKS), U.lidar_masks(MASKS), 2, ld),
                  "refill_lidar")
        return b.run(2)

    def poses(b):
        dets = [given[0], dict(given[1], t_cam_obj=None)]         # one pose given, one from the cuboid
        fd, k = U.frame_dets([U._with_pose(d) for d in dets])
        keep.append(k)
        modes = U.frame_pose_modes(dets)
        ctx.check(lib.dsr_batch_refill_frame_poses(b.h, cam, U.frame_params(**PARAMS), U.frame_pose_params(),
                                                   L.fptr(depth), L.iptr(inst), 2, fd, L.iptr(modes)),
                  "refill_frame_poses")
        return b.run(2)

    def info(b):
        """Per kind the records its info call returns, or None where the call refuses."""
        fr, pr, lr = (L.FrameDetOut * 2)(), (L.FramePoseOut * 2)(), (L.LidarDetOut * 2)()
        f = [U.frame_record(r) for r in fr] if lib.dsr_batch_frame_info(b.h, fr) == 0 else None
        p = ([(r.status, r.n_in, r.n_near, r.n_kept, bytes(r.dims), bytes(r.eig), bytes(r.t_cam_obj)) for r in pr]
             if lib.dsr_batch_frame_pose_info(b.h, pr) == 0 else None)
        s = [U.lidar_record(r) for r in lr] if lib.dsr_batch_lidar_info(b.h, lr) == 0 else None
        return f, p, s

    fills = [("frame", lambda b: frame(b, depth, inst)),
             ("sweep", sweep),
             ("poses", poses),
             ("objects", lambda b: b.host(velo, inst, ldets, **PARAMS)[0]),
             ("frame", lambda b: frame(b, depth1, inst1))]
    answers = dict(frame=(True, False, False), sweep=(False, False, True), poses=(True, True, False),
                   objects=(False, False, False))
    one = Batch(opt, 2, 256, 456)
    try:
        seen = []
        for kind, fill in fills:
            got = (_bytes(fill(one)), info(one))
            fresh = Batch(opt, 2, 256, 456)
            try:
                want = (_bytes(fill(fresh)), info(fresh))
            finally:
                fresh.close()
            assert got == want, kind
            assert tuple(r is not None for r in got[1]) == answers[kind], kind
            seen.append(got)
        assert seen[0][1][0][1].status == 0 and seen[4][1][0][1].status != 0     # label 1: there, then erased
        assert seen[0][0] != seen[4][0]                                          # the two frame fills differ
    finally:
        one.close()


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x["is_good"] == y["is_good"] and np.float32(x["loss"]) == np.float32(y["loss"])
        assert x["iters_done"] == y["iters_done"] and x["fail_reason"] == y["fail_reason"]
        if x["is_good"]:
            assert np.array_equal(x["t_cam_obj"], y["t_cam_obj"]) and np.array_equal(x["code"], y["code"])


def test_reconstruct_lidar_frame_equals_keyframe_of_lidar_inputs(gpu_decoder, sweeps):
    """Optimizer.reconstruct_lidar_frame in slot and graph modes (device ingest) and its oneshot
    fallback (host ingest) against reconstruct_keyframe(utils.lidar_inputs(...)); the third
    detection is behind the camera."""
    from reconstruct import _libdsr as L
    from reconstruct import utils as U

    velo, inst, dets = sweeps[0]
    dets = [dets[0], dict(dets[1], code=_code(1)), dict(dets[0], trans=(-15.0, 0.0, -2.2))]
    objects, records = U.lidar_inputs(velo, inst, MASKS, dets, RCAM, LC.TCV, **PARAMS)
    assert [r.status for r in records] == [0, 0, 1]
    kf = [ob + (True,) for ob in objects]
    results = {}
    for mode in ("slot", "graph", "oneshot"):
        opt = _opt(gpu_decoder)
        opt.keyframe_mode = mode
        got = opt.reconstruct_lidar_frame(velo, inst, MASKS, dets, RCAM, LC.TCV, **PARAMS)
        if mode != "oneshot":                                 # the sweep went through a slot batch
            assert len(opt._slots) == 1
            recs = (L.LidarDetOut * 3)()
            assert opt._ctx.lib.dsr_batch_lidar_info(opt._slots[0].handle, recs) == 0
            assert [r.status for r in recs] == [0, 0, 1]
        else:
            assert opt._slots == []
        ref = opt.reconstruct_keyframe(kf)
        _same(got, ref)
        assert [g["ingest"] for g in got] == records
        assert not got[2]["is_good"]
        results[mode] = got
        opt.close_slots()
    _same(results["slot"], results["oneshot"])
    _same(results["graph"], results["oneshot"])
