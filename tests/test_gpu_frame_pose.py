"""Cuboid start poses and outlier removal on the GPU: the device kernels
(dsr_frame_poses: k_frame_pose + k_frame_compact after the ingest) against the host twin
(dsr_frame_poses_host) bitwise, a capacity batch refilled by dsr_batch_refill_frame_poses against
the same batch refilled from the host twin's arrays and poses, eager and as a replayed hipGraph,
and Optimizer.reconstruct_frame with pose-less detections against reconstruct_keyframe over
utils.frame_poses.  The frames of the batch tests are rendered by SdfRenderer at 96 x 72."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import frame_pose_cases as PC
import frame_pose_oracle as PO
import test_gpu_frame as TF

pytestmark = pytest.mark.gpu

RCAM, PARAMS = TF.RCAM, TF.PARAMS
# the rendered objects are at the renderer fixture's scale (about 2 units across at z = 15), not at
# the reference's map scale: the radius is their size
POSE = dict(outlier_radius=2.0, box_margin=1.2, min_points=50)
CUB, FLIP, GIVEN = PO.CUBOID, PO.CUBOID_FLIPPED, PO.GIVEN


@pytest.fixture(scope="module")
def cases():
    return PC.cases()


# ------------------------------------------------------------------ kernels against the host twin
def _both(ctx, depth, inst, cam, dets, modes, params, pose_params):
    host = PC.run("host", depth, inst, cam, dets, modes, params, pose_params)
    dev = PC.run("device", depth, inst, cam, dets, modes, params, pose_params, ctx=ctx)
    PC.assert_same(dev, host)
    return host


@pytest.mark.parametrize("name", PC.CASE_NAMES)
def test_device_equals_host_on_the_cpu_fixtures(gpu_decoder, cases, name):
    """Also the check that the device's fp64 division, square root and uncontracted products are
    the host's."""
    (depth, inst), cam, dets, modes, params, pose_params = cases[name]
    _both(gpu_decoder.ctx, depth, inst, cam, dets, modes, params, pose_params)


@pytest.mark.parametrize("w,h", [(641, 5), (63, 70)])
def test_device_equals_host_on_odd_image_sizes(gpu_decoder, w, h):
    depth, inst, cam = TF._odd_frame(w, h, 3)
    dets = [PC.det(1), PC.det(2), PC.det(1, bbox=(3, 1, w - 4, h - 2)), PC.det(2, PC.GIVEN_POSE)]
    modes = [CUB, FLIP, CUB, GIVEN]
    for params, pose_params in ((dict(max_pts=100, max_bg=64, min_mask_area=20, downsample=1, expand=2),
                                 dict(outlier_radius=PC.INF, min_points=20)),
                                (dict(max_pts=4096, max_bg=4096, min_mask_area=20, downsample=2, expand=0),
                                 dict(outlier_radius=0.9, box_margin=1.05))):
        _, _, _, _, recs, precs = _both(gpu_decoder.ctx, depth, inst, cam, dets, modes, params, pose_params)
        assert all(r.status == 0 and r.n_pts > 0 and r.n_bg > 0 for r in recs)
        assert [p.status for p in precs] == [PO.OK, PO.OK, PO.OK, PO.NOT_ASKED]
    assert any(p.n_kept < p.n_in for p in precs[:3])


def test_device_equals_host_on_a_whole_image_mask(gpu_decoder):
    depth, _, cam = TF._odd_frame(130, 67, 4)
    inst = np.full((67, 130), 9, np.int32)
    for params, pose_params in ((dict(max_pts=300, min_mask_area=100), dict(outlier_radius=1.5)),
                                (dict(max_pts=10000, min_mask_area=100, far=2.4), dict(outlier_radius=1.0))):
        _, _, _, _, recs, precs = _both(gpu_decoder.ctx, depth, inst, cam, [PC.det(9), PC.det(9)], [CUB, FLIP], params,
                                        pose_params)
        assert recs[0].n_mask == 130 * 67 and recs[0].n_bg == 0
        assert precs[0].status == PO.OK and precs[0].n_in == recs[0].n_pts and 50 <= precs[0].n_kept <= precs[0].n_in
    assert precs[0].n_in > 4096                                   # more points than any on-chip buffer could cap


# ------------------------------------------------------------------ capacity batches
@pytest.fixture(scope="module")
def frames(gpu_decoder):
    """Two rendered frames of two objects (test_gpu_frame.py's), the second with label 1 erased;
    in both a strip of each mask is pushed onto the background's side so that the passes drop
    points: 3 rows of label 0's pixels get depth + 1.2 (inside the radius, outside the box)."""
    from reconstruct.optimizer import SdfRenderer

    ren = SdfRenderer(gpu_decoder, TF.RW, TF.RH, RCAM["fx"], RCAM["fy"], RCAM["cx"], RCAM["cy"])
    out = []
    for k, ts in enumerate((((-2.6, 0.1, 15.0), (2.6, -0.2, 15.5)), ((-1.9, 0.6, 14.0), (2.2, -0.5, 16.0)))):
        poses = [TF._pose(i, t) for i, t in enumerate(ts)]
        img = ren.render([(poses[i], TF._code(i)) for i in range(2)])
        inst, depth = img["instance"].copy(), img["depth"].copy()
        if k == 1:
            inst[inst == 1] = -1
        vs, us = np.nonzero(inst == 0)
        rows = np.unique(vs)[2:5 + k]
        sel = np.isin(vs, rows)
        depth[vs[sel], us[sel]] += np.float32(1.2)
        out.append((depth, inst, poses))
    ren.close()
    return out


def _dets(poses, spec):
    """spec: (label, mode) pairs; a given detection starts beside the rendered pose."""
    out = []
    for lab, mode in spec:
        T = None
        if mode == GIVEN:
            T = poses[min(lab, 1)].copy()
            T[:3, 3] += np.float32(0.05)
        out.append(dict(label=lab, t_cam_obj=T, code=None, bbox=None))
    return out, [m for _, m in spec]


class Batch(TF.Batch):
    def poses(self, depth, inst, dets, modes, pose_params=POSE, cam=RCAM, **params):
        """dsr_batch_refill_frame_poses + run + download + both record kinds"""
        from reconstruct import _libdsr as L
        from reconstruct import utils as U

        fd, keep = U.frame_dets([U._with_pose(d) for d in dets])
        n = len(dets)
        m = np.ascontiguousarray(modes, np.int32)
        self.ctx.check(self.lib.dsr_batch_refill_frame_poses(
            self.h, U.frame_camera(cam), U.frame_params(**params), U.frame_pose_params(pose_params), L.fptr(depth),
            L.iptr(inst), n, fd, L.iptr(m)), "refill_frame_poses")
        outs = self.run(n)
        recs, precs = (L.FrameDetOut * n)(), (L.FramePoseOut * n)()
        self.ctx.check(self.lib.dsr_batch_frame_info(self.h, recs), "frame_info")
        self.ctx.check(self.lib.dsr_batch_frame_pose_info(self.h, precs), "frame_pose_info")
        return outs, [U.frame_record(r) for r in recs], [U.frame_pose_record(r) for r in precs]

    def host_poses(self, depth, inst, dets, modes, pose_params=POSE, cam=RCAM, **params):
        """dsr_frame_poses_host arrays and poses + dsr_batch_refill + run + download"""
        from reconstruct import _libdsr as L

        rc, pts, rays, dobs, recs, precs = PC.run("host", depth, inst, cam, dets, modes, params, pose_params)
        assert rc == 0
        n = len(dets)
        ins = (L.ObjectIn * n)()
        for i, (r, p) in enumerate(zip(recs, precs)):
            n_p, n_r = PC.counted(r, p)
            ins[i].t_cam_obj[:] = p.t_cam_obj.reshape(16).tolist()
            ins[i].pts, ins[i].n_pts = L.fptr(pts[i]), n_p
            ins[i].rays, ins[i].n_rays = L.fptr(rays[i]), n_r
            ins[i].depth, ins[i].n_depth = L.fptr(dobs[i]), n_p
        self.ctx.check(self.lib.dsr_batch_refill(self.h, n, ins), "refill")
        return self.run(n), recs, precs


def _same_records(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert PC.same_pose_record(x, y), (x, y)


def test_pose_refill_equals_host_refill(gpu_decoder, frames):
    b = Batch(TF._opt(gpu_decoder), 4, 256, 456)
    try:
        dropped = False
        for depth, inst, poses in frames:
            dets, modes = _dets(poses, ((0, CUB), (1, CUB), (0, FLIP), (1, GIVEN)))
            fo, frecs, fprecs = b.poses(depth, inst, dets, modes, **PARAMS)
            ho, hrecs, hprecs = b.host_poses(depth, inst, dets, modes, **PARAMS)
            assert frecs == hrecs
            _same_records(fprecs, hprecs)
            assert bytes(fo) == bytes(ho)
            assert fprecs[0].status == fprecs[2].status == PO.OK
            dropped = dropped or any(p.status == PO.OK and p.n_kept < p.n_in for p in fprecs)
        assert dropped                                            # the compaction moved rows
        assert all(o.iters_done == 2 for o in fo[:1])
    finally:
        b.close()


def test_pose_refills_replay_one_graph(gpu_decoder, frames):
    """Two different frames through one DSR_BATCH_GRAPH batch, the second with label 1 erased and
    other counts: one capture, then replays, and the records of an eager batch and of the host
    route."""
    from reconstruct import _libdsr as L

    opt = TF._opt(gpu_decoder)
    g, e = Batch(opt, 3, 256, 456, L.BATCH_GRAPH), Batch(opt, 3, 256, 456)
    try:
        kept = []
        for k, (depth, inst, poses) in enumerate(frames):
            dets, modes = _dets(poses, ((0, CUB), (1, CUB), (0, FLIP)))
            go, grecs, gprecs = g.poses(depth, inst, dets, modes, **PARAMS)
            eo, erecs, eprecs = e.poses(depth, inst, dets, modes, **PARAMS)
            ho, hrecs, hprecs = e.host_poses(depth, inst, dets, modes, **PARAMS)
            assert grecs == erecs == hrecs
            _same_records(gprecs, eprecs)
            _same_records(gprecs, hprecs)
            assert bytes(go) == bytes(eo) == bytes(ho)
            assert [p.status for p in gprecs] == ([PO.OK, PO.OK, PO.OK] if k == 0 else [PO.OK, PO.NO_INPUT, PO.OK])
            assert not go[1].is_good or k == 0
            kept.append(gprecs[0].n_kept)
        assert kept[0] != kept[1]
        st = L.Stats()
        opt._ctx.check(opt._ctx.lib.dsr_batch_stats(g.h, C.byref(st)), "stats")
        assert st.graph_captures == 1 and st.graph_replays >= 1, (st.graph_captures, st.graph_replays)
    finally:
        g.close()
        e.close()


def test_all_given_equals_the_plain_frame_refill(gpu_decoder, frames):
    depth, inst, poses = frames[0]
    b = Batch(TF._opt(gpu_decoder), 2, 256, 456)
    try:
        dets, modes = _dets(poses, ((0, GIVEN), (1, GIVEN)))
        po, precs, pprecs = b.poses(depth, inst, dets, modes, **PARAMS)
        fo, frecs = b.frame(depth, inst, dets, **PARAMS)
        assert precs == frecs and bytes(po) == bytes(fo)
        assert [p.status for p in pprecs] == [PO.NOT_ASKED] * 2 and [p.n_in for p in pprecs] == [r.n_pts for r in frecs]
        assert all(np.array_equal(p.t_cam_obj, d["t_cam_obj"]) for p, d in zip(pprecs, dets))
    finally:
        b.close()


def test_errors_leave_the_batch_usable(gpu_decoder, frames):
    from reconstruct import _libdsr as L
    from reconstruct import utils as U

    depth, inst, poses = frames[0]
    opt = TF._opt(gpu_decoder)
    ctx, lib = opt._ctx, opt._ctx.lib
    b = Batch(opt, 2, 256, 456)
    try:
        dets, modes = _dets(poses, ((0, CUB), (1, CUB), (0, FLIP)))
        fd, keep = U.frame_dets([U._with_pose(d) for d in dets])
        cam = U.frame_camera(RCAM)

        def refill(n=2, modes_=(CUB, CUB, FLIP), pose=None, **params):
            m = np.asarray(modes_, np.int32)
            return lib.dsr_batch_refill_frame_poses(b.h, cam, U.frame_params(**dict(PARAMS, **params)),
                                                    U.frame_pose_params(dict(POSE, **(pose or {}))), L.fptr(depth),
                                                    L.iptr(inst), n, fd, L.iptr(m))

        assert refill(max_pts=257) < 0 and b"max_pts" in lib.dsr_last_error(ctx.handle)
        assert refill(max_bg=201) < 0 and b"max_rays" in lib.dsr_last_error(ctx.handle)
        assert refill(n=3) < 0 and b"capacity" in lib.dsr_last_error(ctx.handle)
        assert refill(max_pts=0) < 0
        assert refill(pose=dict(min_points=0)) < 0 and b"min_points" in lib.dsr_last_error(ctx.handle)
        assert refill(pose=dict(lo_pct=95)) < 0 and b"lo_pct" in lib.dsr_last_error(ctx.handle)
        assert refill(pose=dict(outlier_radius=float("nan"))) < 0 and refill(pose=dict(box_margin=0.0)) < 0
        assert refill(pose=dict(scale_factor=-1.0)) < 0 and refill(pose=dict(up=(0.0, 0.0, 0.0))) < 0
        assert refill(modes_=(CUB, 7, CUB)) < 0 and b"mode" in lib.dsr_last_error(ctx.handle)
        assert lib.dsr_batch_refill_frame_poses(b.h, cam, U.frame_params(**PARAMS), None, L.fptr(depth), L.iptr(inst),
                                                2, fd, L.iptr(np.zeros(2, np.int32))) < 0
        precs = (L.FramePoseOut * 2)()
        assert lib.dsr_batch_frame_pose_info(b.h, precs) < 0          # nothing filled yet
        b.frame(depth, inst, _dets(poses, ((0, GIVEN), (1, GIVEN)))[0], **PARAMS)
        assert lib.dsr_batch_frame_pose_info(b.h, precs) < 0          # a plain frame refill
        assert b"poses" in lib.dsr_last_error(ctx.handle)
        assert refill() == 0                                          # the batch is still usable
        assert lib.dsr_batch_frame_pose_info(b.h, precs) == 0 and precs[0].status == PO.OK
        recs = (L.FrameDetOut * 2)()
        assert lib.dsr_batch_frame_info(b.h, recs) == 0 and recs[0].status == 0
        outs = b.run(2)
        assert outs[0].iters_done == 2
    finally:
        b.close()


def test_reconstruct_frame_without_poses(gpu_decoder, frames):
    """Optimizer.reconstruct_frame with pose-less detections (one not yet reconstructed, so its
    cuboid-flipped duplicate runs) in slot, graph and oneshot modes against reconstruct_keyframe
    over utils.frame_poses of the same hypotheses: the same results, the same hypothesis chosen."""
    from reconstruct import utils as U

    depth, inst, poses = frames[0]
    given = poses[1].copy()
    given[:3, 3] += np.float32(0.05)
    dets = [dict(label=0, reconstructed=False), dict(label=1, t_cam_obj=None, code=TF._code(1), reconstructed=True),
            dict(label=1, t_cam_obj=given, reconstructed=True), dict(label=4, reconstructed=False)]
    hyp = [dict(dets[0], mode=CUB), dict(dets[0], mode=FLIP), dets[1], dets[2], dict(dets[3], mode=CUB),
           dict(dets[3], mode=FLIP)]
    pairs = [(0, 1), (1 + 1, None), (3, None), (4, 5)]
    objects, records, precs = U.frame_poses(depth, inst, hyp, RCAM, POSE, **PARAMS)
    results = {}
    for mode in ("slot", "graph", "oneshot"):
        opt = TF._opt(gpu_decoder)
        opt.keyframe_mode = mode
        got = opt.reconstruct_frame(depth, inst, dets, RCAM, pose_params=POSE, **PARAMS)
        assert len(opt._slots) == (0 if mode == "oneshot" else 1)
        runs = opt.reconstruct_keyframe([ob + (True,) for ob in objects])
        ref, chosen = [], []
        for i, j in pairs:
            k = j if j is not None and float(runs[i]["loss"]) > float(runs[j]["loss"]) else i
            ref.append(runs[k])
            chosen.append(k)
        TF._same(got, ref)
        for g, k in zip(got, chosen):
            assert g["ingest"] == records[k] and PC.same_pose_record(g["pose_init"], precs[k]), k
        assert [g["pose_init"].status for g in got] == [PO.OK, PO.OK, PO.NOT_ASKED, PO.NO_INPUT]
        assert [g["is_good"] for g in got][3] is False or not got[3]["is_good"]
        results[mode] = (got, chosen)
        opt.close_slots()
    for mode in ("slot", "graph"):
        TF._same(results[mode][0], results["oneshot"][0])
        assert results[mode][1] == results["oneshot"][1]
