"""``reconstruct.optimizer`` — the Python API the C++ ORB-SLAM2 side calls (pybind11).

Same class / method names, argument meaning and return conventions as the
reference's ``reconstruct/optimizer.py``, but every numeric step
runs in libdsr's HIP kernels on an MI355X (``include/dsr.h``):

* ``Optimizer(decoder, configs)`` — optimizer.py:26-43
* ``Optimizer.reconstruct_object(t_cam_obj, pts, rays, depth, code=None)`` —
  optimizer.py:90-205 -> ``dsr_reconstruct_batch`` with one object.  Numeric
  failure returns ``is_good=False`` with ``t_cam_obj = code = None`` and ``loss``
  = the previous iteration's loss (0. if the first iteration failed), exactly
  like the reference (optimizer.py:132-152).
* ``Optimizer.reconstruct_objects([...])`` — NEW batched form: all objects of a
  keyframe / frame in one device pass.
* ``Optimizer.reconstruct_objects_views([...])`` / ``reconstruct_object_views`` — NEW: one
  code and one pose per object fitted to the pooled residuals of several keyframes' views
  -> ``dsr_reconstruct_views``.
* ``Optimizer.reconstruct_frame(depth, instance, detections, camera)`` — NEW: a keyframe straight
  from a depth image and an instance-label image; device kernels build every detection's points
  and rays in the slots of a capacity batch -> ``dsr_batch_refill_frame``.
* ``Optimizer.reconstruct_lidar_frame(velo, instance, masks, detections, camera, t_cam_velo)`` —
  NEW: a KITTI keyframe straight from its Velodyne sweep, the 3-D detector's boxes and the
  instance-label image (kitti_sequence.py:99-216 on the device) -> ``dsr_batch_refill_lidar``
  (DESIGN.md §3.5d).
* ``Optimizer.compute_sdf_loss_objectpoint_zhjd(pts_obj, code)`` —
  optimizer.py:207-213 -> ``dsr_sdf_eval``.
* ``Optimizer.estimate_pose_cam_obj(...)`` — optimizer.py:46-87 -> ``dsr_pose_only``.
* ``Optimizer.track_objects([...])`` / ``track_lidar_frame(...)`` — NEW: the per-detection
  ``estimate_pose_cam_obj`` loop of LocalMapping_util.cc:103-110 through a resident
  ``reconstruct.tracker.ObjectTracker`` -> ``dsr_tracker_*``.
* ``MeshExtractor`` — optimizer.py:216-233 -> ``dsr_mesher_*`` (grid decode and
  marching cubes on device).

There is no CPU fallback: without libdsr / a gfx950 device these raise DsrError.
"""
from __future__ import annotations

import ctypes as C
import os
import time

import numpy as np

from reconstruct import _libdsr as L
from reconstruct.utils import ForceKeyErrorDict, create_voxel_grid

_VERBOSE = os.environ.get("DSR_VERBOSE", "0") != "0"


def _code(code, code_len):
    """``code[:code_len]`` as a contiguous float32 vector; the C side reads exactly
    code_len floats, so a shorter array is an error, never an out-of-bounds read."""
    c = np.ascontiguousarray(np.asarray(code, np.float32).reshape(-1)[:code_len])
    if c.shape[0] != code_len:
        raise ValueError(f"code must hold at least {code_len} values, got {c.shape[0]}")
    return c


def _f32(a, shape_tail=None):
    a = np.ascontiguousarray(np.asarray(a), dtype=np.float32)
    if shape_tail is not None and (a.ndim != 2 or a.shape[1] != shape_tail):
        raise ValueError(f"expected an (N, {shape_tail}) array, got {a.shape}")
    return a


class Optimizer(object):
    def __init__(self, decoder, configs):
        self.decoder = decoder
        optim_cfg = configs.optimizer
        jo = optim_cfg.joint_optim
        self.k1 = jo.k1
        self.k2 = jo.k2
        self.k3 = jo.k3
        self.k4 = jo.k4
        self.b1 = jo.b1
        self.b2 = jo.b2
        self.lr = jo.learning_rate
        self.s_damp = jo.scale_damping
        self.num_iterations_joint_optim = jo.num_iterations
        self.code_len = optim_cfg.code_len
        self.num_depth_samples = optim_cfg.num_depth_samples
        self.cut_off = optim_cfg.cut_off_threshold
        self.num_iterations_pose_only = 5
        if configs.data_type == "KITTI":
            self.num_iterations_pose_only = optim_cfg.pose_only_optim.num_iterations
        self.params = L.OptimParams(
            float(self.k1), float(self.k2), float(self.k3), float(self.k4), float(self.b1),
            float(self.b2), float(self.lr), float(self.s_damp),
            int(self.num_iterations_joint_optim), int(self.code_len),
            int(self.num_depth_samples), float(self.cut_off), int(self.num_iterations_pose_only))
        self.last_stats = None
        # keyframe stream (BASELINE config 5): "graph" = fixed-capacity slot batches refilled per
        # keyframe, each replaying ONE captured hipGraph; "slot" = the same slots run eagerly;
        # "oneshot" = a new batch per keyframe (dsr_batch_create)
        self.keyframe_mode = os.environ.get("DSR_KEYFRAME_MODE", "graph")
        self._slots = []

    # ------------------------------------------------------------------ helpers
    @property
    def _ctx(self):
        return self.decoder.ctx

    def _object_in(self, t_cam_obj, pts, rays, depth, code, keep, pose_is_obj_cam=False):
        t = _f32(t_cam_obj).reshape(4, 4)
        pts = _f32(pts, 3)
        rays = _f32(rays, 3)
        depth = np.ascontiguousarray(np.asarray(depth, np.float32).reshape(-1))
        if depth.shape[0] > rays.shape[0]:
            raise ValueError("depth holds more values than there are rays")
        c = None if code is None else _code(code, self.code_len)
        keep.extend([pts, rays, depth, c])
        rec = L.ObjectIn()
        rec.t_cam_obj[:] = t.reshape(-1).tolist()
        rec.pts, rec.n_pts = L.fptr(pts), pts.shape[0]
        rec.rays, rec.n_rays = L.fptr(rays), rays.shape[0]
        rec.depth, rec.n_depth = L.fptr(depth), depth.shape[0]
        rec.code = L.fptr(c)
        rec.pose_is_obj_cam = 1 if pose_is_obj_cam else 0
        return rec

    @staticmethod
    def _result(o, code_len=64):
        """An out-record as the reference's result dict; ``code`` holds code_len values (the
        record's 64-wide code carries a 32-D code in its first 32, LocalMapping_util.cc:416-422)."""
        if o.is_good:
            return ForceKeyErrorDict(t_cam_obj=np.ctypeslib.as_array(o.t_cam_obj).reshape(4, 4).copy(),
                                     code=np.ctypeslib.as_array(o.code)[:code_len].copy(),
                                     is_good=True, loss=float(o.loss))
        return ForceKeyErrorDict(t_cam_obj=None, code=None, is_good=False, loss=float(o.loss))

    def _trace_bufs(self, n):
        """dsr_trace records for n objects and the numpy buffers they point into."""
        it = max(1, self.num_iterations_joint_optim)
        bufs = [dict(H=np.zeros((it, 71, 71), np.float32), b=np.zeros((it, 71), np.float32),
                     dx=np.zeros((it, 71), np.float32), loss=np.zeros(it, np.float32),
                     sdf_loss=np.zeros(it, np.float32), render_loss=np.zeros(it, np.float32),
                     n_valid=np.zeros(it, np.int32), k=np.zeros(it, np.int32),
                     t_obj_cam=np.zeros((it, 4, 4), np.float32),
                     z=np.zeros((it, self.code_len), np.float32),
                     n_decoded=np.zeros(it, np.int32), n_refined=np.zeros(it, np.int32)) for _ in range(n)]
        tr = (L.Trace * n)()
        for i, bb in enumerate(bufs):
            tr[i] = L.Trace(*(L.fptr(bb[k]) for k in ("H", "b", "dx", "loss", "sdf_loss",
                                                      "render_loss")),
                            L.iptr(bb["n_valid"]), L.iptr(bb["k"]), L.fptr(bb["t_obj_cam"]),
                            L.fptr(bb["z"]), L.iptr(bb["n_decoded"]), L.iptr(bb["n_refined"]))
        return tr, bufs

    # ------------------------------------------------------------------ API
    def reconstruct_object(self, t_cam_obj, pts, rays, depth, code=None):
        """optimizer.py:90-205 (one object)."""
        return self.reconstruct_objects([(t_cam_obj, pts, rays, depth, code)])[0]

    def reconstruct_objects(self, objects, trace=False, pose_is_obj_cam=False):
        """Batched ``reconstruct_object``: ``objects`` is a list of
        ``(t_cam_obj, pts, rays, depth, code_or_None)``.  Returns a list of result dicts
        (and per-object traces when ``trace``)."""
        n = len(objects)
        if n == 0:
            return []
        keep = []
        ins = (L.ObjectIn * n)()
        for i, ob in enumerate(objects):
            t, p, r, d = ob[:4]
            c = ob[4] if len(ob) > 4 else None
            ins[i] = self._object_in(t, p, r, d, c, keep, pose_is_obj_cam)
        outs = (L.ObjectOut * n)()
        tr, bufs = self._trace_bufs(n) if trace else (None, None)
        t0 = time.time()
        ctx = self._ctx
        ctx.check(ctx.lib.dsr_reconstruct_batch(ctx.handle, self.decoder.handle,
                                                C.byref(self.params), n, ins, outs, tr),
                  "dsr_reconstruct_batch")
        if _VERBOSE:
            print("Reconstruction takes %f seconds" % (time.time() - t0))
        res = [self._result(outs[i], self.code_len) for i in range(n)]
        for i in range(n):
            res[i]["iters_done"] = int(outs[i].iters_done)
            res[i]["fail_reason"] = L.FAIL_REASONS.get(int(outs[i].fail_reason), "?")
        if trace:
            return res, bufs
        return res

    def reconstruct_object_views(self, t_cam_obj, views, code=None):
        """One object fitted jointly to several cameras' observations (``reconstruct_objects_views``
        with one object)."""
        return self.reconstruct_objects_views([(t_cam_obj, views, code)])[0]

    def reconstruct_objects_views(self, objects, trace=False, pose_is_obj_cam=False):
        """``reconstruct_objects`` with ONE code and ONE pose per object fitted to the pooled
        residuals of several views (dsr_reconstruct_views, include/dsr.h): ``objects`` is a list of
        ``(t_cam_obj, views, code_or_None)`` and ``views`` a list of ``(t_view_ref, pts, rays,
        depth)`` — view 0 the reference view (``t_view_ref`` the identity; ``t_cam_obj`` and the
        result pose are in its camera frame), view v with the rigid ``x_view = t_view_ref @ x_ref``
        (``reconstruct.utils.views_from_world`` builds them from keyframe poses) and its own points,
        rays and depths in its own camera frame.  Returns the result dicts of
        ``reconstruct_objects`` plus ``fail_view`` (the view that failed the object, -1 if none)
        and, with ``trace``, the per-object traces of the pooled normal equations.  The underlying
        batch's statistics are left in ``last_stats``."""
        n = len(objects)
        if n == 0:
            return ([], []) if trace else []
        ctx = self._ctx
        if not hasattr(ctx.lib, "dsr_reconstruct_views"):
            raise L.DsrError("this libdsr build has no dsr_reconstruct_views")
        keep = []
        ins = (L.ViewsObjectIn * n)()
        for i, ob in enumerate(objects):
            t, views = ob[:2]
            code = ob[2] if len(ob) > 2 else None
            c = None if code is None else _code(code, self.code_len)
            vs = (L.ViewIn * max(1, len(views)))()
            for v, (t_view_ref, pts, rays, depth) in enumerate(views):
                tv = np.asarray(t_view_ref, np.float64).reshape(4, 4).astype(np.float32)
                pts, rays = _f32(pts, 3), _f32(rays, 3)
                depth = np.ascontiguousarray(np.asarray(depth, np.float32).reshape(-1))
                if depth.shape[0] > rays.shape[0]:
                    raise ValueError("depth holds more values than there are rays")
                keep.extend([pts, rays, depth])
                vs[v].t_view_ref[:] = tv.reshape(-1).tolist()
                vs[v].pts, vs[v].n_pts = L.fptr(pts), pts.shape[0]
                vs[v].rays, vs[v].n_rays = L.fptr(rays), rays.shape[0]
                vs[v].depth, vs[v].n_depth = L.fptr(depth), depth.shape[0]
            keep.extend([vs, c])
            ins[i].t_cam_obj[:] = _f32(t).reshape(-1).tolist()
            ins[i].code = L.fptr(c)
            ins[i].pose_is_obj_cam = 1 if pose_is_obj_cam else 0
            ins[i].n_views = len(views)
            ins[i].views = vs
        outs = (L.ObjectOut * n)()
        tr, bufs = self._trace_bufs(n) if trace else (None, None)
        fail_view = np.full(n, -1, np.int32)
        st = L.Stats()
        ctx.check(ctx.lib.dsr_reconstruct_views(ctx.handle, self.decoder.handle, C.byref(self.params), n, ins,
                                                outs, tr, L.iptr(fail_view), C.byref(st)),
                  "dsr_reconstruct_views")
        self.last_stats = st
        res = [self._result(outs[i], self.code_len) for i in range(n)]
        for i in range(n):
            res[i]["iters_done"] = int(outs[i].iters_done)
            res[i]["fail_reason"] = L.FAIL_REASONS.get(int(outs[i].fail_reason), "?")
            res[i]["fail_view"] = int(fail_view[i])
        if trace:
            return res, bufs
        return res

    def reconstruct_objects_async(self, objects):
        """Start ``reconstruct_objects(objects)`` and return at once with a
        :class:`BatchHandle`: the inputs are uploaded (dsr_batch_create), the whole GN run is
        enqueued on the device (dsr_batch_run) and the host is free — e.g. for the
        LocalMapping thread's bundle adjustment, which the reference runs after the
        reconstructions (LocalMapping.cc:99-128) — until ``handle.wait()``."""
        return BatchHandle(self, objects)

    def reconstruct_keyframe_async(self, detections):
        """One keyframe's object reconstructions (LocalMapping_util.cc:165-206, 394-410) as
        ONE asynchronous batched call.  ``detections``: list of ``(t_cam_obj, pts, rays,
        depth, code, reconstructed)``.  For a detection whose object is not yet
        reconstructed the reference also runs the left-right flipped hypothesis —
        ``Sim3Two`` with columns 0 and 2 negated, i.e. ``t_cam_obj @ diag(-1, 1, -1, 1)``
        (exact in fp32) — and keeps it when the original's loss is larger
        (LocalMapping_util.cc:400-410; a failed run's loss takes part in that comparison as
        it does there).  Both hypotheses go into the same batch; ``wait()`` applies the
        choice and returns one result per detection."""
        return KeyframeHandle(self, detections)

    def reconstruct_keyframe(self, detections, mesher=None):
        """``reconstruct_keyframe_async(detections).wait()``.  With ``mesher`` (a
        :class:`MeshExtractor`) the good objects are meshed by one batch call
        (LocalMapping_util.cc:197, 429 mesh every successful reconstruction) and every result
        carries ``vertices`` / ``faces`` (``None`` for a failed object)."""
        return self._mesh_results(self.reconstruct_keyframe_async(detections).wait(), mesher)

    @staticmethod
    def _mesh_results(res, mesher):
        if mesher is None:
            return res
        good = [i for i, r in enumerate(res) if r["is_good"]]
        meshes = mesher.extract_meshes_from_codes([res[i]["code"] for i in good])
        for r in res:
            r["vertices"] = r["faces"] = None
        for i, mesh in zip(good, meshes):
            res[i]["vertices"], res[i]["faces"] = mesh.vertices, mesh.faces
        return res

    def reconstruct_frame(self, depth, instance, detections, camera, mesher=None, pose_params=None, **params):
        """One keyframe straight from a depth image and an instance-label image (the format
        ``SdfRenderer.render`` emits): what ``reconstruct_keyframe`` returns for the inputs
        ``reconstruct.utils.frame_inputs`` builds, without building them on the host.  The images
        are uploaded once and device kernels fill the slots of a fixed-capacity batch
        (dsr_batch_refill_frame; the rule is DESIGN.md §3.5b, replacing get_detections /
        pixels_sampler / get_rays, kitti_sequence.py:70-92, mono_sequence.py:51-73,
        loss_utils.py:23-37).  ``detections``: dicts ``{label, t_cam_obj, code=None, bbox=None,
        reconstructed=True}``; for ``reconstructed=False`` the flipped hypothesis
        (``t_cam_obj @ diag(-1, 1, -1, 1)``, same label, so the same pixels) joins the batch and
        the choice between the two is ``KeyframeHandle``'s.  ``camera``: ``utils.frame_camera``;
        ``params``: ``utils.FRAME_PARAM_NAMES`` (the slot's capacity comes from max_pts / max_bg).
        Every result carries the detection's ingest record as ``ingest``.  With ``keyframe_mode``
        "oneshot", or when no slot is within the capacity bounds, the inputs are built on the host
        (``frame_inputs``) and run through ``reconstruct_keyframe``.

        A detection without ``t_cam_obj`` (or with ``None``) — the reference's mono / RGB-D call
        site, LocalMapping_util.cc:284-410, where no 3-D detector supplies a pose — starts from the
        PCA cuboid of its own points with the outliers of ``MapObject::RemoveOutliersSimple`` /
        ``ComputeCuboidPCA_onlyformono`` (MapObject.cc:249-283, :330-443) left out, computed on the
        device after the ingest (dsr_batch_refill_frame_poses; the rule is DESIGN.md §3.5c); with
        ``reconstructed=False`` its duplicate is the cuboid-flipped mode, flipped on the device.
        ``pose_params``: a dict over ``utils.FRAME_POSE_PARAM_NAMES``.  Every result carries the
        pose record as ``pose_init`` (``utils.frame_pose_record``) beside ``ingest``; when every
        detection brings a pose the call goes through dsr_batch_refill_frame exactly as before.
        The fallback then runs ``utils.frame_poses`` + ``reconstruct_keyframe``: bitwise the same
        results."""
        from reconstruct import utils as U

        cam = U.frame_camera(camera)
        p = U.frame_params(**params)
        depth, instance = U.frame_images(depth, instance, cam)
        poses = any(det.get("t_cam_obj") is None for det in detections)
        q = U.frame_pose_params(pose_params) if poses or pose_params is not None else None
        hyp, pairs = [], []
        for det in detections:
            i, j = len(hyp), None
            cuboid = det.get("t_cam_obj") is None
            hyp.append(dict(det, mode=L.FRAME_POSE_CUBOID) if cuboid else dict(det, mode=None))
            if not det.get("reconstructed", True):
                j = len(hyp)
                if cuboid:
                    hyp.append(dict(det, mode=L.FRAME_POSE_CUBOID_FLIPPED))
                else:
                    hyp.append(dict(det, mode=None,
                                    t_cam_obj=np.asarray(det["t_cam_obj"], np.float32).reshape(4, 4) @ FLIP))
            pairs.append((i, j))
        n = len(hyp)
        if n == 0:
            return []
        ctx = self._ctx
        if poses and not hasattr(ctx.lib, "dsr_batch_refill_frame_poses"):
            raise L.DsrError("this libdsr has no dsr_batch_refill_frame_poses: detections without t_cam_obj need it")

        def given_record(h, ingest):
            return ForceKeyErrorDict(status=L.FRAME_POSE_NOT_ASKED, n_in=ingest.n_pts, n_near=0, n_kept=0,
                                     dims=np.zeros(3), eig=np.zeros(3),
                                     t_cam_obj=np.asarray(h["t_cam_obj"], np.float32).reshape(4, 4).copy())

        slot = None
        if hasattr(ctx.lib, "dsr_batch_refill_frame") and p.max_pts >= 1 and p.max_bg >= 0:
            slot = self._slot_for_caps(n, p.max_pts, p.max_pts + p.max_bg, n * (p.max_pts + p.max_bg))
        if slot is None and not poses:
            objects, records = U.frame_inputs(depth, instance, detections, cam, **params)
            res = self.reconstruct_keyframe([ob + (det.get("reconstructed", True),)
                                             for ob, det in zip(objects, detections)], mesher)
            for r, rec, det in zip(res, records, detections):
                r["ingest"] = rec
                r["pose_init"] = given_record(det, rec)
            return res
        if slot is None:                                       # host twin, every hypothesis its own object
            objects, records, precs = U.frame_poses(depth, instance, hyp, cam, q, **params)
            runs = self.reconstruct_keyframe([ob + (True,) for ob in objects])
            res = []
            for i, j in pairs:
                k = i
                if j is not None and float(runs[i]["loss"]) > float(runs[j]["loss"]):
                    k = j
                r = runs[k]
                r["ingest"], r["pose_init"] = records[k], precs[k]
                res.append(r)
            return self._mesh_results(res, mesher)
        dets, keep = U.frame_dets([U._with_pose(h) for h in hyp], self.code_len)
        infos = [("dsr_batch_frame_info", L.FrameDetOut)]
        if poses:
            modes = U.frame_pose_modes(hyp)
            ctx.check(ctx.lib.dsr_batch_refill_frame_poses(slot.handle, cam, p, q, L.fptr(depth), L.iptr(instance), n,
                                                           dets, L.iptr(modes)), "dsr_batch_refill_frame_poses")
            infos.append(("dsr_batch_frame_pose_info", L.FramePoseOut))
        else:
            ctx.check(ctx.lib.dsr_batch_refill_frame(slot.handle, cam, p, L.fptr(depth), L.iptr(instance), n, dets),
                      "dsr_batch_refill_frame")
        outs, recs, result = self._run_slot(slot, n, infos)
        res = []
        for i, j in pairs:
            k = i
            if j is not None and float(outs[i].loss) > float(outs[j].loss):
                k = j
            ingest = U.frame_record(recs[0][k])
            res.append(result(k, ingest=ingest, pose_init=(U.frame_pose_record(recs[1][k]) if poses
                                                            else given_record(hyp[k], ingest))))
        return self._mesh_results(res, mesher)

    def _run_slot(self, slot, n, infos):
        """The slot sequence after a refill of ``n`` objects: mark the slot busy, run, download the
        out-records, fetch the fill's info records (``infos``: (entry point, record type) pairs) and
        release the slot.  Returns the out-records, one record array per entry of ``infos``, and
        ``result(k, **more)``: out-record k as a result dict with ``iters_done``, ``fail_reason``
        and ``more``."""
        ctx = self._ctx
        outs = (L.ObjectOut * n)()
        recs = [(rtype * n)() for _, rtype in infos]
        slot.busy = True
        try:
            ctx.check(ctx.lib.dsr_batch_run(slot.handle), "dsr_batch_run")
            ctx.check(ctx.lib.dsr_batch_download(slot.handle, outs), "dsr_batch_download")
            for (name, _), rec in zip(infos, recs):
                ctx.check(getattr(ctx.lib, name)(slot.handle, rec), name)
        finally:
            slot.busy = False

        def result(k, **more):
            r = self._result(outs[k], self.code_len)
            r.update(iters_done=int(outs[k].iters_done),
                     fail_reason=L.FAIL_REASONS.get(int(outs[k].fail_reason), "?"), **more)
            return r

        return outs, recs, result

    def reconstruct_lidar_frame(self, velo, instance, masks, detections, camera, t_cam_velo, mesher=None, **params):
        """One KITTI keyframe straight from its Velodyne sweep, the 3-D detector's boxes and the
        instance-label image with its mask list: what ``reconstruct_keyframe`` returns for the
        inputs ``reconstruct.utils.lidar_inputs`` builds, without building them on the host.  The
        sweep and the image are uploaded once and device kernels crop, sub-sample, project,
        associate and fill the slots of a fixed-capacity batch (dsr_batch_refill_lidar; the rule is
        DESIGN.md §3.5d, replacing FrameWithLiDAR.get_detections, kitti_sequence.py:99-216, before
        CreateNewMapObjects_foronlyStereo, LocalMapping_util.cc:156-208).  ``masks``:
        ``utils.lidar_masks``; ``detections``: ``utils.lidar_dets``; ``camera``:
        ``utils.frame_camera``; ``params``: ``utils.LIDAR_PARAM_NAMES`` (the slot's capacity comes
        from max_pts / max_bg).  Every result carries the detection's ingest record as ``ingest``
        (``utils.lidar_record``); a detection that is not ok fails like an empty object.  There are
        no flipped hypotheses: the 3-D detector supplies the heading.  With ``keyframe_mode``
        "oneshot", or when no slot is within the capacity bounds, the inputs are built on the host
        (``lidar_inputs``) and run through ``reconstruct_keyframe``: bitwise the same results."""
        from reconstruct import utils as U

        cam = U.frame_camera(camera)
        p = U.lidar_params(**params)
        velo, instance, tcv = U.lidar_sweep(velo, instance, cam, t_cam_velo)
        n = len(detections)
        if n == 0:
            return []
        ctx = self._ctx
        slot = None
        if hasattr(ctx.lib, "dsr_batch_refill_lidar") and p.max_pts >= 1 and p.max_bg >= 0:
            slot = self._slot_for_caps(n, p.max_pts, p.max_pts + p.max_bg, n * (p.max_pts + p.max_bg))
        if slot is None:
            objects, records = U.lidar_inputs(velo, instance, masks, detections, cam, tcv, **params)
            res = self.reconstruct_keyframe([ob + (True,) for ob in objects], mesher)
            for r, rec in zip(res, records):
                r["ingest"] = rec
            return res
        dets, keep = U.lidar_dets(detections, self.code_len)
        ml = U.lidar_masks(masks)
        ctx.check(ctx.lib.dsr_batch_refill_lidar(slot.handle, cam, p, L.fptr(tcv), L.fptr(velo), velo.shape[0],
                                                 velo.shape[1], L.iptr(instance), len(masks), ml, n, dets),
                  "dsr_batch_refill_lidar")
        _, (recs,), result = self._run_slot(slot, n, [("dsr_batch_lidar_info", L.LidarDetOut)])
        return self._mesh_results([result(k, ingest=U.lidar_record(recs[k])) for k in range(n)], mesher)

    MAX_SLOTS = 4
    # A slot batch is laid out for max_obj x max_rays x M ray samples whatever the fill, and every
    # run launches its render chunks over that capacity (~580 B of device memory per sample with
    # the kept ReLU masks).  A keyframe only uses a slot whose capacity is at most SLOT_WASTE x its
    # own ray count (or SLOT_MIN_RAYS), a slot only grows while it stays inside that bound, and no
    # slot exceeds SLOT_MAX_SAMPLES ray samples (2^24: ~9.7 GB); otherwise the keyframe runs as a
    # one-shot batch (INTEGRATION.md §2 states the bound)
    SLOT_WASTE = 4.0
    SLOT_MIN_RAYS = 8 * 1024
    SLOT_MAX_SAMPLES = 1 << 24

    def _slot_ok(self, n_obj, n_rays_cap, real_rays):
        cap = n_obj * n_rays_cap
        return (cap <= max(self.SLOT_WASTE * real_rays, self.SLOT_MIN_RAYS)
                and cap * self.num_depth_samples <= self.SLOT_MAX_SAMPLES)

    def _slot_for(self, objects):
        """A free fixed-capacity batch (dsr_batch_create_capacity) that holds ``objects``, or
        None (``keyframe_mode`` "oneshot", every slot busy with an in-flight keyframe, or no slot
        within the capacity bounds above: the keyframe then runs as a one-shot batch).  A free
        slot is grown (replaced by a larger one) only when the grown size stays inside the bounds;
        otherwise the keyframe gets a slot of its own — beside the others while fewer than
        MAX_SLOTS exist, else in place of the least recently used free slot (a small
        keyframe no longer destroys a large free slot and its captured graph)."""
        if self.keyframe_mode not in ("slot", "graph") or not objects:
            return None
        rays = [_f32(ob[2], 3).shape[0] for ob in objects]
        return self._slot_for_caps(len(objects), max(_f32(ob[1], 3).shape[0] for ob in objects), max(rays), sum(rays))

    def _slot_for_caps(self, n, need_p, need_r, real):
        """``_slot_for`` by numbers: ``n`` objects of at most ``need_p`` points and ``need_r`` rays,
        ``real`` rays in all."""
        if self.keyframe_mode not in ("slot", "graph") or n <= 0:
            return None
        graph = self.keyframe_mode == "graph"
        self._slot_tick = getattr(self, "_slot_tick", 0) + 1
        free = [sl for sl in self._slots if not sl.busy and sl.graph == graph]
        for sl in free:
            if sl.fits(n, need_p, need_r) and self._slot_ok(sl.max_obj, sl.max_rays, real):
                sl.last_used = self._slot_tick
                return sl
        pad = lambda v: -(-v // 128) * 128  # noqa: E731
        cn, cp, cr = n, pad(need_p), pad(need_r)
        old = None
        for sl in free:                              # grow a free slot inside the bounds
            gn, gp, gr = max(cn, sl.max_obj), max(cp, sl.max_pts), max(cr, sl.max_rays)
            if self._slot_ok(gn, gr, real):
                old, (cn, cp, cr) = sl, (gn, gp, gr)
                break
        if old is None:
            if not self._slot_ok(cn, cr, real):
                return None
            if len(self._slots) >= self.MAX_SLOTS:   # evict the least recently used free slot
                if not free:
                    return None
                old = min(free, key=lambda sl: getattr(sl, "last_used", 0))
        if old is not None:
            self._slots.remove(old)
            old.close()
        sl = SlotBatch(self, cn, cp, cr, graph)
        sl.last_used = self._slot_tick
        self._slots.append(sl)
        return sl

    def close_slots(self):
        """Release the keyframe slot batches (their device memory goes back to the context pool)."""
        for sl in self._slots:
            sl.close()
        self._slots = []

    def estimate_pose_cam_obj(self, t_co_se3, scale, pts, code):
        """optimizer.py:46-87: pose-only SE(3) GN on the SDF term."""
        t = _f32(t_co_se3).reshape(4, 4)
        pts = _f32(pts, 3)
        c = _code(code, self.code_len)
        out = np.zeros((4, 4), np.float32)
        ctx = self._ctx
        ctx.check(ctx.lib.dsr_pose_only(ctx.handle, self.decoder.handle, C.byref(self.params),
                                        L.fptr(t), float(scale), L.fptr(pts), pts.shape[0],
                                        L.fptr(c), L.fptr(out)), "dsr_pose_only")
        return out

    def estimate_pose_cam_obj_batch(self, objects):
        """Batched ``estimate_pose_cam_obj``: ``objects`` is a list of
        ``(t_co_se3, scale, pts, code)``; every object's pose-only GN runs in one device
        pass per iteration (dsr_pose_only_batch).  The stereo path calls the single form
        once per associated object per keyframe (LocalMapping_util.cc:103-110)."""
        n = len(objects)
        if n == 0:
            return []
        keep = []
        ins = (L.PoseIn * n)()
        for i, (t, scale, pts, code) in enumerate(objects):
            t = _f32(t).reshape(4, 4)
            pts = _f32(pts, 3)
            c = _code(code, self.code_len)
            keep += [pts, c]
            rec = L.PoseIn()
            rec.t_co_se3[:] = t.reshape(-1).tolist()
            rec.scale = float(scale)
            rec.pts, rec.n_pts = L.fptr(pts), pts.shape[0]
            rec.code = L.fptr(c)
            ins[i] = rec
        out = np.zeros((n, 4, 4), np.float32)
        ctx = self._ctx
        ctx.check(ctx.lib.dsr_pose_only_batch(ctx.handle, self.decoder.handle, C.byref(self.params), n,
                                              ins, L.fptr(out)), "dsr_pose_only_batch")
        return [out[i] for i in range(n)]

    def _tracker_for(self, n_obj, n_pts):
        """The optimizer's one ``ObjectTracker``, recreated larger when a call does not fit."""
        from reconstruct.tracker import ObjectTracker

        tr = getattr(self, "_tracker", None)
        if tr is None or tr._h is None or not tr.fits(n_obj, n_pts):
            pad = lambda v, m: -(-max(v, 1) // m) * m  # noqa: E731
            cn, cp = pad(n_obj, 8), pad(n_pts, 64)
            if tr is not None:
                cn, cp = max(cn, tr.max_obj), max(cp, tr.max_pts)
                tr.close()
            tr = self._tracker = ObjectTracker(self, cn, cp)
        return tr

    def track_objects(self, objects):
        """``estimate_pose_cam_obj_batch`` through the optimizer's resident ``ObjectTracker``
        (reconstruct/tracker.py): the loop of
        LocalMapping::GetNewObservations_onyforStereo (LocalMapping_util.cc:103-110) as one call
        without per-call allocation or a host step inside the GN loop.  Returns ``(poses,
        records)``; the poses are bitwise those of ``estimate_pose_cam_obj_batch``."""
        n = len(objects)
        if n == 0:
            return [], []
        tr = self._tracker_for(n, max(_f32(ob[2], 3).shape[0] for ob in objects))
        tr.track(objects)
        return tr.result()

    def track_lidar_frame(self, velo, t_cam_velo, detections, priors, **params):
        """The same from a Velodyne sweep: every detection's surface points are cropped on the
        device (the rows of ``utils.lidar_inputs``) and tracked without coming back to the host.
        ``detections``, ``priors`` and ``params`` (max_pts, radius, box_margin): see
        ``ObjectTracker.track_lidar``.  Returns ``(poses, records)``."""
        from reconstruct import utils as U

        n = len(detections)
        if n == 0:
            return [], []
        tr = self._tracker_for(n, U.lidar_params(**params).max_pts)
        tr.track_lidar(velo, t_cam_velo, detections, priors, params)
        return tr.result()

    def track_frame(self, depth, instance, detections, priors, camera, **params):
        """The same from a depth image and an instance-label image (the RGB-D path): every
        detection's surface points are the ``pts`` rows of ``utils.frame_inputs``, built on the
        device and tracked without coming back to the host.  ``detections`` (``{label, code}``),
        ``priors`` (``(scale, t_co_se3)``), ``camera`` and ``params`` (max_pts, min_mask_area,
        near, far): see ``ObjectTracker.track_frame``.  Returns ``(poses, records)``."""
        from reconstruct import utils as U

        n = len(detections)
        if len(priors) != n:
            raise ValueError("one prior per detection")
        if n == 0:
            return [], []
        tr = self._tracker_for(n, U.frame_params(**params).max_pts)
        tr.track_frame(depth, instance, detections, priors, camera, params)
        return tr.result()

    def reconstruct_objects_multi(self, objects, decoders, return_path=False):
        """``reconstruct_objects`` spread over several devices from ONE process
        (dsr_reconstruct_multi_ex): ``decoders`` holds one decoder handle per device (e.g.
        ``[decoder_from_state(state, specs, device=g) for g in range(n)]``); objects are
        LPT-partitioned, each device's shard runs on its own host thread and one RCCL gather
        returns the records to the first device (host memory when RCCL refuses the device
        list); ``return_path`` adds which ("rccl" / "host").  One process per GPU is
        reconstruct.parallel.reconstruct_sharded."""
        n = len(objects)
        if n == 0:
            return []
        keep = []
        ins = (L.ObjectIn * n)()
        for i, ob in enumerate(objects):
            ins[i] = self._object_in(*ob[:4], ob[4] if len(ob) > 4 else None, keep)
        outs = (L.ObjectOut * n)()
        nd = len(decoders)
        ctxs = (C.c_void_p * nd)(*[d.ctx.handle.value for d in decoders])
        decs = (C.c_void_p * nd)(*[d.handle.value for d in decoders])
        ctx = decoders[0].ctx
        path = C.c_int(-1)
        ctx.check(ctx.lib.dsr_reconstruct_multi_ex(ctxs, decs, nd, C.byref(self.params), n, ins, outs,
                                                   C.byref(path)), "dsr_reconstruct_multi_ex")
        res = [self._result(outs[i], self.code_len) for i in range(n)]
        for i in range(n):
            res[i]["iters_done"] = int(outs[i].iters_done)
            res[i]["fail_reason"] = L.FAIL_REASONS.get(int(outs[i].fail_reason), "?")
        if return_path:
            return res, ("rccl" if path.value == L.GATHER_RCCL else "host")
        return res

    def compute_sdf_loss_objectpoint_zhjd(self, pts_surface_obj, code):
        """optimizer.py:207-213: mean decoder SDF of object-frame points."""
        sdf = sdf_eval(self.decoder, _code(code, self.code_len), pts_surface_obj)
        mean_value = np.float32(np.mean(sdf)) if sdf.size else np.float32(np.nan)
        if _VERBOSE:
            print("[mapobject sdf loss]python:", mean_value)
        return float(mean_value)


class SlotBatch:
    """A fixed-capacity batch (dsr_batch_create_capacity) that keyframe after keyframe is
    refilled (dsr_batch_refill) and re-run — with ``graph``, as replays of ONE hipGraph."""

    def __init__(self, opt, max_obj, max_pts, max_rays, graph):
        self.opt = opt
        self.max_obj, self.max_pts, self.max_rays, self.graph = max_obj, max_pts, max_rays, graph
        self.busy = False
        ctx = opt._ctx
        h = C.c_void_p()
        ctx.check(ctx.lib.dsr_batch_create_capacity(ctx.handle, opt.decoder.handle, C.byref(opt.params), max_obj,
                                                    max_pts, max_rays, L.BATCH_GRAPH if graph else 0, C.byref(h)),
                  "dsr_batch_create_capacity")
        self.handle = h

    def fits(self, n, n_pts, n_rays):
        return n <= self.max_obj and n_pts <= self.max_pts and n_rays <= self.max_rays

    def close(self):
        h = getattr(self, "handle", None)
        if h is not None:
            try:
                self.opt._ctx.lib.dsr_batch_destroy(h)
            except Exception:
                pass
            self.handle = None

    def __del__(self):
        self.close()


class BatchHandle:
    """An in-flight batched reconstruction (Optimizer.reconstruct_objects_async); with a
    ``slot`` (SlotBatch) the objects are refilled into that fixed-capacity batch instead of a
    new batch being created."""

    def __init__(self, opt, objects, slot=None):
        self.opt = opt
        self.n = len(objects)
        self._h = None
        self._res = None
        self._slot = None
        if self.n == 0:
            self._res = []
            return
        keep = []
        ins = (L.ObjectIn * self.n)()
        for i, ob in enumerate(objects):
            ins[i] = opt._object_in(*ob[:4], ob[4] if len(ob) > 4 else None, keep)
        ctx = opt._ctx
        if slot is not None:
            ctx.check(ctx.lib.dsr_batch_refill(slot.handle, self.n, ins), "dsr_batch_refill")
            ctx.check(ctx.lib.dsr_batch_run(slot.handle), "dsr_batch_run")
            slot.busy = True
            self._slot = slot
            self._h = slot.handle
            return
        h = C.c_void_p()
        ctx.check(ctx.lib.dsr_batch_create(ctx.handle, opt.decoder.handle, C.byref(opt.params), self.n,
                                           ins, C.byref(h)), "dsr_batch_create")
        self._h = h
        # DSR_GRAPH=1: the whole GN run is captured as one hipGraph and replayed
        # (dsr_batch_graph is a no-op otherwise)
        ctx.check(ctx.lib.dsr_batch_graph(h), "dsr_batch_graph")
        ctx.check(ctx.lib.dsr_batch_run(h), "dsr_batch_run")

    def done(self) -> bool:
        """True once the device has finished (never blocks)."""
        if self._res is not None:
            return True
        ctx = self.opt._ctx
        rc = ctx.lib.dsr_batch_query(self._h)
        if rc < 0:
            ctx.check(rc, "dsr_batch_query")
        return rc == 1

    def wait(self):
        """Block until the run finishes; the list of result dicts, like reconstruct_objects."""
        if self._res is None:
            ctx = self.opt._ctx
            outs = (L.ObjectOut * self.n)()
            try:
                ctx.check(ctx.lib.dsr_batch_download(self._h, outs), "dsr_batch_download")
            finally:
                self._release()
            res = [Optimizer._result(outs[i], self.opt.code_len) for i in range(self.n)]
            for i in range(self.n):
                res[i]["iters_done"] = int(outs[i].iters_done)
                res[i]["fail_reason"] = L.FAIL_REASONS.get(int(outs[i].fail_reason), "?")
            self._res = res
        return self._res

    def _release(self):
        if self._slot is not None:           # the slot batch stays; its next fill may start
            self._slot.busy = False
            self._slot = None
        elif self._h is not None:
            self.opt._ctx.lib.dsr_batch_destroy(self._h)
        self._h = None

    def __del__(self):
        if getattr(self, "_h", None) is not None:
            try:
                if self._slot is not None:   # an abandoned keyframe: finish its run before reuse
                    self.opt._ctx.lib.dsr_batch_sync(self._h)
                self._release()
            except Exception:
                pass


FLIP = np.diag(np.array([-1.0, 1.0, -1.0, 1.0], np.float32))


class KeyframeHandle:
    """In-flight keyframe batch (Optimizer.reconstruct_keyframe_async)."""

    def __init__(self, opt, detections):
        objs, self.pairs = [], []
        for det in detections:
            t, pts, rays, depth = det[:4]
            code = det[4] if len(det) > 4 else None
            done = bool(det[5]) if len(det) > 5 else False
            i = len(objs)
            objs.append((t, pts, rays, depth, code))
            j = None
            if not done:
                j = len(objs)
                objs.append((np.asarray(t, np.float32).reshape(4, 4) @ FLIP, pts, rays, depth, code))
            self.pairs.append((i, j))
        self.batch = BatchHandle(opt, objs, opt._slot_for(objs))

    def done(self) -> bool:
        return self.batch.done()

    def wait(self):
        res = self.batch.wait()
        out = []
        for i, j in self.pairs:
            r = res[i]
            if j is not None and float(r["loss"]) > float(res[j]["loss"]):
                r = res[j]
            out.append(r)
        return out


def sdf_eval(decoder, code, pts, with_jac=False):
    """decode_sdf / get_batch_sdf_jacobian (loss_utils.py:51-113) on device."""
    ctx = decoder.ctx
    pts = _f32(pts, 3)
    c = _code(code, decoder.code_len)
    n = pts.shape[0]
    sdf = np.zeros(n, np.float32)
    jac = np.zeros((n, c.shape[0] + 3), np.float32) if with_jac else None
    ctx.check(ctx.lib.dsr_sdf_eval(ctx.handle, decoder.handle, L.fptr(c), L.fptr(pts), n,
                                   L.fptr(sdf), L.fptr(jac)), "dsr_sdf_eval")
    return (sdf, jac) if with_jac else sdf


class MeshExtractor(object):
    """optimizer.py:216-233 — grid decode + marching cubes on device (dsr_mesher_*).

    The voxel grid is reconstruct.utils.create_voxel_grid (bit-exact, including the
    reference's true-division shear) and is uploaded once, like the reference builds it
    once in __init__.  The reference meshes with skimage.measure.marching_cubes_lewiner
    (utils.py:119-140); the build's marching cubes (dsr_mc.hpp) is a closed,
    consistently oriented surface through the same level set — vertex/face ORDER and
    the triangulation of ambiguous cells are its own (parity unpinned: skimage is absent,
    DESIGN.md §3.5)."""

    def __init__(self, decoder, code_len=64, voxels_dim=64):
        self.decoder = decoder
        self.code_len = code_len
        self.voxels_dim = voxels_dim
        self.voxel_points = create_voxel_grid(vol_dim=self.voxels_dim)
        ctx = decoder.ctx
        h = C.c_void_p()
        ctx.check(ctx.lib.dsr_mesher_create(ctx.handle, decoder.handle, L.fptr(self.voxel_points),
                                            self.voxels_dim, C.byref(h)), "dsr_mesher_create")
        self._h = h
        d = self.voxels_dim
        self._verts = np.zeros((3 * d ** 3, 3), np.float32)
        self._faces = np.zeros((5 * (d - 1) ** 3, 3), np.int32)

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                self.decoder.ctx.lib.dsr_mesher_destroy(h)
            except Exception:
                pass
            self._h = None

    def decode_grid(self, code):
        """The (voxels_dim^3,) SDF grid of optimizer.py:226 (decode_sdf on device)."""
        return sdf_eval(self.decoder, _code(code, self.code_len), self.voxel_points)

    def extract_mesh_from_code(self, code, level=0.0):
        ctx = self.decoder.ctx
        c = _code(code, self.code_len)
        nv, nf = C.c_int(), C.c_int()
        ctx.check(ctx.lib.dsr_mesher_run(self._h, L.fptr(c), float(level), L.fptr(self._verts),
                                         self._verts.shape[0], L.iptr(self._faces), self._faces.shape[0],
                                         C.byref(nv), C.byref(nf)), "dsr_mesher_run")
        return ForceKeyErrorDict(vertices=self._verts[:nv.value].copy(), faces=self._faces[:nf.value].copy())

    def extract_meshes_from_codes(self, codes, level=0.0):
        """The meshes of several codes from one call (dsr_mesher_run_batch): one lite decode of
        all grids settles the sign away from the surface, exact tiles cover the band, marching
        cubes runs over all of them at once.  Each mesh is bitwise the one
        ``extract_mesh_from_code`` gives.  The output buffers grow to what a call needed (one
        retry after a -5), not to the worst case times the number of codes."""
        n = len(codes)
        if n == 0:
            return []
        ctx = self.decoder.ctx
        cs = np.ascontiguousarray(np.stack([_code(c, self.code_len) for c in codes]), np.float32)
        voff = np.zeros(n + 1, np.int32)
        foff = np.zeros(n + 1, np.int32)
        bv, bf = getattr(self, "_bverts", None), getattr(self, "_bfaces", None)
        if bv is None:
            d = self.voxels_dim                       # a first guess: a closed surface of ~d^2 cells per code
            bv = np.zeros((max(1024, 8 * d * d * n), 3), np.float32)
            bf = np.zeros((max(2048, 16 * d * d * n), 3), np.int32)
        for attempt in range(2):
            rc = ctx.lib.dsr_mesher_run_batch(self._h, n, L.fptr(cs), float(level), L.fptr(bv), bv.shape[0],
                                              L.iptr(bf), bf.shape[0], L.iptr(voff), L.iptr(foff))
            if rc != -5 or attempt == 1:
                break
            bv = np.zeros((max(int(voff[n]), bv.shape[0]), 3), np.float32)
            bf = np.zeros((max(int(foff[n]), bf.shape[0]), 3), np.int32)
        self._bverts, self._bfaces = bv, bf
        ctx.check(rc, "dsr_mesher_run_batch")
        return [ForceKeyErrorDict(vertices=bv[voff[i]:voff[i + 1]].copy(), faces=bf[foff[i]:foff[i + 1]].copy())
                for i in range(n)]

    def stats(self):
        """dsr_mesher_stats of the last ``extract_meshes_from_codes`` call, as a dict."""
        st = L.MesherStats()
        rc = self.decoder.ctx.lib.dsr_mesher_stats_get(self._h, C.byref(st))
        if rc != 0:
            raise L.DsrError(f"dsr_mesher_stats_get failed ({rc})")
        return {k: getattr(st, k) for k, _ in L.MesherStats._fields_}

    def peek(self, slot):
        """Diagnostic (dsr_mesher_peek): the lite volume, the merged volume and the 64-point tile
        flags (1 needed, 2 audit) of one slot of the last pass."""
        ctx = self.decoder.ctx
        n = self.voxels_dim ** 3
        lite, final = np.zeros(n, np.float32), np.zeros(n, np.float32)
        flags = np.zeros((n + 63) // 64, np.uint8)
        ctx.check(ctx.lib.dsr_mesher_peek(self._h, int(slot), L.fptr(lite), L.fptr(final),
                                          flags.ctypes.data_as(C.POINTER(C.c_ubyte))), "dsr_mesher_peek")
        return lite, final, flags


class SdfRenderer(object):
    """Depth, instance and normal images of reconstructed objects, sphere-traced over the decoder
    on device (dsr_renderer_*).  Replaces the reference's mesh + OpenGL path
    (ObjectRenderer::SetupCamera / Render, src/ObjectRenderer.cc:82-125) without a mesh: the
    camera is a zero-skew pinhole, pixel (u, v) has the ray ((u-cx)/fx, (v-cy)/fy, 1), depth is
    z-depth (``get_rays``, loss_utils.py:23-37)."""

    def __init__(self, decoder, width, height, fx, fy, cx, cy, code_len=64):
        self.decoder = decoder
        self.code_len = code_len
        self.width, self.height = int(width), int(height)
        ctx = decoder.ctx
        if not hasattr(ctx.lib, "dsr_renderer_create"):
            raise L.DsrError("this libdsr was built without dsr_renderer_* (no fallback)")
        cam = L.Camera(self.width, self.height, float(fx), float(fy), float(cx), float(cy))
        h = C.c_void_p()
        ctx.check(ctx.lib.dsr_renderer_create(ctx.handle, decoder.handle, C.byref(cam), C.byref(h)),
                  "dsr_renderer_create")
        self._h = h

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                self.decoder.ctx.lib.dsr_renderer_destroy(h)
            except Exception:
                pass
        self._h = None

    def __del__(self):
        self.close()

    def render(self, objects, normals=False, **params):
        """``objects``: a list of ``(t_cam_obj (4,4), code)``.  ``params``: hit_eps, max_steps, damp,
        near (unset or 0 = the defaults 1e-4, 48, 1, 0.01).  Returns depth (H,W) f32 (0 = nothing
        hit), instance (H,W) i32 (index into ``objects``, -1 = nothing hit), normals (H,W,3) f32 in
        the camera frame or None, and ``objects``: per object its status (0 rendered, 1 off-screen,
        2 skipped at the near plane), rect (u_min, v_min, u_max, v_max), n_rays, n_ball, n_hit,
        n_unconverged and n_visible."""
        if self._h is None:
            raise L.DsrError("renderer is closed")
        unknown = set(params) - {"hit_eps", "max_steps", "damp", "near"}
        if unknown:
            raise TypeError(f"unknown render parameters: {sorted(unknown)}")
        ctx = self.decoder.ctx
        n = len(objects)
        p = L.RenderParams(float(params.get("hit_eps", 0.0)), int(params.get("max_steps", 0)),
                           float(params.get("damp", 0.0)), float(params.get("near", 0.0)), int(bool(normals)))
        ins = (L.RenderObject * max(n, 1))()
        keep = []
        for i, (t, code) in enumerate(objects):
            t = np.ascontiguousarray(np.asarray(t, np.float32).reshape(16))
            c = _code(code, self.code_len)
            keep.append(c)
            ins[i].t_cam_obj[:] = t.tolist()
            ins[i].code = L.fptr(c)
        outs = (L.RenderObjectOut * max(n, 1))()
        depth = np.zeros((self.height, self.width), np.float32)
        inst = np.zeros((self.height, self.width), np.int32)
        nrm = np.zeros((self.height, self.width, 3), np.float32) if normals else None
        ctx.check(ctx.lib.dsr_renderer_render(self._h, C.byref(p), n, ins, L.fptr(depth), L.iptr(inst),
                                              L.fptr(nrm), outs), "dsr_renderer_render")
        recs = [ForceKeyErrorDict(status=o.status, rect=tuple(o.rect), n_rays=o.n_rays, n_ball=o.n_ball,
                                  n_hit=o.n_hit, n_unconverged=o.n_unconverged, n_visible=o.n_visible)
                for o in outs[:n]]
        return ForceKeyErrorDict(depth=depth, instance=inst, normals=nrm, objects=recs)

    def stats(self):
        """dsr_render_stats of the last ``render`` call, as a dict."""
        st = L.RenderStats()
        rc = self.decoder.ctx.lib.dsr_renderer_stats_get(self._h, C.byref(st))
        if rc != 0:
            raise L.DsrError(f"dsr_renderer_stats_get failed ({rc})")
        return {k: getattr(st, k) for k, _ in L.RenderStats._fields_}


def _scene_objects(objects, code_len):
    """[(t_world_obj (4,4), code or None), ...] -> (SceneObject array, the arrays it points into)"""
    ins = (L.SceneObject * max(len(objects), 1))()
    keep = []
    for i, (t, code) in enumerate(objects):
        t = np.ascontiguousarray(np.asarray(t, np.float32).reshape(16))
        ins[i].t_world_obj[:] = t.tolist()
        if code is not None:
            c = _code(code, code_len)
            keep.append(c)
            ins[i].code = L.fptr(c)
    return ins, keep


def scene_bin(objects, pts_world, i):
    """The binning rule of ``SceneSdf.query`` on the host (dsr_scene_bin_host; no device): the
    indices of the points inside object ``i``'s unit ball, in point order, their object-frame
    coordinates and the object's scale s — the inside test of MapObject::compute_sdf_loss
    (src/MapObject_util.cc:9-69) made exact.  ``objects``: ``[(t_world_obj (4,4), code), ...]``
    (the codes are not read)."""
    lib = L.load_library()
    if not hasattr(lib, "dsr_scene_bin_host"):
        raise L.DsrError("this libdsr was built without dsr_scene_* (no fallback)")
    pts = _f32(pts_world, 3)
    ins, _ = _scene_objects([(t, None) for t, _ in objects], 0)
    n = pts.shape[0]
    idx = np.zeros(n, np.int32)
    x = np.zeros((n, 3), np.float32)
    cnt, s = C.c_int(), C.c_float()
    rc = lib.dsr_scene_bin_host(len(objects), ins, n, L.fptr(pts), int(i), n, L.iptr(idx), L.fptr(x),
                                C.cast(C.byref(cnt), L.IP), C.cast(C.byref(s), L.FP))
    if rc != 0:
        raise L.DsrError(f"dsr_scene_bin_host failed ({rc}): bad argument or pose")
    return idx[:cnt.value].copy(), x[:cnt.value].copy(), float(s.value)


class SceneSdf(object):
    """World points against every object of a map at once, on device (dsr_scene_*; DESIGN.md
    §3.6c).  Replaces the per-object loop of MapObject::compute_sdf_loss /
    compute_sdf_loss_of_all_inside_points (src/MapObject_util.cc:9-69) over
    ``Optimizer.compute_sdf_loss_objectpoint_zhjd`` (reconstruct/optimizer.py:207-213) and the
    per-vertex collision check of the planner (src/NbvGenerator.cpp:320-327): the objects' poses
    and folded codes stay resident, a query uploads the points once."""

    def __init__(self, decoder, max_obj, max_pts, code_len=64):
        self.decoder = decoder
        self.code_len = code_len
        self.max_obj, self.max_pts = int(max_obj), int(max_pts)
        self._n_obj = 0
        ctx = decoder.ctx
        if not hasattr(ctx.lib, "dsr_scene_create"):
            raise L.DsrError("this libdsr was built without dsr_scene_* (no fallback)")
        h = C.c_void_p()
        ctx.check(ctx.lib.dsr_scene_create(ctx.handle, decoder.handle, self.max_obj, self.max_pts, C.byref(h)),
                  "dsr_scene_create")
        self._h = h

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                self.decoder.ctx.lib.dsr_scene_destroy(h)
            except Exception:
                pass
        self._h = None

    def __del__(self):
        self.close()

    def _handle(self):
        if self._h is None:
            raise L.DsrError("scene is closed")
        return self._h

    def set_objects(self, objects):
        """``objects``: a list of ``(t_world_obj (4,4), code)`` — MapObject::Sim3Two and vShapeCode.
        The codes are folded on device here, once."""
        ctx = self.decoder.ctx
        ins, keep = _scene_objects(objects, self.code_len)
        ctx.check(ctx.lib.dsr_scene_set_objects(self._handle(), len(objects), ins), "dsr_scene_set_objects")
        self._n_obj = len(objects)

    def query(self, pts_world, grad=False):
        """``pts_world`` (n,3).  Returns dist (n,) f32 (the smallest s_i f_i over the balls that hold
        the point, +inf in no ball), obj (n,) i32 (its object, -1 in no ball; ties go to the lower
        index), grad (n,3) f32 (the world-frame gradient of dist, 0 where nothing won) or None, and
        ``objects``: per object n_in, n_win, n_neg, n_nan, sum_sdf, sum_abs and mean_sdf = sum_sdf /
        n_in — compute_sdf_loss_objectpoint_zhjd on the points inside its ball (NaN when empty)."""
        ctx = self.decoder.ctx
        pts = _f32(pts_world, 3)
        n = pts.shape[0]
        dist = np.zeros(n, np.float32)
        obj = np.zeros(n, np.int32)
        g = np.zeros((n, 3), np.float32) if grad else None
        outs = (L.SceneObjectOut * max(self._n_obj, 1))()
        ctx.check(ctx.lib.dsr_scene_query(self._handle(), n, L.fptr(pts), L.fptr(dist), L.iptr(obj), L.fptr(g), outs),
                  "dsr_scene_query")
        recs = [ForceKeyErrorDict(n_in=o.n_in, n_win=o.n_win, n_neg=o.n_neg, n_nan=o.n_nan, sum_sdf=o.sum_sdf,
                                  sum_abs=o.sum_abs, mean_sdf=o.sum_sdf / o.n_in if o.n_in else float("nan"))
                for o in outs[:self._n_obj]]
        return ForceKeyErrorDict(dist=dist, obj=obj, grad=g, objects=recs)

    def peek(self, i):
        """Diagnostic (dsr_scene_peek): object ``i``'s candidates of the last query in point order —
        their point indices, object-frame coordinates and decoded f."""
        ctx = self.decoder.ctx
        n = C.c_int()
        rc = ctx.lib.dsr_scene_peek(self._handle(), int(i), 0, None, None, None, C.cast(C.byref(n), L.IP))
        if rc not in (0, -5):
            ctx.check(rc, "dsr_scene_peek")
        cnt = n.value
        idx = np.zeros(cnt, np.int32)
        x = np.zeros((cnt, 3), np.float32)
        sdf = np.zeros(cnt, np.float32)
        if cnt:
            ctx.check(ctx.lib.dsr_scene_peek(self._handle(), int(i), cnt, L.iptr(idx), L.fptr(x), L.fptr(sdf),
                                             C.cast(C.byref(n), L.IP)), "dsr_scene_peek")
        return idx, x, sdf

    def _associated(self, n_det, outs, table):
        from reconstruct import utils as U

        t = table.reshape(3, n_det, self._n_obj)
        return ForceKeyErrorDict(records=[U.assoc_record(outs[j]) for j in range(n_det)], n_in=t[0].copy(),
                                 n_hit=t[1].copy(), n_neg=t[2].copy())

    def associate_frame(self, depth, instance, labels, camera, t_world_cam, **params):
        """Which of a frame's detections are map objects already seen (dsr_scene_associate_frame;
        DESIGN.md §3.6d) — Tracking::AssociateObjectsByProjection_onlyformono
        (src/Tracking_util.cc:210-288) with the depth under each mask as the evidence.  ``labels``:
        each detection's value in ``instance``; ``camera``: see ``utils.frame_camera``;
        ``t_world_cam`` (4,4) rigid; ``params``: ``max_pts``, ``min_mask_area``, ``near``, ``far`` of the
        ingest and ``inlier_tol``, ``min_hits``, ``min_pct`` of the decision.  Returns
        ``dict(records=[...], n_in=, n_hit=, n_neg=)``: per detection its record
        (``utils.assoc_record``) and the three (n_det, n_obj) int32 vote tables."""
        from reconstruct import utils as U

        ctx = self.decoder.ctx
        if not hasattr(ctx.lib, "dsr_scene_associate_frame"):
            raise L.DsrError("this libdsr was built without dsr_scene_associate_* (no fallback)")
        fp, ap = U.assoc_split_params(params)
        cam = U.frame_camera(camera)
        depth, instance = U.frame_images(depth, instance, cam)
        lab = np.ascontiguousarray(np.asarray(labels, np.int32).reshape(-1))
        n = lab.shape[0]
        t = np.ascontiguousarray(np.asarray(t_world_cam, np.float32).reshape(16))
        outs = (L.AssocOut * max(n, 1))()
        table = np.zeros(3 * n * self._n_obj, np.int32)
        ctx.check(ctx.lib.dsr_scene_associate_frame(self._handle(), cam, fp, ap, L.fptr(t), L.fptr(depth),
                                                    L.iptr(instance), n, L.iptr(lab), outs, L.iptr(table)),
                  "dsr_scene_associate_frame")
        return self._associated(n, outs, table)

    def associate_points(self, rows, t_world_cam=None, **params):
        """The same for rows the caller holds (dsr_scene_associate_points), e.g. the LiDAR path's
        from ``utils.lidar_inputs``.  ``rows``: per detection an (n_j, 3) array of camera-frame
        points (an empty one is a detection without points); ``t_world_cam`` None: the rows are
        world points already; ``params``: ``inlier_tol``, ``min_hits``, ``min_pct`` and ``max_pts``,
        the stride of the detections in the scene's point buffer (default: the longest detection)."""
        from reconstruct import utils as U

        ctx = self.decoder.ctx
        if not hasattr(ctx.lib, "dsr_scene_associate_points"):
            raise L.DsrError("this libdsr was built without dsr_scene_associate_* (no fallback)")
        params = dict(params)
        max_pts = params.pop("max_pts", None)
        fp, ap = U.assoc_split_params(params)
        arrays = [_f32(r, 3) for r in rows]
        n = len(arrays)
        if max_pts is None:
            max_pts = max([a.shape[0] for a in arrays] + [1])
        max_pts = int(max_pts)
        n_rows = np.asarray([a.shape[0] for a in arrays], np.int32).reshape(-1)
        packed = np.zeros((max(n, 1), max(max_pts, 1), 3), np.float32)
        for j, a in enumerate(arrays):
            packed[j, :min(a.shape[0], max(max_pts, 0))] = a[:max(max_pts, 0)]
        t = None if t_world_cam is None else np.ascontiguousarray(np.asarray(t_world_cam, np.float32).reshape(16))
        outs = (L.AssocOut * max(n, 1))()
        table = np.zeros(3 * n * self._n_obj, np.int32)
        ctx.check(ctx.lib.dsr_scene_associate_points(self._handle(), ap, L.fptr(t), n, max_pts, L.iptr(n_rows),
                                                     L.fptr(packed), outs, L.iptr(table)),
                  "dsr_scene_associate_points")
        return self._associated(n, outs, table)

    def stats(self):
        """dsr_scene_stats of the last ``query`` or ``associate_*`` call, as a dict."""
        st = L.SceneStats()
        rc = self.decoder.ctx.lib.dsr_scene_stats_get(self._handle(), C.byref(st))
        if rc != 0:
            raise L.DsrError(f"dsr_scene_stats_get failed ({rc})")
        return {k: getattr(st, k) for k, _ in L.SceneStats._fields_}
