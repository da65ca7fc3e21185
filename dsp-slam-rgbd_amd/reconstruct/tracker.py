"""``reconstruct.tracker`` — the resident object tracker (dsr_tracker_*).

The reference tracks every detection that is associated with a map object by one call of
``Optimizer.estimate_pose_cam_obj`` (reconstruct/optimizer.py:46-87) per detection
(LocalMapping::GetNewObservations_onyforStereo, src/LocalMapping_util.cc:84-154).  An
``ObjectTracker`` does the whole loop in one asynchronous call: its device blocks and pinned
staging exist from its creation, the inlier filter and the tile table run on the device, and the
points come from host rows (``track``), straight from a Velodyne sweep (``track_lidar``) or
straight from a depth image and its instance labels (``track_frame``).  The poses are bitwise those
of ``Optimizer.estimate_pose_cam_obj_batch`` on the same rows.

There is no CPU fallback: without libdsr / a gfx950 device the constructor raises DsrError.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from reconstruct import _libdsr as L
from reconstruct.utils import ForceKeyErrorDict


def track_record(o):
    """A ``dsr_track_out`` as a dict."""
    return ForceKeyErrorDict(status=int(o.status), n_pts=int(o.n_pts), n_inliers=int(o.n_inliers),
                             n_near=int(o.n_near), n_crop=int(o.n_crop))


class ObjectTracker(object):
    """Pose-only GN of at most ``max_obj`` tracked objects x ``max_pts`` points per call, with the
    decoder and the pose-only settings of ``optimizer``."""

    def __init__(self, optimizer, max_obj, max_pts):
        self.optimizer = optimizer
        self.decoder = optimizer.decoder
        self.code_len = int(optimizer.code_len)
        self.max_obj, self.max_pts = int(max_obj), int(max_pts)
        self._n = 0
        self._h = None
        ctx = self.decoder.ctx
        if not hasattr(ctx.lib, "dsr_tracker_create"):
            raise L.DsrError("this libdsr was built without dsr_tracker_* (no fallback)")
        h = C.c_void_p()
        ctx.check(ctx.lib.dsr_tracker_create(ctx.handle, self.decoder.handle, C.byref(optimizer.params), self.max_obj,
                                             self.max_pts, C.byref(h)), "dsr_tracker_create")
        self._h = h

    def close(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                self.decoder.ctx.lib.dsr_tracker_destroy(h)
            except Exception:
                pass
        self._h = None

    def __del__(self):
        self.close()

    def _handle(self):
        if self._h is None:
            raise L.DsrError("tracker is closed")
        return self._h

    def fits(self, n_obj, n_pts):
        return n_obj <= self.max_obj and n_pts <= self.max_pts

    def track(self, objects):
        """``objects``: a list of ``(t_co_se3, scale, pts, code)`` as ``estimate_pose_cam_obj`` takes
        them (LocalMapping_util.cc:103-110).  Returns once the work is enqueued."""
        from reconstruct.optimizer import _code, _f32

        n = len(objects)
        keep = []
        ins = (L.PoseIn * max(n, 1))()
        for i, (t, scale, pts, code) in enumerate(objects):
            t = _f32(t).reshape(4, 4)
            pts = _f32(pts, 3)
            c = _code(code, self.code_len)
            keep += [pts, c]
            ins[i].t_co_se3[:] = t.reshape(-1).tolist()
            ins[i].scale = float(scale)
            ins[i].pts, ins[i].n_pts = L.fptr(pts), pts.shape[0]
            ins[i].code = L.fptr(c)
        ctx = self.decoder.ctx
        ctx.check(ctx.lib.dsr_tracker_track(self._handle(), n, ins), "dsr_tracker_track")
        self._n = n

    def track_lidar(self, velo, t_cam_velo, detections, priors, params=None):
        """Every detection's points are cropped from the sweep on the device (the rows of
        ``utils.lidar_inputs``; kitti_sequence.py:118-146).  ``detections``: ``utils.lidar_dets``
        input, each with the map object's ``code``; ``priors``: per detection a scale, or a pair
        ``(scale, t_co_se3)`` giving the start pose — without one it is ``utils.lidar_track_prep``'s
        (det->SE3Tco); ``params``: a dict of ``max_pts``, ``radius``, ``box_margin``."""
        from reconstruct import utils as U

        p = U.lidar_params(**(params or {}))
        velo = np.ascontiguousarray(np.asarray(velo), dtype=np.float32)
        if velo.ndim != 2 or velo.shape[1] < 3:
            raise ValueError(f"velo {velo.shape} must be (n, stride >= 3)")
        tcv = np.ascontiguousarray(np.asarray(t_cam_velo, np.float32).reshape(16))
        n = len(detections)
        if len(priors) != n:
            raise ValueError("one prior per detection")
        dets, keep = U.lidar_dets(detections, self.code_len)
        pri = (L.TrackDet * max(n, 1))()
        for i, pr in enumerate(priors):
            scale, pose = pr if isinstance(pr, (tuple, list)) else (pr, None)
            pri[i].scale = float(scale)
            pri[i].pose_given = 0 if pose is None else 1
            if pose is not None:
                pri[i].t_co_se3[:] = np.asarray(pose, np.float32).reshape(16).tolist()
        ctx = self.decoder.ctx
        ctx.check(ctx.lib.dsr_tracker_track_lidar(self._handle(), p, L.fptr(tcv), L.fptr(velo), velo.shape[0],
                                                  velo.shape[1], n, dets, pri), "dsr_tracker_track_lidar")
        self._n = n

    def track_frame(self, depth, instance, detections, priors, camera, params=None):
        """Every detection's points are its surface-point rows of the depth image, built on the
        device (the ``pts`` rows of ``utils.frame_inputs``) — the RGB-D path,
        which has no sweep.  ``detections``: dicts ``{label, code}``, the code the map object's;
        ``priors``: per detection a pair ``(scale, t_co_se3)``, the map object's scale and the start
        pose (Tcw Two, LocalMapping_util.cc:106 — there is no 3-D detector to take one from);
        ``camera``: see ``utils.frame_camera``; ``params``: a dict of ``max_pts``,
        ``min_mask_area``, ``near``, ``far``.  The records' ``n_near`` / ``n_crop`` hold the
        ingest's ``n_mask`` / ``n_valid``."""
        from reconstruct import utils as U
        from reconstruct.optimizer import _code

        n = len(detections)
        if len(priors) != n:
            raise ValueError("one prior per detection")
        pri = (L.TrackDet * max(n, 1))()
        for i, pr in enumerate(priors):
            scale, pose = pr if isinstance(pr, (tuple, list)) else (pr, None)
            if pose is None:
                raise ValueError("a frame call needs every prior's start pose: (scale, t_co_se3)")
            pri[i].scale = float(scale)
            pri[i].pose_given = 1
            pri[i].t_co_se3[:] = np.asarray(pose, np.float32).reshape(16).tolist()
        unknown = set(params or {}) - {"max_pts", "min_mask_area", "near", "far"}
        if unknown:
            raise TypeError(f"unknown frame tracking parameters: {sorted(unknown)}")
        p = U.frame_params(**(params or {}))
        cam = U.frame_camera(camera)
        depth, instance = U.frame_images(depth, instance, cam)
        dets = (L.FrameDet * max(n, 1))()
        keep = []
        for i, det in enumerate(detections):
            dets[i].label = int(det["label"])
            code = det.get("code")
            if code is not None:
                keep.append(_code(code, self.code_len))
                dets[i].code = L.fptr(keep[-1])
        ctx = self.decoder.ctx
        if not hasattr(ctx.lib, "dsr_tracker_track_frame"):
            raise L.DsrError("this libdsr was built without dsr_tracker_track_frame (no fallback)")
        ctx.check(ctx.lib.dsr_tracker_track_frame(self._handle(), cam, p, L.fptr(depth), L.iptr(instance), n, dets,
                                                  pri), "dsr_tracker_track_frame")
        self._n = n

    def query(self):
        """True once the last call has finished (never blocks)."""
        ctx = self.decoder.ctx
        rc = ctx.lib.dsr_tracker_query(self._handle())
        if rc < 0:
            ctx.check(rc, "dsr_tracker_query")
        return rc == 1

    def result(self):
        """Waits for the last call.  Returns ``(poses, records)``: the (4, 4) float32 t_cam_obj per
        object (NaN where the record's status is not ok) and the records as dicts
        (``track_record``)."""
        ctx = self.decoder.ctx
        n = self._n
        out = np.zeros((max(n, 1), 4, 4), np.float32)
        recs = (L.TrackOut * max(n, 1))()
        ctx.check(ctx.lib.dsr_tracker_download(self._handle(), L.fptr(out), recs), "dsr_tracker_download")
        return [out[i] for i in range(n)], [track_record(recs[i]) for i in range(n)]
