"""``reconstruct/utils.py`` of the reference, every public name (utils.py:26-161).

Same names and behaviour the C++ side relies on (src/System.cc:95-98):
``get_configs(path)`` returns an attribute dict that raises ``KeyError`` on a
missing key (``ForceKeyErrorDict``, utils.py:82-90), ``get_decoder(cfg)`` returns
the decoder handle built from ``cfg.DeepSDF_DIR`` (utils.py:93-94).  The mesher half
(``create_voxel_grid``, ``convert_sdf_voxels_to_mesh``, ``write_mesh_to_ply``) and the
viewer helpers the reference's scripts import (``color_table``, ``set_view``:
reconstruct_frame.py:20, visualize_map.py:22) keep their names too.
"""
from __future__ import annotations

import json

import numpy as np


# the reference's visualisation palette (utils.py:26-37), RGB in [0, 1]: red, green, blue,
# magenta, orange, purple, cyan, lime, pink, teal
color_table = [[r / 255., g / 255., b / 255.] for r, g, b in (
    (230, 0, 0), (60, 180, 75), (0, 0, 255), (255, 0, 255), (255, 165, 0),
    (128, 0, 128), (0, 255, 255), (210, 245, 60), (250, 190, 190), (0, 128, 128))]


def set_view(vis, dist=100., theta=np.pi / 6.):
    """utils.py:40-55: point an Open3D visualiser's camera at the world origin from `dist`
    along its z axis, tilted by `theta` about x (world -> eye extrinsic).  Needs only the
    visualiser object the caller passes (no open3d import here)."""
    ctl = vis.get_view_control()
    cam = ctl.convert_to_pinhole_camera_parameters()
    c, s = np.cos(theta), np.sin(theta)
    cam.extrinsic = np.array([[1., 0., 0., 0.],
                              [0., c, -s, 0.],
                              [0., s, c, dist],
                              [0., 0., 0., 1.]])
    ctl.convert_from_pinhole_camera_parameters(cam)


class ForceKeyErrorDict(dict):
    """addict.Dict-like attribute dict whose missing keys raise KeyError (utils.py:82-84)."""

    def __init__(self, *args, **kwargs):
        super().__init__()
        for k, v in dict(*args, **kwargs).items():
            self[k] = self._conv(v)

    @classmethod
    def _conv(cls, v):
        if isinstance(v, dict) and not isinstance(v, ForceKeyErrorDict):
            return cls(v)
        if isinstance(v, list):
            return [cls._conv(x) for x in v]
        return v

    def __getattr__(self, k):
        if k.startswith("__") and k.endswith("__"):
            raise AttributeError(k)
        try:
            return self[k]
        except KeyError:
            raise KeyError(k) from None

    def __setattr__(self, k, v):
        self[k] = self._conv(v)

    def __missing__(self, key):
        raise KeyError(key)


def read_calib_file(filepath):
    """utils.py:58-73: a KITTI calibration file as {key: float64 array}; parsing stops at the
    first empty line and keys whose values are not all numbers (dates) are skipped.  Used by
    the reference's kitti_sequence.py (data ingest, kept by the C++ caller)."""
    data = {}
    with open(filepath, "r") as f:
        for line in f.readlines():
            if line == "\n":
                break
            key, value = line.split(":", 1)
            try:
                data[key] = np.array([float(x) for x in value.split()])
            except ValueError:
                pass
    return data


def load_velo_scan(file):
    """utils.py:76-79: a velodyne .bin scan as an (N, 4) float32 array (x, y, z, reflectance)."""
    return np.fromfile(file, dtype=np.float32).reshape((-1, 4))


def get_configs(cfg_file):
    """utils.py:87-90."""
    with open(cfg_file) as f:
        cfg_dict = json.load(f)
    return ForceKeyErrorDict(**cfg_dict)


def get_decoder(configs, device=None):
    """utils.py:93-94: ``config_decoder(configs.DeepSDF_DIR)`` -> device decoder handle."""
    from deep_sdf.workspace import config_decoder

    return config_decoder(configs.DeepSDF_DIR, device=device)


def views_from_world(t_cam_world_list):
    """The ``t_view_ref`` of ``Optimizer.reconstruct_objects_views`` from what a SLAM caller holds
    per keyframe: world -> camera poses ``T_cv_w`` (SE(3), 4x4).  Keyframe 0 is the reference
    view; ``t_view_ref_v = T_cv_w @ inverse(T_c0_w)`` in float64 (the identity, exactly, for
    v = 0).  No reference counterpart (the reference fits one camera at a time)."""
    ts = [np.asarray(t, np.float64).reshape(4, 4) for t in t_cam_world_list]
    if not ts:
        return []
    inv0 = np.eye(4)
    inv0[:3, :3] = ts[0][:3, :3].T
    inv0[:3, 3] = -ts[0][:3, :3].T @ ts[0][:3, 3]
    return [np.eye(4)] + [t @ inv0 for t in ts[1:]]


FRAME_PARAM_NAMES = ("max_pts", "max_bg", "downsample", "expand", "min_mask_area", "near", "far")


def frame_params(**params):
    """``dsr_frame_params``: the library's defaults (dsr_frame_params_default: max_pts 250, max_bg
    200, downsample 4, expand 5, min_mask_area 1000, near 0.01, far +inf) with ``params`` on top."""
    from reconstruct import _libdsr as L

    unknown = set(params) - set(FRAME_PARAM_NAMES)
    if unknown:
        raise TypeError(f"unknown frame parameters: {sorted(unknown)}")
    p = L.FrameParams()
    if L.load_library().dsr_frame_params_default(p) != 0:
        raise L.DsrError("dsr_frame_params_default failed")
    for k, v in params.items():
        setattr(p, k, float(v) if k in ("near", "far") else int(v))
    return p


def frame_camera(camera):
    """``dsr_camera`` from a ``_libdsr.Camera``, a dict or an object with width, height, fx, fy, cx,
    cy, or that 6-tuple."""
    from reconstruct import _libdsr as L

    if isinstance(camera, L.Camera):
        return camera
    names = ("width", "height", "fx", "fy", "cx", "cy")
    if isinstance(camera, dict):
        v = [camera[k] for k in names]
    elif hasattr(camera, "fx"):
        v = [getattr(camera, k) for k in names]
    else:
        v = list(camera)
    return L.Camera(int(v[0]), int(v[1]), float(v[2]), float(v[3]), float(v[4]), float(v[5]))


def frame_dets(detections, code_len=64):
    """The ``dsr_frame_det`` array of a list of detection dicts ``{label, t_cam_obj, code=None,
    bbox=None, reconstructed=True}`` (``reconstructed`` is the caller's business), and the arrays
    it points into."""
    from reconstruct import _libdsr as L

    n = len(detections)
    dets = (L.FrameDet * max(n, 1))()
    keep = []
    for i, det in enumerate(detections):
        dets[i].label = int(det["label"])
        bbox = det.get("bbox")
        dets[i].bbox[:] = [0, 0, -1, -1] if bbox is None else [int(x) for x in bbox]
        dets[i].t_cam_obj[:] = np.asarray(det["t_cam_obj"], np.float32).reshape(16).tolist()
        code = det.get("code")
        if code is not None:
            c = np.ascontiguousarray(np.asarray(code, np.float32).reshape(-1)[:code_len])
            if c.shape[0] != code_len:
                raise ValueError(f"code must hold at least {code_len} values, got {c.shape[0]}")
            keep.append(c)
            dets[i].code = L.fptr(c)
        dets[i].pose_is_obj_cam = 0
    return dets, keep


def frame_record(o):
    """A ``dsr_frame_det_out`` as a dict."""
    return ForceKeyErrorDict(status=int(o.status), n_mask=int(o.n_mask), n_valid=int(o.n_valid),
                             n_pts=int(o.n_pts), n_bg=int(o.n_bg), box=tuple(o.box), grid_h=int(o.grid_h),
                             grid_w=int(o.grid_w))


def frame_images(depth, instance, camera):
    """depth / instance as contiguous (height, width) float32 / int32 arrays of the camera's size."""
    depth = np.ascontiguousarray(np.asarray(depth), dtype=np.float32)
    instance = np.ascontiguousarray(np.asarray(instance), dtype=np.int32)
    shape = (camera.height, camera.width)
    if depth.shape != shape or instance.shape != shape:
        raise ValueError(f"depth {depth.shape} / instance {instance.shape} must be (height, width) = {shape}")
    return depth, instance


def _input_arrays(n, p):
    """Zeroed ``(n, max_pts, 3)`` points, ``(n, max_pts + max_bg, 3)`` rays and ``(n, max_pts)`` depths
    for the host ingest entry points to fill (at least one row, so that the pointers are real)."""
    mp, mr = max(p.max_pts, 0), max(p.max_pts, 0) + max(p.max_bg, 0)
    return [np.zeros((max(n, 1),) + tail, np.float32) for tail in ((mp, 3), (mr, 3), (mp,))]


def _object(t_cam_obj, arrays, i, n_pts, n_rays, code):
    """Detection ``i`` of the filled ``arrays`` as the tuple ``Optimizer.reconstruct_objects`` takes,
    trimmed to its counts."""
    pts, rays, dobs = arrays
    return (np.array(t_cam_obj, np.float32).reshape(4, 4), pts[i, :n_pts].copy(), rays[i, :n_rays].copy(),
            dobs[i, :n_pts].copy(), None if code is None else np.asarray(code, np.float32))


def frame_inputs(depth, instance, detections, camera, **params):
    """What the reference builds per detection on the CPU — ``FrameWithLiDAR.get_detections`` +
    ``pixels_sampler`` (kitti_sequence.py:70-92, :139-146, :200-210), ``Frame.pixels_sampler``
    (mono_sequence.py:51-73) and ``get_rays`` (loss_utils.py:23-37) — from a depth image and an
    instance-label image, by the exact rule of DESIGN.md §3.5b (``dsr_frame_inputs_host``: plain
    C++ on the host, no device).  ``detections``: dicts ``{label, t_cam_obj, code=None, bbox=None,
    reconstructed=True}``; ``camera``: see ``frame_camera``; ``params``: ``FRAME_PARAM_NAMES``.
    Returns ``(objects, records)``: per detection ``(t_cam_obj, pts, rays, depth, code)`` trimmed to
    its counts — the tuple ``Optimizer.reconstruct_objects`` takes — and its ingest record
    (``frame_record``).  A detection that is not ok has empty arrays."""
    from reconstruct import _libdsr as L

    lib = L.load_library()
    cam = frame_camera(camera)
    p = frame_params(**params)
    depth, instance = frame_images(depth, instance, cam)
    n = len(detections)
    dets, keep = frame_dets(detections)
    arrays = _input_arrays(n, p)
    out = (L.FrameDetOut * max(n, 1))()
    rc = lib.dsr_frame_inputs_host(cam, p, L.fptr(depth), L.iptr(instance), n, dets, *map(L.fptr, arrays), out)
    if rc != 0:
        raise L.DsrError(f"dsr_frame_inputs_host failed ({rc}): bad camera, image or frame parameters")
    records = [frame_record(out[i]) for i in range(n)]
    objects = [_object(det["t_cam_obj"], arrays, i, r.n_pts, r.n_pts + r.n_bg, det.get("code"))
               for i, (det, r) in enumerate(zip(detections, records))]
    return objects, records


FRAME_POSE_PARAM_NAMES = ("outlier_radius", "lo_pct", "hi_pct", "box_margin", "scale_factor", "min_points", "up")


def frame_pose_params(pose_params=None):
    """``dsr_frame_pose_params``: the reference's constants (dsr_frame_pose_params_default:
    outlier_radius 1.0, lo_pct 5, hi_pct 95, box_margin 1.2, scale_factor 0.40, min_points 50, up
    (0, -1, 0); MapObject.cc:278, :380, :387-388, :410, :437, LocalMapping_util.cc:333) with the
    dict ``pose_params`` on top; a ``_libdsr.FramePoseParams`` is passed through."""
    from reconstruct import _libdsr as L

    if isinstance(pose_params, L.FramePoseParams):
        return pose_params
    pose_params = dict(pose_params or {})
    unknown = set(pose_params) - set(FRAME_POSE_PARAM_NAMES)
    if unknown:
        raise TypeError(f"unknown frame pose parameters: {sorted(unknown)}")
    p = L.FramePoseParams()
    if L.load_library().dsr_frame_pose_params_default(p) != 0:
        raise L.DsrError("dsr_frame_pose_params_default failed")
    for k, v in pose_params.items():
        if k == "up":
            p.up[:] = [float(x) for x in v]
        else:
            setattr(p, k, int(v) if k in ("lo_pct", "hi_pct", "min_points") else float(v))
    return p


def frame_pose_modes(detections):
    """Per detection its pose mode (include/dsr.h DSR_FRAME_POSE_*): ``mode`` if the dict carries
    one, else given when it brings a ``t_cam_obj``, else cuboid."""
    from reconstruct import _libdsr as L

    return np.asarray([int(d["mode"]) if d.get("mode") is not None else
                       (L.FRAME_POSE_GIVEN if d.get("t_cam_obj") is not None else L.FRAME_POSE_CUBOID)
                       for d in detections], np.int32).reshape(-1)


def frame_pose_record(o):
    """A ``dsr_frame_pose_out`` as a dict."""
    return ForceKeyErrorDict(status=int(o.status), n_in=int(o.n_in), n_near=int(o.n_near), n_kept=int(o.n_kept),
                             dims=np.array(o.dims[:], np.float64), eig=np.array(o.eig[:], np.float64),
                             t_cam_obj=np.array(o.t_cam_obj[:], np.float32).reshape(4, 4))


def _with_pose(det):
    return det if det.get("t_cam_obj") is not None else dict(det, t_cam_obj=np.eye(4, dtype=np.float32))


def frame_poses(depth, instance, detections, camera, pose_params=None, **params):
    """``frame_inputs`` for detections that may come without a pose — the reference's mono / RGB-D
    call site (LocalMapping_util.cc:284-410): ``MapObject::RemoveOutliersSimple`` and
    ``ComputeCuboidPCA_onlyformono`` (MapObject.cc:249-283, :330-443) give the start pose and the
    points / rays that survive, by the exact rule of DESIGN.md §3.5c (``dsr_frame_poses_host``:
    plain C++ on the host, no device).  A detection without ``t_cam_obj`` (or with ``None``) gets
    the cuboid pose; ``mode`` (``_libdsr.FRAME_POSE_*``) overrides that, e.g. the flipped cuboid.
    ``pose_params``: a dict over ``FRAME_POSE_PARAM_NAMES`` (see ``frame_pose_params``).  Returns
    ``(objects, records, pose_records)``: objects as ``frame_inputs`` with the start pose and the
    kept rows, the ingest records, and the pose records (``frame_pose_record``).  A detection
    without a start pose has empty arrays and the identity."""
    from reconstruct import _libdsr as L

    lib = L.load_library()
    cam = frame_camera(camera)
    p = frame_params(**params)
    q = frame_pose_params(pose_params)
    depth, instance = frame_images(depth, instance, cam)
    n = len(detections)
    modes = frame_pose_modes(detections)
    dets, keep = frame_dets([_with_pose(d) for d in detections])
    arrays = _input_arrays(n, p)
    out = (L.FrameDetOut * max(n, 1))()
    pout = (L.FramePoseOut * max(n, 1))()
    rc = lib.dsr_frame_poses_host(cam, p, q, L.fptr(depth), L.iptr(instance), n, dets, L.iptr(modes),
                                  *map(L.fptr, arrays), out, pout)
    if rc != 0:
        raise L.DsrError(f"dsr_frame_poses_host failed ({rc}): bad camera, image, frame or pose parameters")
    objects, records, poses = [], [], []
    for i, det in enumerate(detections):
        r, pr = frame_record(out[i]), frame_pose_record(pout[i])
        if pr.status == L.FRAME_POSE_NOT_ASKED:
            n_p, n_r = r.n_pts, r.n_pts + r.n_bg
        elif pr.status == L.FRAME_POSE_OK:
            n_p, n_r = pr.n_kept, pr.n_kept + r.n_bg
        else:
            n_p = n_r = 0
        objects.append(_object(pr.t_cam_obj, arrays, i, n_p, n_r, det.get("code")))
        records.append(r)
        poses.append(pr)
    return objects, records, poses


LIDAR_PARAM_NAMES = ("max_pts", "max_bg", "downsample", "expand", "min_mask_area", "radius", "box_margin")


def lidar_params(**params):
    """``dsr_lidar_params``: the library's defaults (dsr_lidar_params_default: max_pts 250, max_bg
    200, downsample 4, expand 5, min_mask_area 1000, radius 3.0, box_margin 1.1) with ``params`` on
    top."""
    from reconstruct import _libdsr as L

    unknown = set(params) - set(LIDAR_PARAM_NAMES)
    if unknown:
        raise TypeError(f"unknown lidar parameters: {sorted(unknown)}")
    p = L.LidarParams()
    if L.load_library().dsr_lidar_params_default(p) != 0:
        raise L.DsrError("dsr_lidar_params_default failed")
    for k, v in params.items():
        setattr(p, k, float(v) if k in ("radius", "box_margin") else int(v))
    return p


def lidar_dets(detections, code_len=64):
    """The ``dsr_lidar_det`` array of a list of detections — dicts ``{trans, size = (w, l, h), theta,
    code=None}`` or rows ``(x, y, z, w, l, h, theta, ...)`` as the 3-D detector emits them
    (kitti_sequence.py:116) — and the arrays it points into."""
    from reconstruct import _libdsr as L

    n = len(detections)
    dets = (L.LidarDet * max(n, 1))()
    keep = []
    for i, det in enumerate(detections):
        if isinstance(det, dict):
            row = [*det["trans"], *det["size"], det["theta"]]
            code = det.get("code")
        else:
            row, code = list(det)[:7], None
        row = np.asarray(row, np.float32).reshape(7)
        dets[i].trans[:] = row[:3].tolist()
        dets[i].size[:] = row[3:6].tolist()
        dets[i].theta = float(row[6])
        if code is not None:
            c = np.ascontiguousarray(np.asarray(code, np.float32).reshape(-1)[:code_len])
            if c.shape[0] != code_len:
                raise ValueError(f"code must hold at least {code_len} values, got {c.shape[0]}")
            keep.append(c)
            dets[i].code = L.fptr(c)
    return dets, keep


def lidar_masks(masks):
    """The ``dsr_lidar_mask`` array of a list of masks: dicts ``{label, bbox=None}``, pairs
    ``(label, bbox)`` or bare labels (``bbox`` None: the mask's tight box)."""
    from reconstruct import _libdsr as L

    n = len(masks)
    out = (L.LidarMask * max(n, 1))()
    for i, m in enumerate(masks):
        if isinstance(m, dict):
            label, bbox = m["label"], m.get("bbox")
        elif isinstance(m, (tuple, list)):
            label, bbox = m
        else:
            label, bbox = m, None
        out[i].label = int(label)
        out[i].bbox[:] = [0, 0, -1, -1] if bbox is None else [int(x) for x in bbox]
    return out


def lidar_record(o):
    """A ``dsr_lidar_det_out`` as a dict; ``t_cam_obj`` as a tuple of its 16 row-major values, so
    that records compare with ``==``."""
    return ForceKeyErrorDict(status=int(o.status), n_near=int(o.n_near), n_crop=int(o.n_crop), n_pts=int(o.n_pts),
                             n_proj=int(o.n_proj), mask=int(o.mask), n_hits=int(o.n_hits),
                             n_mask_px=int(o.n_mask_px), n_bg=int(o.n_bg), box=tuple(o.box), grid_h=int(o.grid_h),
                             grid_w=int(o.grid_w), t_cam_obj=tuple(o.t_cam_obj))


def lidar_sweep(velo, instance, camera, t_cam_velo):
    """The sweep as a contiguous (n, stride >= 3) float32 array, the instance image as frame_images
    wants it and t_cam_velo as 16 float32."""
    velo = np.ascontiguousarray(np.asarray(velo), dtype=np.float32)
    if velo.ndim != 2 or velo.shape[1] < 3:
        raise ValueError(f"velo {velo.shape} must be (n, stride >= 3)")
    instance = np.ascontiguousarray(np.asarray(instance), dtype=np.int32)
    if instance.shape != (camera.height, camera.width):
        raise ValueError(f"instance {instance.shape} must be (height, width) = {(camera.height, camera.width)}")
    tcv = np.ascontiguousarray(np.asarray(t_cam_velo, np.float32).reshape(16))
    return velo, instance, tcv


def lidar_inputs(velo, instance, masks, detections, camera, t_cam_velo, **params):
    """What ``FrameWithLiDAR.get_detections`` builds per 3-D detection on the CPU
    (kitti_sequence.py:99-216, with ``pixels_sampler`` :70-92 and ``get_rays``,
    loss_utils.py:23-37) — from a Velodyne sweep ``velo`` (n, stride >= 3), an instance-label image
    and its mask list, by the exact rule of DESIGN.md §3.5d (``dsr_lidar_inputs_host``: plain C++
    on the host, no device).  ``masks``: see ``lidar_masks``; ``detections``: see ``lidar_dets``;
    ``camera``: see ``frame_camera``; ``t_cam_velo``: rigid 4x4; ``params``: ``LIDAR_PARAM_NAMES``.
    Returns ``(objects, records)`` shaped like ``frame_inputs``: per detection ``(t_cam_obj, pts,
    rays, depth, code)`` — the tuple ``Optimizer.reconstruct_objects`` takes — and its ingest record
    (``lidar_record``).  A detection that is not ok has empty arrays (the reference's ``rays =
    None``)."""
    from reconstruct import _libdsr as L

    lib = L.load_library()
    cam = frame_camera(camera)
    p = lidar_params(**params)
    velo, instance, tcv = lidar_sweep(velo, instance, cam, t_cam_velo)
    n = len(detections)
    dets, keep = lidar_dets(detections)
    ml = lidar_masks(masks)
    arrays = _input_arrays(n, p)
    out = (L.LidarDetOut * max(n, 1))()
    rc = lib.dsr_lidar_inputs_host(cam, p, L.fptr(tcv), L.fptr(velo), velo.shape[0], velo.shape[1], L.iptr(instance),
                                   len(masks), ml, n, dets, *map(L.fptr, arrays), out)
    if rc != 0:
        raise L.DsrError(f"dsr_lidar_inputs_host failed ({rc}): bad camera, sweep, masks, detections or lidar "
                         "parameters")
    objects, records = [], []
    for i, det in enumerate(detections):
        r = lidar_record(out[i])
        n_p, n_r = (r.n_pts, r.n_pts + r.n_bg) if r.status == L.LIDAR_OK else (0, 0)
        objects.append(_object(r.t_cam_obj, arrays, i, n_p, n_r, det.get("code") if isinstance(det, dict) else None))
        records.append(r)
    return objects, records


def lidar_track_prep(detections, t_cam_velo, **params):
    """The start poses of detections tracked from a sweep (``dsr_lidar_track_prep_host``: plain C++
    on the host, no device): per detection the SE(3) ``t_co_se3`` (n, 4, 4) =
    t_cam_velo [R | o] and ``det_scale`` (n,) = box_margin l / 2 — ObjectDetection's decomposition of
    the ingest's t_cam_obj (src/ObjectDetection.cc:29-37).  ``params``: ``box_margin``."""
    from reconstruct import _libdsr as L

    p = lidar_params(**params)
    tcv = np.ascontiguousarray(np.asarray(t_cam_velo, np.float32).reshape(16))
    n = len(detections)
    dets, keep = lidar_dets(detections)
    t = np.zeros((max(n, 1), 4, 4), np.float32)
    sc = np.zeros(max(n, 1), np.float32)
    rc = L.load_library().dsr_lidar_track_prep_host(p, L.fptr(tcv), n, dets, L.fptr(t), L.fptr(sc))
    if rc != 0:
        raise L.DsrError(f"dsr_lidar_track_prep_host failed ({rc}): bad detections, t_cam_velo or box_margin")
    return t[:n], sc[:n]


ASSOC_PARAM_NAMES = ("inlier_tol", "min_hits", "min_pct")
ASSOC_FRAME_PARAM_NAMES = ("max_pts", "min_mask_area", "near", "far")


def assoc_params(**params):
    """``dsr_assoc_params``: the library's defaults (dsr_assoc_params_default: inlier_tol 0.05,
    min_hits 20, min_pct 50) with ``params`` on top."""
    from reconstruct import _libdsr as L

    unknown = set(params) - set(ASSOC_PARAM_NAMES)
    if unknown:
        raise TypeError(f"unknown association parameters: {sorted(unknown)}")
    lib = L.load_library()
    if not hasattr(lib, "dsr_assoc_params_default"):
        raise L.DsrError("this libdsr was built without dsr_assoc_* (no fallback)")
    p = L.AssocParams()
    if lib.dsr_assoc_params_default(p) != 0:
        raise L.DsrError("dsr_assoc_params_default failed")
    for k, v in params.items():
        setattr(p, k, float(v) if k == "inlier_tol" else int(v))
    return p


def assoc_split_params(params):
    """``params`` of an association call -> (``dsr_frame_params`` of the ingest fields it reads,
    ``dsr_assoc_params``)."""
    unknown = set(params) - set(ASSOC_PARAM_NAMES) - set(ASSOC_FRAME_PARAM_NAMES)
    if unknown:
        raise TypeError(f"unknown association parameters: {sorted(unknown)}")
    return (frame_params(**{k: v for k, v in params.items() if k in ASSOC_FRAME_PARAM_NAMES}),
            assoc_params(**{k: v for k, v in params.items() if k in ASSOC_PARAM_NAMES}))


def assoc_record(o):
    """A ``dsr_assoc_out`` as a dict."""
    return ForceKeyErrorDict(status=int(o.status), n_pts=int(o.n_pts), obj=int(o.obj), n_hit=int(o.n_hit),
                             n_in=int(o.n_in), n_neg=int(o.n_neg), second=int(o.second),
                             second_hit=int(o.second_hit), ingest_status=int(o.ingest_status), n_mask=int(o.n_mask),
                             n_valid=int(o.n_valid))


def assoc_points(depth, instance, labels, camera, t_world_cam, **params):
    """The points ``SceneSdf.associate_frame`` queries, on the host (``dsr_assoc_points_host``: plain
    C++, no device): every label's surface-point rows of the depth image moved to
    the world by ``t_world_cam``, at the fixed stride ``max_pts`` with NaN beyond a detection's
    count — the evidence that stands in for the map points of src/Tracking_util.cc:210-288.
    ``params``: ``max_pts``, ``min_mask_area``, ``near``, ``far``.  Returns ``(pts_world (n_det,
    max_pts, 3), n_rows (n_det,), records)`` with the ingest records of ``frame_record``."""
    from reconstruct import _libdsr as L

    lib = L.load_library()
    if not hasattr(lib, "dsr_assoc_points_host"):
        raise L.DsrError("this libdsr was built without dsr_assoc_* (no fallback)")
    unknown = set(params) - set(ASSOC_FRAME_PARAM_NAMES)
    if unknown:
        raise TypeError(f"unknown association frame parameters: {sorted(unknown)}")
    p = frame_params(**params)
    cam = frame_camera(camera)
    depth, instance = frame_images(depth, instance, cam)
    lab = np.ascontiguousarray(np.asarray(labels, np.int32).reshape(-1))
    n = lab.shape[0]
    t = np.ascontiguousarray(np.asarray(t_world_cam, np.float32).reshape(16))
    pts = np.zeros((max(n, 1), max(p.max_pts, 1), 3), np.float32)
    n_rows = np.zeros(max(n, 1), np.int32)
    out = (L.FrameDetOut * max(n, 1))()
    rc = lib.dsr_assoc_points_host(cam, p, L.fptr(t), L.fptr(depth), L.iptr(instance), n, L.iptr(lab), L.fptr(pts),
                                   L.iptr(n_rows), out)
    if rc != 0:
        raise L.DsrError(f"dsr_assoc_points_host failed ({rc}): bad camera, image, labels, frame parameters or "
                         "t_world_cam")
    return pts[:n], n_rows[:n], [frame_record(out[i]) for i in range(n)]


def assoc_pick(n_in, n_hit, n_neg, n_rows, **params):
    """The decision of ``SceneSdf.associate_*`` from the vote tables, on the host
    (``dsr_assoc_pick_host``; DESIGN.md §3.6d — the winner of the vote of
    src/Tracking_util.cc:210-288): ``n_in``, ``n_hit``, ``n_neg`` (n_det, n_obj) int32, ``n_rows``
    (n_det,) the detections' row counts; ``params``: ``ASSOC_PARAM_NAMES``.  Returns the records."""
    from reconstruct import _libdsr as L

    lib = L.load_library()
    if not hasattr(lib, "dsr_assoc_pick_host"):
        raise L.DsrError("this libdsr was built without dsr_assoc_* (no fallback)")
    p = assoc_params(**params)
    n_rows = np.ascontiguousarray(np.asarray(n_rows, np.int32).reshape(-1))
    n = n_rows.shape[0]
    tabs = [np.asarray(t, np.int32) for t in (n_in, n_hit, n_neg)]
    n_obj = tabs[0].shape[1] if tabs[0].ndim == 2 else -1
    if any(t.shape != (n, n_obj) for t in tabs):
        raise ValueError("n_in, n_hit and n_neg must share the shape (n_det, n_obj)")
    table = np.ascontiguousarray(np.stack(tabs)).reshape(-1)
    out = (L.AssocOut * max(n, 1))()
    rc = lib.dsr_assoc_pick_host(p, n, n_obj, L.iptr(table) if table.size else None, L.iptr(n_rows), out)
    if rc != 0:
        raise L.DsrError(f"dsr_assoc_pick_host failed ({rc}): bad parameters, tables or counts")
    return [assoc_record(out[i]) for i in range(n)]


def create_voxel_grid(vol_dim=128):
    """utils.py:97-116.  Note the reference's ``LongTensor / vol_dim`` is TRUE division
    in torch >= 1.6 (fp32), so its x/y columns are not integer lattice indices; this
    restates that fp32 arithmetic exactly (verified against torch in the tests)."""
    voxel_origin = [-1, -1, -1]
    voxel_size = 2.0 / (vol_dim - 1)
    idx = np.arange(vol_dim ** 3, dtype=np.int64)
    fidx = idx.astype(np.float32)
    fv = np.float32(vol_dim)
    values = np.zeros((vol_dim ** 3, 3), np.float32)
    values[:, 2] = idx % vol_dim
    values[:, 1] = np.remainder(fidx / fv, fv)
    values[:, 0] = np.remainder((fidx / fv) / fv, fv)
    values[:, 0] = values[:, 0] * np.float32(voxel_size) + np.float32(voxel_origin[2])
    values[:, 1] = values[:, 1] * np.float32(voxel_size) + np.float32(voxel_origin[1])
    values[:, 2] = values[:, 2] * np.float32(voxel_size) + np.float32(voxel_origin[0])
    return values


def convert_sdf_voxels_to_mesh(pytorch_3d_sdf_tensor, level=0.0, device=None):
    """utils.py:119-140 on device (``dsr_mc_volume``): marching cubes of an (n, n, n) SDF
    volume (torch tensor or array, C order — the grid order of ``create_voxel_grid``), vertices
    as voxel index x 2/(n-1) - 1 (the reference's spacing and origin shift), faces as vertex
    indices.  Returns (vertices float32 (V, 3), faces int32 (F, 3)) — float32 because the
    build's only caller, ``MeshExtractor``, casts to it anyway (optimizer.py:228).  The
    triangulation is the build's marching cubes, not skimage's ``marching_cubes_lewiner``
    (absent here: parity unpinned)."""
    import ctypes as C

    from reconstruct import _libdsr as L

    t = pytorch_3d_sdf_tensor
    if hasattr(t, "detach"):
        t = t.detach().cpu().numpy()
    vol = np.ascontiguousarray(t, dtype=np.float32)
    if vol.ndim != 3 or len(set(vol.shape)) != 1:
        raise ValueError(f"expected an (n, n, n) volume, got shape {vol.shape}")
    d = vol.shape[0]
    ctx = L.Context.get(device)
    verts = np.zeros((3 * d ** 3, 3), np.float32)
    faces = np.zeros((5 * (d - 1) ** 3, 3), np.int32)
    nv, nf = C.c_int(), C.c_int()
    ctx.check(ctx.lib.dsr_mc_volume(ctx.handle, L.fptr(vol), d, float(level), L.fptr(verts), verts.shape[0],
                                    L.iptr(faces), faces.shape[0], C.byref(nv), C.byref(nf)), "dsr_mc_volume")
    return verts[:nv.value].copy(), faces[:nf.value].copy()


# PLY layout plyfile.PlyData([vertex(x,y,z f4), face(vertex_indices i4 x3)]).write() produces
# (utils.py:143-161): binary, native (little-endian) byte order, list counts as uchar.
_PLY_HEADER = ("ply\nformat binary_little_endian 1.0\nelement vertex {nv}\nproperty float x\n"
               "property float y\nproperty float z\nelement face {nf}\n"
               "property list uchar int vertex_indices\nend_header\n")


def write_mesh_to_ply(v, f, ply_filename_out):
    """utils.py:141-161 without plyfile: the same binary PLY."""
    v = np.ascontiguousarray(v, dtype="<f4").reshape(-1, 3)
    f = np.ascontiguousarray(f, dtype="<i4").reshape(-1, 3)
    rec = np.zeros(f.shape[0], dtype=[("n", "u1"), ("idx", "<i4", (3,))])
    rec["n"] = 3
    rec["idx"] = f
    with open(ply_filename_out, "wb") as fh:
        fh.write(_PLY_HEADER.format(nv=v.shape[0], nf=f.shape[0]).encode("ascii"))
        fh.write(v.tobytes())
        fh.write(rec.tobytes())


def read_mesh_ply(path):
    """Inverse of write_mesh_to_ply (triangle meshes in that layout only)."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").split("\n")
    nv = int(next(x for x in head if x.startswith("element vertex")).split()[-1])
    nf = int(next(x for x in head if x.startswith("element face")).split()[-1])
    v = np.frombuffer(data, dtype="<f4", count=3 * nv, offset=end).reshape(nv, 3)
    rec = np.frombuffer(data, dtype=[("n", "u1"), ("idx", "<i4", (3,))], count=nf, offset=end + 12 * nv)
    if nf and not np.all(rec["n"] == 3):
        raise ValueError("not a triangle mesh")
    return v.copy(), rec["idx"].copy()
