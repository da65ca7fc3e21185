"""F24: one synthetic KITTI keyframe through the REFERENCE's FrameWithLiDAR.get_detections
(reconstruct/kitti_sequence.py:99-216; CPU, build container only):

    python tests/golden/make_lidar_frame.py     # writes tests/golden/f24_lidar_frame.npz

The reference is imported in place through refshim (plus an empty ``cv2`` module and the
``np.bool`` alias it still uses); the frame object is made with ``object.__new__`` and given the
attributes ``get_detections`` reads, ``online=False``, and the two ``.lbl`` files are written with
``torch.save`` into a temporary directory.  The fixture holds data only: the inputs (sweep, image
masks and boxes, detector rows, camera, t_cam_velo) and the reference's recorded outputs per
instance.

The inputs are screened so that the comparison with the rule of DESIGN.md §3.5d is about
arithmetic, not about a decision sitting on an edge; another seed is drawn until the screen passes,
and the screen's margins are recorded in the file:

* no near-point within 1e-4 of a box or cube face;
* every n_crop such that np.linspace(0, N-1, n).astype(int32) equals the integer sel;
* no projected row within 1e-3 px of a pixel boundary;
* no hit count within 2 of the match threshold or of a tie.
"""
from __future__ import annotations

import functools
import math
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(REPO, "dsp-slam-rgbd_amd"))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import refshim  # noqa: E402
import lidar_cases as LC  # noqa: E402
import lidar_oracle as LO  # noqa: E402

W, H = 311, 94
CAM = dict(width=W, height=H, fx=180.0, fy=180.0, cx=155.5, cy=46.5)
PARAMS = dict(LO.DEFAULTS)
FACE_EPS, PIXEL_EPS, HIT_MARGIN = 1e-4, 1e-3, 2
f32 = np.float32


def load_kitti_sequence():
    """The reference's reconstruct.kitti_sequence, imported in place."""
    ref = refshim.load()
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))
    if not hasattr(np, "bool"):
        np.bool = bool
    mine = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "reconstruct" or k.startswith("reconstruct.")}
    sys.modules.update(ref.modules)
    sys.path.insert(0, refshim.REF)
    try:
        import reconstruct.kitti_sequence as ks
    finally:
        sys.path.remove(refshim.REF)
        for k in list(sys.modules):
            if k == "reconstruct" or k.startswith("reconstruct.") or k == "deep_sdf" or k.startswith("deep_sdf."):
                sys.modules.pop(k)
        sys.modules.update(mine)
    return ref, ks


def draw(seed):
    """Three cars in depth order, a distractor mask, clutter: the inputs of one keyframe."""
    rng = np.random.default_rng(seed)
    jit = lambda s: float(rng.uniform(-s, s))  # noqa: E731
    cars = [LC.det(7.5 + jit(0.4), 1.2 + jit(0.3), z=-1.6 + jit(0.05), theta=0.25 + jit(0.2)),
            LC.det(10.0 + jit(0.4), -3.4 + jit(0.3), z=-1.65 + jit(0.05), w=1.7, l=4.2, h=1.55, theta=-1.3 + jit(0.2)),
            LC.det(16.0 + jit(0.4), 9.5 + jit(0.3), z=-1.6 + jit(0.05), w=1.5, l=3.6, h=1.4, theta=1.45 + jit(0.1))]
    cars.sort(key=lambda d: d["trans"][0])                  # the reference sorts by x: keep its order ours
    tcv = LC.t_cam_velo(0.008, -0.015, (0.06, -0.07, -0.28))
    pts = [LC.box_points(d, n, rng, 0.97) for d, n in zip(cars, (640, 420, 160))]
    ground = np.stack([rng.uniform(2, 30, 2400), rng.uniform(-12, 12, 2400), rng.normal(-1.7, 0.03, 2400)], 1).astype(f32)
    velo = LC.sweep(pts + [ground], 4, rng)
    velo[:, 3] = rng.random(velo.shape[0]).astype(f32)      # reflectance
    # masks: the cars' rectangles (farther first, nearer painted over), then a distractor; listed in
    # another order than the detections
    inst = LC.blank(CAM)
    for i in (2, 1, 0):
        LC.paint_rect(inst, pts[i], 20 + i, 2, CAM, tcv)
    inst[2:30, 250:300] = np.where(inst[2:30, 250:300] < 0, 30, inst[2:30, 250:300])
    order = [30, 21, 20, 22]
    masks, bboxes = [], []
    for lab in order:
        m = inst == lab
        vs, us = np.nonzero(m)
        masks.append(m)
        # a detector's box: float corners, a little wider than the mask, truncated by the reference
        bboxes.append([us.min() - 1.4, vs.min() - 0.7, us.max() + 1.6, vs.max() + 1.2])
    dets = np.array([[*d["trans"], *d["size"], d["theta"]] for d in cars], f32)
    return dict(velo=velo, inst=inst, labels=np.array(order, np.int32), masks=np.stack(masks),
                bboxes=np.array(bboxes, f32), dets=dets, t_cam_velo=tcv)


def mask_list(x):
    return [(int(lab), tuple(int(v) for v in np.asarray(b).astype(np.int32))) for lab, b in zip(x["labels"], x["bboxes"])]


def det_dicts(dets):
    return [dict(trans=tuple(r[:3]), size=tuple(r[3:6]), theta=r[6]) for r in np.asarray(dets, f32)]


def screen(x):
    """The margins of the four conditions, or None when one fails."""
    tcv = x["t_cam_velo"]
    p = x["velo"][:, :3].astype(np.float64)
    face = math.inf
    pixel = math.inf
    hit = math.inf
    for d in det_dicts(x["dets"]):
        L = LO.prepare(d, tcv, PARAMS)
        lo, hi, e = (L[k].astype(np.float64) for k in ("lo", "hi", "e"))
        A = L["A"].astype(np.float64)
        close = np.all((p > lo - FACE_EPS) & (p < hi + FACE_EPS), 1)
        pc = p[close]
        xo = pc @ A[:, :3].T + A[:, 3]
        face = min(face, np.abs(pc - lo).min(), np.abs(pc - hi).min(), np.abs(np.abs(xo) - e).min())
        pts, rays, dobs, rec = LO.ingest(x["velo"], x["inst"], mask_list(x), d, CAM, tcv, **PARAMS)
        n, N = rec["n_pts"], rec["n_crop"]
        if N > n and not np.array_equal(np.linspace(0, N - 1, n).astype(np.int32), np.asarray(LO.FO.sel(n, N))):
            return None
        front = dobs[:n] > 0
        uf = CAM["fx"] * rays[:n, 0][front].astype(np.float64) + CAM["cx"]
        vf = CAM["fy"] * rays[:n, 1][front].astype(np.float64) + CAM["cy"]
        for c in (uf, vf):                                  # (the image borders are integers too)
            if c.size:
                pixel = min(pixel, np.abs(c - np.rint(c)).min())
        # hits per entry (the labels are listed once each), recounted here from the rows
        fov = (uf > 0) & (uf < W) & (vf > 0) & (vf < H)
        lab = x["inst"][vf[fov].astype(np.int64), uf[fov].astype(np.int64)]
        counts = np.array([int((lab == m).sum()) for m in x["labels"]], np.int64)
        srt = np.sort(counts)[::-1]
        hit = min(hit, abs(2 * int(srt[0]) - rec["n_proj"]) / 2.0, float(srt[0] - srt[1]) if srt[0] > 0 else math.inf)
        assert int(srt[0]) == rec["n_hits"], (srt, rec)
    if face <= FACE_EPS or pixel <= PIXEL_EPS or hit <= HIT_MARGIN:
        return None
    return dict(face=face, pixel=pixel, hit=hit)


def run_reference(x, ks):
    """get_detections on the inputs; the recorded outputs per instance, in the reference's order."""
    import torch

    K = np.array([[CAM["fx"], 0, CAM["cx"]], [0, CAM["fy"], CAM["cy"]], [0, 0, 1]], np.float32)
    fr = object.__new__(ks.FrameWithLiDAR)
    fr.online = False
    fr.frame_id = 0
    fr.K, fr.invK = K, np.linalg.inv(K).astype(np.float32)
    fr.T_cam_velo = x["t_cam_velo"].astype(np.float32)
    fr.velo_pts = x["velo"]
    fr.img_rgb = np.zeros((H, W, 3), np.uint8)
    fr.img_h, fr.img_w = H, W
    fr.max_lidar_pts, fr.min_mask_area = PARAMS["max_pts"], PARAMS["min_mask_area"]
    fr.configs = types.SimpleNamespace(downsample_ratio=PARAMS["downsample"])
    fr.instances = []
    load = torch.load
    with tempfile.TemporaryDirectory() as d:
        fr.lbl3d_dir, fr.lbl2d_dir = os.path.join(d, "3d"), os.path.join(d, "2d")
        os.makedirs(fr.lbl3d_dir)
        os.makedirs(fr.lbl2d_dir)
        torch.save(x["dets"], os.path.join(fr.lbl3d_dir, "000000.lbl"))
        torch.save(dict(pred_masks=x["masks"], pred_boxes=x["bboxes"]), os.path.join(fr.lbl2d_dir, "000000.lbl"))
        torch.load = functools.partial(load, weights_only=False)   # the labels are pickled numpy arrays
        try:
            fr.get_detections()
        finally:
            torch.load = load
    out = {}
    for i, ins in enumerate(fr.instances):
        has_mask = "mask" in ins
        out[f"ref{i}_num_surface_points"] = np.array(ins.num_surface_points)
        out[f"ref{i}_surface_points"] = np.asarray(ins.surface_points, np.float32)
        out[f"ref{i}_t_cam_obj"] = np.asarray(ins.T_cam_obj, np.float32)
        out[f"ref{i}_is_front"] = np.array(bool(ins.is_front))
        out[f"ref{i}_mask"] = np.array(next(j for j in range(len(x["masks"])) if np.array_equal(ins.mask, x["masks"][j]))
                                       if has_mask else -1)
        has_rays = ins.rays is not None
        out[f"ref{i}_has_rays"] = np.array(has_rays)
        out[f"ref{i}_rays"] = np.asarray(ins.rays, np.float32) if has_rays else np.zeros((0, 3), np.float32)
        out[f"ref{i}_depth"] = np.asarray(ins.depth, np.float32) if has_rays else np.zeros(0, np.float32)
    out["n_instances"] = np.array(len(fr.instances))
    return out


def main():
    import torch

    ref, ks = load_kitti_sequence()
    seed, margins = 2400, None
    while margins is None:
        seed += 1
        x = draw(seed)
        margins = screen(x)
    out = run_reference(x, ks)
    assert np.array_equal(np.argsort(x["dets"][:, 0]), np.arange(len(x["dets"])))
    out.update(velo=x["velo"], labels=x["labels"], masks=np.packbits(x["masks"], axis=-1), bboxes=x["bboxes"],
               dets=x["dets"], t_cam_velo=x["t_cam_velo"], cam=np.array([W, H, CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"]]),
               params=np.array([PARAMS[k] for k in ("max_pts", "max_bg", "downsample", "expand", "min_mask_area",
                                                    "radius", "box_margin")], np.float64),
               seed=np.array(seed), screen_face=np.array(margins["face"]), screen_pixel=np.array(margins["pixel"]),
               screen_hit=np.array(margins["hit"]),
               screen_limits=np.array([FACE_EPS, PIXEL_EPS, HIT_MARGIN]), torch=np.array(torch.__version__),
               numpy=np.array(np.__version__))
    path = os.path.join(HERE, "f24_lidar_frame.npz")
    np.savez_compressed(path, **out)
    print("seed", seed, "margins", margins, "bytes", os.path.getsize(path))
    for i in range(int(out["n_instances"])):
        print(i, int(out[f"ref{i}_num_surface_points"]), int(out[f"ref{i}_mask"]), bool(out[f"ref{i}_has_rays"]),
              out[f"ref{i}_rays"].shape)


if __name__ == "__main__":
    main()
