"""``gn_step_views``: one Gauss-Newton iteration of the multi-view reconstruction
(dsr_reconstruct_views, include/dsr.h) restated in numpy from the oracle's public pieces only —
``compute_sdf_loss``, ``compute_render_loss``, ``get_robust_res``,
``compute_rotation_loss_sim3``, ``exp_sim3``, ``linspace_torch`` (oracle/dsr_oracle.py).

It is ``oracle.gn_step`` (optimizer.py:120-194) with the residual sets pooled: view v's terms
are taken under ``T_v = T @ inverse(t_view_ref_v)`` (``T_0 = T`` itself), the sdf rows and the
render rows of all views are concatenated, and everything from the Huber weights on is the
single-view code applied to the pooled sets; the rotation prior is evaluated once, at ``T``.
Shared by tests/test_views_cpu.py and tests/test_gpu_views.py.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

from oracle import dsr_oracle as O


@dataclass
class ViewsTrace:
    t_obj_cam: np.ndarray
    z: np.ndarray
    loss: float = float("nan")
    sdf_loss: float = float("nan")
    render_loss: float = float("nan")
    n_valid: list = field(default_factory=list)      # per view
    k: list = field(default_factory=list)            # per view
    fail_view: int = -1
    H: np.ndarray = None
    b: np.ndarray = None
    dx: np.ndarray = None


def rigid_inverse(t_view_ref):
    """inverse of a rigid 4x4 in float64: [R^T | -R^T t], of the float32 matrix the C ABI carries."""
    t = np.asarray(t_view_ref, np.float32).astype(np.float64)
    c = np.eye(4)
    c[:3, :3] = t[:3, :3].T
    c[:3, 3] = -t[:3, :3].T @ t[:3, 3]
    return c


def view_pose(t_obj_ref, t_view_ref, v, dt):
    """T_v = T . C_v in the decoder's dtype, C_v rounded once; view 0 is T itself."""
    if v == 0:
        return t_obj_ref
    return t_obj_ref @ rigid_inverse(t_view_ref).astype(dt)


def gn_step_views(dec, p, t_obj_ref, z, views):
    """One iteration at state (t_obj_ref, z).  ``views``: list of
    ``(t_view_ref, pts, rays, depth_obs, n_fg)`` with depth_obs padded to the ray count like
    oracle.gn_step's.  Returns (ViewsTrace, new t_obj_ref, new z), or (ViewsTrace, None, None) on
    the reference's failure exits (optimizer.py:132-152), ``fail_view`` naming the view with
    fewer than 10 in-ball samples."""
    dt = dec.dtype
    tr = ViewsTrace(t_obj_ref.copy(), z.copy())
    poses, depth_lists, dobs = [], [], []
    for v, (t_view_ref, pts, rays, depth_obs, n_fg) in enumerate(views):
        t_v = view_pose(t_obj_ref, t_view_ref, v, dt)
        t_cam_obj = np.linalg.inv(t_v)                                    # :122
        scale = dt(np.linalg.det(t_cam_obj[:3, :3])) ** dt(1.0 / 3.0)    # :123
        d_min = t_cam_obj[2, 3] - dt(1.0) * scale
        d_max = t_cam_obj[2, 3] + dt(1.0) * scale
        depth_lists.append(O.linspace_torch(d_min, d_max, p.num_depth_samples, dt))   # :126
        d = depth_obs.copy()
        d[n_fg:] = dt(1.1) * d_max                                        # :128
        dobs.append(d)
        poses.append(t_v)
    L = p.code_len
    js, rs = [], []
    for v, (_, pts, _, _, _) in enumerate(views):                         # :131, every view's points
        if pts.shape[0] == 0:
            continue
        jp, jc, r = O.compute_sdf_loss(dec, pts, poses[v], z)
        js.append(np.concatenate([jp, jc], -1))
        rs.append(r)
    J_s = np.concatenate(js, 0) if js else np.zeros((0, 7 + L), dt)
    r_s = np.concatenate(rs, 0) if rs else np.zeros(0, dt)
    rr_s, l_s, _ = O.get_robust_res(r_s, p.b2)
    tr.sdf_loss = float(l_s)
    if math.isnan(l_s):
        return tr, None, None
    jr, rr = [], []
    for v, (_, _, rays, _, _) in enumerate(views):
        ren = O.compute_render_loss(dec, rays, dobs[v], poses[v], depth_lists[v], z, th=p.cut_off)
        if ren is None:                                                   # loss.py:86-88
            tr.fail_view = v
            return tr, None, None
        tr.n_valid.append(ren.n_valid)
        tr.k.append(int(ren.res.shape[0]))
        jr.append(np.concatenate([ren.j_pose, ren.j_code], -1))
        rr.append(ren.res)
    J_r = np.concatenate(jr, 0)
    rr_r, l_r, _ = O.get_robust_res(np.concatenate(rr, 0), p.b1)
    tr.render_loss = float(l_r)
    if math.isnan(l_r):
        return tr, None, None
    j_rot, r_rot = O.compute_rotation_loss_sim3(t_obj_ref)                # :155, the reference view
    loss = dt(p.k1) * l_r + dt(p.k2) * l_s                                # :157
    tr.loss = float(loss)
    pd = 7
    H_s = dt(p.k2) * (J_s.T @ J_s) / dt(J_s.shape[0])                     # :163
    b_s = -dt(p.k2) * (J_s.T @ rr_s) / dt(J_s.shape[0])                   # :164
    H_r = dt(p.k1) * (J_r.T @ J_r) / dt(J_r.shape[0])
    b_r = -dt(p.k1) * (J_r.T @ rr_r) / dt(J_r.shape[0])
    H = H_r + H_s
    H[pd:pd + L, pd:pd + L] += dt(p.k3) * np.eye(L, dtype=dt)              # :172
    b = b_r + b_s
    b[pd:pd + L] -= dt(p.k3) * z
    H_rot = np.outer(j_rot, j_rot)                                        # :176-181
    b_rot = -(j_rot * r_rot)
    H[:pd, :pd] += dt(p.k4) * H_rot
    b[:pd] -= dt(p.k4) * b_rot
    H[:pd, :pd] += np.eye(pd, dtype=dt)                                   # :185
    H[pd - 1, pd - 1] += dt(p.s_damp)                                     # :186
    dx = np.linalg.inv(H) @ b                                             # :188
    tr.H, tr.b, tr.dx = H, b, dx
    t_new = O.exp_sim3(dt(p.lr) * dx[:pd]) @ t_obj_ref                    # :192
    z_new = z + dt(p.lr) * dx[pd:pd + L]                                  # :194
    return tr, t_new, z_new


def oracle_views(obj, dt=np.float32):
    """A synthetic.SyntheticObjectViews' views as gn_step_views takes them."""
    out = []
    for t_view_ref, pts, rays, depth in obj.views:
        n_fg = depth.shape[0]
        dobs = np.concatenate([depth, np.zeros(rays.shape[0] - n_fg)]).astype(dt)
        out.append((np.asarray(t_view_ref, np.float64), pts.astype(dt), rays.astype(dt), dobs, n_fg))
    return out
