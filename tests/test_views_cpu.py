"""Multi-view reconstruction (dsr_reconstruct_views) without a GPU: the numpy restatement the GPU
tests check against (tests/views_oracle.py) reduces to the single-view oracle, the host helpers
are exact and deterministic, and the C ABI grew by the two records and the one symbol only."""
from __future__ import annotations

import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import synthetic as S
from conftest import REPO
from views_oracle import gn_step_views, oracle_views

HDR = os.path.join(REPO, "include", "dsr.h")
REDWOOD = dict(scale=1.0, tz=3.0, upright=False)
KITTI = dict(scale=2.0, tz=15.0, upright=True)


def _params(optim):
    from oracle import dsr_oracle as O

    return O.OptimParams.from_cfg(optim)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("optim,shape", [(S.REDWOOD_OPTIM, REDWOOD), (S.KITTI_OPTIM, KITTI)])
def test_one_view_is_the_single_view_oracle(oracle_dec, dtype, optim, shape):
    from oracle import dsr_oracle as O

    dec = type(oracle_dec)(oracle_dec.layers, dtype=dtype)
    ob = S.make_object_views(700, 1, n_pts=130, n_bg=40, **shape)
    (view,) = oracle_views(ob, dtype)
    T = np.linalg.inv(ob.t_cam_obj.astype(dtype))
    z = (0.05 * np.random.default_rng(1).standard_normal(64)).astype(dtype)
    P = _params(optim)
    tv, Tv, zv = gn_step_views(dec, P, T, z, [view])
    t1, T1, z1 = O.gn_step(dec, P, T, z, view[1], view[2], view[3], view[4])
    assert Tv is not None and T1 is not None
    for a, b in ((tv.H, t1.H), (tv.b, t1.b), (tv.dx, t1.dx), (Tv, T1), (zv, z1)):
        assert a.dtype == dtype and np.array_equal(a, b)
    assert (tv.loss, tv.sdf_loss, tv.render_loss) == (t1.loss, t1.sdf_loss, t1.render_loss)
    assert tv.k == [t1.k] and tv.n_valid == [t1.n_valid]


def test_identity_views_pool_like_one_object(oracle_dec):
    """Two views with identity t_view_ref that split one object's points and rays between them
    are that object: the pooled normal equations equal the unsplit ones to fp64 rounding."""
    from oracle import dsr_oracle as O

    dec = type(oracle_dec)(oracle_dec.layers, dtype=np.float64)
    ob = S.make_object(701, n_pts=130, n_bg=40, **REDWOOD)
    dt = np.float64
    n = 130
    pts, rays, depth = ob.pts.astype(dt), ob.rays.astype(dt), ob.depth.astype(dt)
    T = np.linalg.inv(ob.t_cam_obj.astype(dt))
    z = np.zeros(64, dt)
    P = _params(S.REDWOOD_OPTIM)
    dobs = np.concatenate([depth, np.zeros(40)])
    t1, T1, z1 = O.gn_step(dec, P, T, z, pts, rays, dobs, n)
    h = 61                                      # fg split 61 / 69, bg split 17 / 23
    va = (np.eye(4), pts[:h], np.concatenate([rays[:h], rays[n:n + 17]]),
          np.concatenate([depth[:h], np.zeros(17)]), h)
    vb = (np.eye(4), pts[h:], np.concatenate([rays[h:n], rays[n + 17:]]),
          np.concatenate([depth[h:], np.zeros(23)]), n - h)
    tv, Tv, zv = gn_step_views(dec, P, T, z, [va, vb])
    assert sum(tv.k) == t1.k and sum(tv.n_valid) == t1.n_valid
    for a, b in ((tv.H, t1.H), (tv.b, t1.b), (tv.dx, t1.dx), (Tv, T1), (zv, z1)):
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max()
    assert abs(tv.loss - t1.loss) <= 1e-12 * abs(t1.loss)


def test_failures_of_the_restatement(oracle_dec):
    """A view whose rays miss the ball fails with its index; no points anywhere is the sdf NaN;
    one view without points is fine."""
    ob = S.make_object_views(702, 3, n_pts=130, n_bg=40, **REDWOOD)
    views = oracle_views(ob)
    T = np.linalg.inv(ob.t_cam_obj)
    z = np.zeros(64, np.float32)
    P = _params(S.REDWOOD_OPTIM)
    miss = list(views)
    miss[1] = (views[1][0], views[1][1], views[1][2] + np.float32([5.0, 0.0, 0.0]), views[1][3], views[1][4])
    tr, Tn, _ = gn_step_views(oracle_dec, P, T, z, miss)
    assert Tn is None and tr.fail_view == 1
    nopts = [(v[0], v[1][:0], v[2], v[3], v[4]) for v in views]
    tr, Tn, _ = gn_step_views(oracle_dec, P, T, z, nopts)
    assert Tn is None and np.isnan(tr.sdf_loss) and tr.fail_view == -1
    one = list(views)
    one[2] = nopts[2]
    tr, Tn, _ = gn_step_views(oracle_dec, P, T, z, one)
    assert Tn is not None and np.isfinite(tr.loss)


def test_views_from_world_round_trips():
    from reconstruct.utils import views_from_world

    rng = np.random.default_rng(3)
    poses = []
    for _ in range(4):
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        q *= np.sign(np.linalg.det(q))
        t = np.eye(4)
        t[:3, :3] = q
        t[:3, 3] = rng.uniform(-5, 5, 3)
        poses.append(t)
    tv = views_from_world(poses)
    assert len(tv) == 4 and all(t.dtype == np.float64 and t.shape == (4, 4) for t in tv)
    assert np.array_equal(tv[0], np.eye(4))
    xw = rng.uniform(-3, 3, (50, 4))
    xw[:, 3] = 1.0
    x_ref = xw @ poses[0].T
    for v in range(1, 4):
        assert np.abs(tv[v] - poses[v] @ np.linalg.inv(poses[0])).max() <= 1e-14
        assert np.abs(x_ref @ tv[v].T - xw @ poses[v].T).max() <= 1e-13     # x_view = t_view_ref x_ref
    assert views_from_world([]) == []


def test_make_object_views_is_deterministic_and_extends_make_object():
    a = S.make_object_views(700, 3, n_pts=130, n_bg=40, **KITTI)
    b = S.make_object_views(700, 3, n_pts=130, n_bg=40, **KITTI)
    ob = S.make_object(700, n_pts=130, n_bg=40, **KITTI)
    assert np.array_equal(a.t_cam_obj, ob.t_cam_obj) and np.array_equal(a.t_true, ob.t_true)
    for x, y in zip(a.views[0][1:], (ob.pts, ob.rays, ob.depth)):
        assert np.array_equal(x, y)
    assert np.array_equal(a.views[0][0], np.eye(4))
    signs = []
    for v, (va, vb) in enumerate(zip(a.views, b.views)):
        for x, y in zip(va, vb):
            assert np.array_equal(x, y)
        t, pts, rays, depth = va
        assert pts.shape == (130 + 13 * v, 3) and rays.shape == (130 + 13 * v + 40, 3)
        assert pts.dtype == rays.dtype == depth.dtype == np.float32
        assert np.array_equal(depth, pts[:, 2]) and np.allclose(rays[:pts.shape[0]], pts / pts[:, 2:3])
        assert np.abs(t[:3, :3].T @ t[:3, :3] - np.eye(3)).max() < 1e-12       # rigid
        assert np.abs(t[:3, :3] @ [0, 1, 0] - [0, 1, 0]).max() < 1e-12         # about camera y
        # the surface points lie on the true object's sphere as view v sees it
        tv = t @ a.t_true.astype(np.float64)
        xo = (pts - tv[:3, 3]) @ np.linalg.inv(tv[:3, :3]).T
        assert np.abs(np.linalg.norm(xo, axis=1) - 0.5).max() < 1e-4
        if v:
            ang = np.arctan2(t[0, 2], t[0, 0])
            assert 0.5 <= abs(ang) <= 2.5
            signs.append(np.sign(ang))
    assert signs == [1.0, -1.0]
    # view 0 and the start pose do not depend on the number of views
    c = S.make_object_views(700, 2, n_pts=130, n_bg=40, **KITTI)
    assert all(np.array_equal(x, y) for x, y in zip(c.views[1], a.views[1]))


# ---- ABI: additive, detected by the symbol
STRUCTS = {"dsr_view_in": "ViewIn", "dsr_views_object_in": "ViewsObjectIn"}


def test_abi_version_is_unchanged():
    from reconstruct import _libdsr as L

    assert re.search(r"^#define DSR_ABI_VERSION 12$", open(HDR).read(), flags=re.M)
    assert L.ABI_VERSION == 12


def test_view_struct_layouts_match_ctypes():
    from reconstruct import _libdsr as L

    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HDR}"', "int main(void){"]
    for cname, pyname in STRUCTS.items():
        lines.append(f'printf("{pyname} size %zu\\n", sizeof({cname}));')
        for fld, _ in getattr(L, pyname)._fields_:
            lines.append(f'printf("{pyname} {fld} %zu\\n", offsetof({cname}, {fld}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c99", "-o", exe, src], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    seen = set()
    for line in out.strip().splitlines():
        py, what, val = line.split()
        cls = getattr(L, py)
        if what == "size":
            assert ctypes.sizeof(cls) == int(val), line
            seen.add(py)
        else:
            assert getattr(cls, what).offset == int(val), line
    assert seen == set(STRUCTS.values())


def test_library_exports_dsr_reconstruct_views():
    from reconstruct import _libdsr as L

    lib = L.load_library()
    assert hasattr(lib, "dsr_reconstruct_views")
    out = subprocess.run(["nm", "-D", "--defined-only", L.lib_path()], capture_output=True, text=True,
                         check=True).stdout
    assert re.search(r"\bT dsr_reconstruct_views$", out, flags=re.M)
    assert lib.dsr_reconstruct_views.argtypes == L.SIGNATURES["dsr_reconstruct_views"][1]


def test_argument_errors_need_no_device():
    """n_views < 1 and null arguments are rejected before anything touches the device."""
    from reconstruct import _libdsr as L

    lib = L.load_library()
    ins = (L.ViewsObjectIn * 1)()
    outs = (L.ObjectOut * 1)()
    P = L.optim_params(S.REDWOOD_OPTIM)
    assert lib.dsr_reconstruct_views(None, None, ctypes.byref(P), 1, ins, outs, None, None, None) < 0
