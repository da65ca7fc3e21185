"""The scene query (dsr_scene_*, include/dsr.h) without a GPU: the numpy
restatement (tests/scene_oracle.py) against a closed form, the host-only binning rule
(dsr_scene_bin_host) against the restatement, the new structs against their ctypes mirrors and the
argument and pose errors that are checked before the device is touched."""
from __future__ import annotations

import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import scene_oracle as SO
from conftest import REPO

HDR = os.path.join(REPO, "include", "dsr.h")
SYMBOLS = ("dsr_scene_create", "dsr_scene_set_objects", "dsr_scene_query", "dsr_scene_peek", "dsr_scene_stats_get",
           "dsr_scene_destroy", "dsr_scene_bin_host")
STRUCTS = {"dsr_scene_object": "SceneObject", "dsr_scene_object_out": "SceneObjectOut",
           "dsr_scene_stats": "SceneStats"}


def load():
    from reconstruct import _libdsr as L

    return L, L.load_library()


def test_symbols_exported_and_abi_unchanged():
    L, lib = load()
    out = subprocess.run(["nm", "-D", "--defined-only", L.lib_path()], capture_output=True, text=True,
                         check=True).stdout
    for f in SYMBOLS:
        assert hasattr(lib, f), f
        assert re.search(rf"\bT {f}$", out, flags=re.M), f
        assert f in L.SIGNATURES and f in L.BY_SYMBOL, f
    assert lib.dsr_abi_version() == 12 == L.ABI_VERSION
    assert "#define DSR_ABI_VERSION 12" in open(HDR).read()


def test_struct_layouts_match_ctypes():
    L, _ = load()
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
    seen = 0
    for line in out.strip().splitlines():
        py, what, val = line.split()
        cls = getattr(L, py)
        if what == "size":
            assert ctypes.sizeof(cls) == int(val), line
        else:
            assert getattr(cls, what).offset == int(val), line
        seen += 1
    assert seen == sum(1 + len(getattr(L, p)._fields_) for p in STRUCTS.values())


def test_the_scene_is_the_one_the_gpu_tests_rely_on():
    """the conditions tests/test_gpu_scene.py re-asserts, on the restatement alone"""
    poses = [t for t, _ in SO.scene_objects()]
    for n, counts in SO.COUNTS.items():
        pts = SO.scene_points(n)
        recs = [SO.bin_object(t, pts) for t in poses]
        assert tuple(r[0].size for r in recs) == counts
        r2 = np.stack([r[3] for r in recs])
        assert np.abs(r2 - 1.0).min() > 1e-4
    pts = SO.scene_points(1500)
    r2 = np.stack([SO.bin_object(t, pts)[3] for t in poses])
    assert int(((r2 < 1).sum(0) >= 1).sum()) == 1038 and int(((r2 < 1).sum(0) >= 2).sum()) == 275
    assert all(c % 64 for c in SO.COUNTS[1500]) and min(SO.COUNTS[1500]) < 64


@pytest.mark.parametrize("n", [1500, 400])
def test_bin_host_against_the_restatement(n):
    from reconstruct.optimizer import scene_bin

    objs = SO.scene_objects()
    pts = SO.scene_points(n)
    for i, (t, _) in enumerate(objs):
        idx, x, s = scene_bin(objs, pts, i)
        ridx, rx, rs, _ = SO.bin_object(t, pts)
        assert idx.dtype == np.int32 and x.dtype == np.float32 and x.shape == (idx.size, 3)
        assert np.array_equal(idx, ridx) and idx.size == SO.COUNTS[n][i]           # membership and order
        _, mag = SO.transform(t, pts)
        err = np.abs(x.astype(np.float64) - rx)
        assert np.all(err <= 1e-6 * mag[ridx]), float((err / mag[ridx]).max())
        # s: det(R)^(1/3) in float64 rounded once, within 1 ulp of float32 of the scale put in
        T = np.asarray(t, np.float64)
        exact = np.cbrt(np.linalg.det(T[:3, :3]))
        assert abs(s - exact) <= np.spacing(np.float32(exact)) and np.float32(s) == np.float32(rs)
        assert abs(s - SO.SCALES[i]) <= 4 * np.spacing(np.float32(SO.SCALES[i]))   # (the fp32 rotation is not exactly orthonormal)


def bin_rc(lib, L, objs, pts, i, cap=None, n_obj=None):
    from reconstruct.optimizer import _scene_objects

    ins, _ = _scene_objects([(t, None) for t, _ in objs], 0)
    pts = np.ascontiguousarray(pts, np.float32)
    n = pts.shape[0]
    cap = n if cap is None else cap
    idx, x = np.zeros(max(cap, 1), np.int32), np.zeros((max(cap, 1), 3), np.float32)
    cnt, s = ctypes.c_int(-7), ctypes.c_float()
    rc = lib.dsr_scene_bin_host(len(objs) if n_obj is None else n_obj, ins, n, L.fptr(pts), i, cap, L.iptr(idx),
                                L.fptr(x), ctypes.cast(ctypes.byref(cnt), L.IP), ctypes.cast(ctypes.byref(s), L.FP))
    return rc, cnt.value, idx, x


def test_argument_and_pose_errors_before_the_device():
    """No GPU is needed to see them: nothing is created, the status is the argument's (-2; there
    is no context to carry a message), and a capacity too small is -5 with the count."""
    L, lib = load()
    objs = SO.scene_objects()
    pts = SO.scene_points(400)
    assert bin_rc(lib, L, objs, pts, 0)[:2] == (0, 141)
    rc, cnt, idx, _ = bin_rc(lib, L, objs, pts, 0, cap=140)
    assert rc == -5 and cnt == 141 and not idx.any()                   # the count, and nothing copied
    assert bin_rc(lib, L, objs, pts, 0, cap=141)[0] == 0
    assert bin_rc(lib, L, objs, pts, 4)[0] == -2 and bin_rc(lib, L, objs, pts, -1)[0] == -2
    assert bin_rc(lib, L, objs, pts, 0, n_obj=0)[0] == -2
    assert lib.dsr_scene_bin_host(4, None, 0, None, 0, 0, None, None, None, None) == -2
    row, mirror, flat, nan, inf = (SO.scene_pose(1) for _ in range(5))
    row[3, 3] = 2.0
    mirror[:3, 0] *= -1.0
    flat[:3, :3] = 0.0
    nan[1, 3] = np.nan
    inf[0, 0] = np.inf
    for bad in (row, mirror, flat, nan, inf):
        assert SO.pose(bad) is None
        # a bad pose anywhere in the list is refused, whichever object is asked for
        assert bin_rc(lib, L, [objs[0], (bad, None)], pts, 0)[0] == -2
        with pytest.raises(L.DsrError):
            from reconstruct.optimizer import scene_bin
            scene_bin([objs[0], (bad, None)], pts, 0)
    # the device entry points refuse null arguments before anything else: no context exists here
    h = ctypes.c_void_p(123)
    assert lib.dsr_scene_create(None, None, 4, 1024, ctypes.byref(h)) < 0
    assert lib.dsr_scene_create(None, None, 4, 1024, None) < 0
    assert lib.dsr_scene_set_objects(None, 0, None) < 0
    assert lib.dsr_scene_query(None, 0, None, None, None, None, None) < 0
    assert lib.dsr_scene_peek(None, 0, 0, None, None, None, None) < 0
    assert lib.dsr_scene_stats_get(None, None) < 0
    assert lib.dsr_scene_destroy(None) == 0


def test_non_finite_points_land_in_no_ball():
    L, lib = load()
    objs = SO.scene_objects()
    pts = SO.scene_points(400)
    base = [bin_rc(lib, L, objs, pts, i)[1] for i in range(4)]
    assert tuple(base) == SO.COUNTS[400]
    inside0 = SO.bin_object(objs[0][0], pts)[0]
    bad = pts.copy()
    a, b, c, d = (int(v) for v in inside0[:4])
    bad[a, 0] = np.nan
    bad[b, 1] = np.inf
    bad[c, 2] = -np.inf
    bad[d] = np.nan
    for i in range(4):
        rc, cnt, idx, _ = bin_rc(lib, L, objs, bad, i)
        ridx = SO.bin_object(objs[i][0], bad)[0]
        assert rc == 0 and np.array_equal(idx[:cnt], ridx)
        assert not set(idx[:cnt].tolist()) & {a, b, c, d}
    assert bin_rc(lib, L, objs, bad, 0)[1] == base[0] - 4
    # a finite point far outside float32's squared range is outside as well
    far = np.array([[3e38, 0, 0], [1e20, -1e20, 1e20]], np.float32)
    assert bin_rc(lib, L, objs, far, 0)[1] == 0


def sphere_sdf(x):
    return np.linalg.norm(x, axis=1) - 0.5


def sphere_grad(x):
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def test_restatement_on_an_analytic_sdf():
    """|x| - 0.5 under a Sim(3): dist = s (|x| - 0.5) in closed form (|x| = |p - c| / s), grad the
    unit radial direction in the world; of two overlapping spheres the nearer surface wins and an
    exact tie goes to the lower index."""
    rng = np.random.default_rng(3)
    T = SO.scene_pose(1, scale=1.5, centre=(0.25, -0.5, 1.0))
    c = T[:3, 3].astype(np.float64)
    pts = (c + rng.uniform(-2, 2, (600, 3))).astype(np.float32)
    r = SO.query([sphere_sdf], [T], pts, [sphere_grad])
    rad = np.linalg.norm(pts.astype(np.float64) - c, axis=1)
    s = SO.pose(T)[2]
    inside = rad < s * (1 - 1e-6)
    outside = rad > s * (1 + 1e-6)
    assert inside.sum() > 100 and outside.sum() > 100
    assert np.all(r.obj[inside] == 0) and np.all(r.obj[outside] == -1) and np.all(np.isinf(r.dist[outside]))
    assert np.abs(r.dist[inside] - (rad[inside] - 0.5 * s)).max() <= 1e-5
    radial = (pts.astype(np.float64) - c) / rad[:, None]
    assert np.abs(r.grad[inside] - radial[inside]).max() <= 1e-5
    assert np.all(r.grad[r.obj < 0] == 0.0)
    rec = r.objects[0]
    assert rec.n_in == rec.n_win == int((r.obj == 0).sum()) and rec.n_neg == int((r.dist < 0).sum())
    assert abs(rec.sum_sdf - (r.dist[r.obj == 0] / s).sum()) <= 1e-9 * rec.n_in
    # two overlapping spheres: the nearer surface wins
    T2 = SO.scene_pose(2, scale=1.0, centre=(1.0, -0.5, 1.0))
    both = SO.query([sphere_sdf, sphere_sdf], [T, T2], pts, [sphere_grad, sphere_grad])
    one = SO.query([sphere_sdf], [T2], pts)
    in1, in2 = r.obj == 0, one.obj == 0
    assert (in1 & in2).sum() > 20
    want = np.where(in1 & (~in2 | (r.dist <= one.dist)), 0, np.where(in2, 1, -1))
    assert np.array_equal(both.obj, want)
    assert np.array_equal(both.dist, np.minimum(r.dist, one.dist))
    assert both.objects[0].n_win + both.objects[1].n_win == int((in1 | in2).sum())
    assert both.objects[1].n_in == one.objects[0].n_in              # n_in does not depend on who wins
    # the same object twice: an exact tie, the lower index wins every point
    tie = SO.query([sphere_sdf, sphere_sdf], [T, T], pts)
    assert np.all(tie.obj[in1] == 0) and tie.objects[1].n_win == 0 and tie.objects[1].n_in == rec.n_in
    # no objects, no points
    e = SO.query([], [], pts)
    assert np.all(np.isinf(e.dist)) and np.all(e.obj == -1) and np.all(e.grad == 0)
    e = SO.query([sphere_sdf], [T], np.zeros((0, 3), np.float32))
    assert e.dist.shape == (0,) and e.objects[0].n_in == 0
