"""The sphere tracer (dsr_renderer_*, include/dsr.h) without a GPU: the numpy
restatement (tests/render_oracle.py) against a closed form, the host-only rectangle rule
(dsr_render_layout) against the restatement, the new structs against their ctypes mirrors and the
argument errors that are checked before the device is touched."""
from __future__ import annotations

import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

import render_oracle as RO
import synthetic as S
from conftest import REPO

HDR = os.path.join(REPO, "include", "dsr.h")
RENDER_FUNCS = ("dsr_renderer_create", "dsr_renderer_render", "dsr_renderer_stats_get", "dsr_renderer_destroy",
                "dsr_render_layout")


def sim3(seed, scale, t):
    T = S.make_object(seed, n_pts=8, scale=scale, tz=15, perturb=0).t_true.copy()
    T[:3, 3] = t
    return T.astype(np.float32)


def test_restatement_traces_an_analytic_sphere_to_the_closed_form():
    """|x| - 0.5 in the object frame under a Sim(3) pose is a sphere of radius 0.5 s at c in the
    camera frame.  Every hit lies within hit_eps / |g^.d^| * s of the closed-form ray-sphere depth
    (|y| < hit_eps bounds the distance to the surface along the ray by hit_eps / |g^.d^| in object
    units, s / |r| <= s camera units of depth each), pixels outside the silhouette are exactly
    0 / -1, and every pixel that meets the sphere at |g^.d^| >= 0.2 is hit."""
    cam = RO.Camera(48, 36, 120.0, 120.0, 23.5, 17.5)
    T = sim3(7, 2.0, (0.1, -0.05, 15.0))
    hit_eps = 1e-4
    depth, inst, (tr,) = RO.render([lambda x: np.linalg.norm(x, axis=1) - 0.5], cam, [T])
    toc, c, s = RO.pose(T)
    assert abs(s - 2.0) < 1e-6
    vv, uu = np.meshgrid(np.arange(cam.height), np.arange(cam.width), indexing="ij")
    r = np.stack([(uu - cam.cx) / cam.fx, (vv - cam.cy) / cam.fy, np.ones_like(uu, float)], -1)
    a = (r * r).sum(-1)
    b = r @ c
    disc = b * b - a * (c @ c - (0.5 * s) ** 2)
    inside = disc > 0
    lam_ref = (b - np.sqrt(np.where(inside, disc, 0))) / a
    assert np.all(depth[~inside] == 0.0) and np.all(inst[~inside] == -1)
    hit = inst == 0
    assert not np.any(hit & ~inside)
    # |g^ . d^| at the closed-form hit: the normal is (x - c) / (0.5 s), the ray r / |r|
    x = lam_ref[..., None] * r
    cosang = np.abs(((x - c) / (0.5 * s) * r).sum(-1)) / np.sqrt(a)
    assert np.all(hit[inside & (cosang >= 0.2)])
    assert hit.sum() > 150                              # a disc of radius 120 * 1 / 15 = 8 pixels
    err = np.abs(depth - lam_ref)[hit]
    bound = hit_eps / cosang[hit] * s
    assert np.all(err <= bound), float((err / bound).max())
    assert tr.hit.sum() == hit.sum() and tr.ball.sum() >= tr.hit.sum() + tr.unconverged.sum()


def test_restatement_composite_keeps_the_nearer_surface_and_the_lower_index():
    cam = RO.Camera(48, 36, 120.0, 120.0, 23.5, 17.5)
    sph = lambda x: np.linalg.norm(x, axis=1) - 0.5   # noqa: E731
    near, far = sim3(7, 2.0, (0.0, 0.0, 12.0)), sim3(8, 2.0, (0.0, 0.0, 18.0))
    d0, i0, _ = RO.render([sph, sph], cam, [near, far])
    d1, i1, _ = RO.render([sph, sph], cam, [far, near])
    assert np.array_equal(d0, d1)
    both = (i0 >= 0)
    assert np.array_equal(i0[both], 1 - i1[both]) and np.all(i0[d0 > 0][d0[d0 > 0] < 13.0] == 0)
    d2, i2, _ = RO.render([sph, sph], cam, [near, near])
    assert np.all(i2[i2 >= 0] == 0)                    # a tie goes to the lower index


def load():
    from reconstruct import _libdsr as L

    return L, L.load_library()


def test_symbols_exist_and_the_abi_is_still_12():
    L, lib = load()
    for f in RENDER_FUNCS:
        assert hasattr(lib, f), f
        assert f in L.SIGNATURES and f in L.BY_SYMBOL
    assert lib.dsr_abi_version() == 12 == L.ABI_VERSION
    txt = open(HDR).read()
    assert "#define DSR_ABI_VERSION 12" in txt
    for f in RENDER_FUNCS:                              # every entry point names what it replaces
        assert f in txt
    assert txt.count("src/ObjectRenderer.cc:82-125") >= 4


def c_layout(lib, L, cam, near, poses):
    n = len(poses)
    objs = (L.RenderObject * max(n, 1))()
    for i, t in enumerate(poses):
        objs[i].t_cam_obj[:] = np.asarray(t, np.float32).reshape(16).tolist()
    rect = np.full((max(n, 1), 4), 77, np.int32)
    status = np.full(max(n, 1), 77, np.int32)
    c = L.Camera(cam.width, cam.height, cam.fx, cam.fy, cam.cx, cam.cy)
    rc = lib.dsr_render_layout(ctypes.byref(c), float(near), n, objs, L.iptr(rect), L.iptr(status))
    return rc, rect[:n], status[:n]


CAM = RO.Camera(48, 36, 120.0, 120.0, 23.5, 17.5)
LAYOUT_CASES = {
    "centred": [(0.0, 0.0, 15.0, 1.0)],
    "left_edge": [(-2.5, 0.0, 15.0, 1.0)],
    "right_edge": [(2.5, 0.0, 15.0, 1.0)],
    "top_edge": [(0.0, -2.0, 15.0, 1.0)],
    "bottom_edge": [(0.0, 2.0, 15.0, 1.0)],
    "off_screen": [(30.0, 0.0, 15.0, 1.0), (0.0, -30.0, 15.0, 1.0)],
    "near_plane": [(0.0, 0.0, 1.0, 1.0), (0.0, 0.0, 1.005, 1.0), (0.0, 0.0, -5.0, 1.0)],
    "mixed": [(0.0, 0.0, 15.0, 2.0), (30.0, 0.0, 15.0, 1.0), (0.1, -0.05, 15.0, 2.0), (0.0, 0.0, 0.5, 1.0)],
}


@pytest.mark.parametrize("case", sorted(LAYOUT_CASES))
def test_layout_equals_the_restated_rectangle_rule(case):
    L, lib = load()
    poses = [sim3(7 + i, sc, (x, y, z)) for i, (x, y, z, sc) in enumerate(LAYOUT_CASES[case])]
    rc, rect, status = c_layout(lib, L, CAM, 0.01, poses)
    assert rc == 0
    rect_o, status_o = RO.layout(CAM, 0.01, poses)
    assert np.array_equal(status, status_o) and np.array_equal(rect, rect_o), (rect, rect_o, status, status_o)
    W, H = CAM.width, CAM.height
    for r, s in zip(rect, status):
        if s != RO.OK:
            assert tuple(r) == (0, 0, -1, -1)           # zero rays
        else:
            assert 0 <= r[0] <= r[2] < W and 0 <= r[1] <= r[3] < H
    if case == "centred":
        assert status[0] == RO.OK and 0 < rect[0][0] and rect[0][2] < W - 1 and 0 < rect[0][1] and rect[0][3] < H - 1
    if case.endswith("_edge"):
        edge = {"left_edge": rect[0][0] == 0, "right_edge": rect[0][2] == W - 1, "top_edge": rect[0][1] == 0,
                "bottom_edge": rect[0][3] == H - 1}[case]
        assert status[0] == RO.OK and edge
        assert (rect[0][2] - rect[0][0] + 1) * (rect[0][3] - rect[0][1] + 1) < W * H
    if case == "off_screen":
        assert list(status) == [RO.OFFSCREEN] * 2
    if case == "near_plane":                            # c_z - rho < near: 0 < 0.01, 0.005 < 0.01, behind
        assert list(status) == [RO.SKIP_NEAR] * 3


def test_layout_of_no_objects_and_bad_arguments():
    L, lib = load()
    rc, rect, status = c_layout(lib, L, CAM, 0.01, [])
    assert rc == 0 and rect.shape == (0, 4)
    assert lib.dsr_render_layout(ctypes.byref(L.Camera(48, 36, 120.0, 120.0, 23.5, 17.5)), 0.01, 0, None, None, None) == 0
    good = sim3(7, 1.0, (0.0, 0.0, 15.0))
    assert c_layout(lib, L, RO.Camera(0, 36, 120.0, 120.0, 0.0, 0.0), 0.01, [good])[0] < 0
    assert c_layout(lib, L, RO.Camera(48, 36, 0.0, 120.0, 0.0, 0.0), 0.01, [good])[0] < 0
    bad_row = good.copy()
    bad_row[3, 3] = 2.0
    assert c_layout(lib, L, CAM, 0.01, [bad_row])[0] < 0
    mirror = good.copy()
    mirror[:3, 0] *= -1.0                               # determinant < 0
    assert c_layout(lib, L, CAM, 0.01, [mirror])[0] < 0
    assert lib.dsr_render_layout(None, 0.01, 0, None, None, None) < 0
    # near <= 0 means the default
    a = c_layout(lib, L, CAM, 0.0, [good])
    b = c_layout(lib, L, CAM, 0.01, [good])
    assert a[0] == b[0] == 0 and np.array_equal(a[1], b[1])


STRUCTS = {"dsr_camera": "Camera", "dsr_render_params": "RenderParams", "dsr_render_object": "RenderObject",
           "dsr_render_object_out": "RenderObjectOut", "dsr_render_stats": "RenderStats"}


def test_render_struct_layouts_match_ctypes():
    L, _ = load()
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HDR}"', "int main(void){"]
    for cname, pyname in STRUCTS.items():
        lines.append(f'printf("{pyname} size %zu\\n", sizeof({cname}));')
        for fld, _t in getattr(L, pyname)._fields_:
            lines.append(f'printf("{pyname} {fld} %zu\\n", offsetof({cname}, {fld}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "layout.c")
        exe = os.path.join(d, "layout")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c99", "-o", exe, src], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    seen = set()
    for line in out.strip().splitlines():
        py, what, val = line.split()
        cls = getattr(L, py)
        seen.add(py)
        if what == "size":
            assert ctypes.sizeof(cls) == int(val), line
        else:
            assert getattr(cls, what).offset == int(val), line
    assert seen == set(STRUCTS.values())
    assert (L.RENDER_OK, L.RENDER_OFFSCREEN, L.RENDER_SKIP_NEAR) == (RO.OK, RO.OFFSCREEN, RO.SKIP_NEAR)


def test_renderer_create_argument_errors_before_the_device():
    """Null arguments and a non-positive image size or focal length are refused before the device
    is touched: no context is needed to see them, and nothing is created."""
    L, lib = load()
    cam = L.Camera(48, 36, 120.0, 120.0, 23.5, 17.5)
    h = ctypes.c_void_p(123)
    fake_ctx = None                                     # no device here: a null context is refused first
    assert lib.dsr_renderer_create(fake_ctx, None, ctypes.byref(cam), ctypes.byref(h)) < 0
    assert lib.dsr_renderer_create(None, None, None, None) < 0
    assert lib.dsr_renderer_destroy(None) == 0
    assert lib.dsr_renderer_stats_get(None, None) < 0
    st = L.RenderStats()
    assert lib.dsr_renderer_stats_get(None, ctypes.byref(st)) < 0
    assert lib.dsr_renderer_render(None, None, 0, None, None, None, None, None) < 0
