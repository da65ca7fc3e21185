"""Sphere-traced depth / instance / normal images on the GPU (dsr_renderer_*, SdfRenderer;
DESIGN.md §3.6b) against the numpy restatement of the algorithm (tests/render_oracle.py) over the
float64 oracle decoder.

Shapes: a 48 x 36 image.  Camera A (f = 300): the ball covers the image, 1728 rays = 27 full
tiles.  Camera B (f = 120): at this pose the ball's rectangle is 38 rows high,
more than the image's 36, so it cannot lie inside the image — it lies inside horizontally
(columns 5..43) and is clipped at the top and bottom: 1404 rays, no multiple of 64.  Camera C
(f = 100) is the rectangle strictly inside the image (33 x 33 = 1089 rays, no multiple of 64).
All three were confirmed against the caps with the oracle alone (fp32 against fp64 numpy): no
hit-mask difference, grazing share 1.0-4.5 %, worst err |m| / hit_eps 0.83.
"""
from __future__ import annotations

import numpy as np
import pytest

import render_oracle as RO
import synthetic as S
from conftest import assert_jac_close

pytestmark = pytest.mark.gpu

W, H = 48, 36
CAMS = {"A": RO.Camera(W, H, 300.0, 300.0, 23.5, 17.5),
        "B": RO.Camera(W, H, 120.0, 120.0, 23.5, 17.5),
        "C": RO.Camera(W, H, 100.0, 100.0, 23.5, 17.5)}
HIT_EPS = 1e-4
SCALES = (0.0, 0.1, 0.3, 0.3)


def pose(i, t=(0.1, -0.05, 15.0), scale=2.0):
    T = S.make_object(7 + i, n_pts=8, scale=scale, tz=15, perturb=0).t_true.copy()
    T[:3, 3] = t
    return T.astype(np.float32)


def code(i, n=64):
    scale = SCALES[i] if i < 4 else 1.0
    return (scale * np.random.default_rng(100 + i).standard_normal(n)).astype(np.float32)


_REN = {}


def renderer(dec, cam_name, code_len=64):
    """one SdfRenderer per (decoder, camera), kept for the module"""
    from reconstruct.optimizer import SdfRenderer

    key = (id(dec), cam_name)
    if key not in _REN:
        c = CAMS[cam_name]
        _REN[key] = (dec, SdfRenderer(dec, c.width, c.height, c.fx, c.fy, c.cx, c.cy, code_len=code_len))
    return _REN[key][1]


@pytest.fixture(scope="module")
def dec64(full_layers):
    from oracle.dsr_oracle import Decoder

    return Decoder(full_layers, 64, (4,), dtype=np.float64)


_ORACLE = {}


def oracle_trace(dec64, cam_name, i):
    """the float64 restatement's trace of (code i, pose i) on a camera, computed once"""
    if (cam_name, i) not in _ORACLE:
        _ORACLE[(cam_name, i)] = RO.trace_object(RO.decoder_sdf(dec64, code(i)), CAMS[cam_name], pose(i))
    return _ORACLE[(cam_name, i)]


def check_against_trace(out, tr, dec, z, label):
    """Hit masks differ on <= 2 % of the rays entering the ball; on commonly hit
    pixels with -g^.d^ >= 0.2, |lam_gpu - lam_oracle| <= 2.5 hit_eps / |m| (m = g.d, g the oracle
    gradient at the oracle hit: both tracers stop within hit_eps / |m| of the root, 0.5 for
    curvature and fp32-class decoding); grazing pixels are reported, their share <= 10 %."""
    depth, inst = out["depth"], out["instance"]
    u, v = tr.u, tr.v
    g_hit = inst[v, u] == 0
    assert np.array_equal(depth[v, u] > 0, g_hit)
    n_ball = int(tr.ball.sum())
    diff = int((g_hit != tr.hit).sum())
    both = g_hit & tr.hit
    x = tr.o + tr.lam[both, None] * tr.d[both]
    zz = np.broadcast_to(np.asarray(z, np.float64), (x.shape[0], z.shape[0]))
    _, g = dec.forward_jac(np.concatenate([zz, x], axis=1))
    g = g[:, -3:]
    m = (g * tr.d[both]).sum(1)
    cosang = m / np.linalg.norm(g, axis=1) / np.linalg.norm(tr.d[both], axis=1)
    ok = -cosang >= 0.2
    err = np.abs(depth[v, u][both].astype(np.float64) - tr.lam[both])
    ratio = err * np.abs(m) / HIT_EPS
    graze = float((~ok).mean())
    print(f"{label}: rays {u.size} ball {n_ball} hit gpu {int(g_hit.sum())} oracle {int(tr.hit.sum())} "
          f"mask diff {diff} grazing {graze:.4f} worst err|m|/eps {ratio[ok].max():.3f} "
          f"(grazing worst {ratio[~ok].max() if (~ok).any() else 0.0:.3f})")
    assert diff <= 0.02 * n_ball, (diff, n_ball)
    assert both.sum() > 50
    assert graze <= 0.10, graze
    assert np.all(ratio[ok] <= 2.5), float(ratio[ok].max())
    # everything outside the rectangle is empty
    mask = np.ones((H, W), bool)
    mask[v, u] = False
    assert np.all(depth[mask] == 0.0) and np.all(inst[mask] == -1)


@pytest.mark.parametrize("cam", ["A", "B", "C"])
@pytest.mark.parametrize("i", [0, 1, 2, 3])
def test_depth_against_the_fp64_oracle(gpu_decoder, dec64, cam, i):
    tr = oracle_trace(dec64, cam, i)
    out = renderer(gpu_decoder, cam).render([(pose(i), code(i))])
    rec = out["objects"][0]
    assert rec["status"] == 0 and tuple(rec["rect"]) == tuple(tr.rect) and rec["n_rays"] == tr.u.size
    if cam == "A":
        assert rec["n_rays"] == 1728 and rec["n_ball"] == 1728
    else:
        assert rec["n_rays"] % 64 != 0 and rec["n_rays"] == {"B": 1404, "C": 1089}[cam]
        assert (rec["rect"][0] > 0 and rec["rect"][2] < W - 1) and ((rec["rect"][1] > 0 and rec["rect"][3] < H - 1) == (cam == "C"))
    assert abs(rec["n_ball"] - int(tr.ball.sum())) <= 0.02 * tr.u.size
    assert rec["n_ball"] >= rec["n_hit"] + rec["n_unconverged"]
    assert rec["n_hit"] == rec["n_visible"] == int((out["instance"] == 0).sum())
    assert out["normals"] is None
    check_against_trace(out, tr, dec64, code(i), f"camera {cam} code {i}")


def test_nothing_to_hit(gpu_decoder, dec64):
    """code 1.0 N(0,1), seed 104: the fp64 tracer finds no surface in the ball"""
    tr = oracle_trace(dec64, "A", 4)
    assert tr.hit.sum() == 0 and tr.ball.sum() == 1728
    out = renderer(gpu_decoder, "A").render([(pose(4), code(4))], normals=True)
    assert np.all(out["depth"] == 0.0) and np.all(out["instance"] == -1) and np.all(out["normals"] == 0.0)
    rec = out["objects"][0]
    assert rec["n_hit"] == 0 and rec["n_visible"] == 0 and rec["n_ball"] == 1728 and rec["status"] == 0


def same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def rect_slice(rect):
    return slice(rect[1], rect[3] + 1), slice(rect[0], rect[2] + 1)


def test_bitwise_reproducible_and_independent_of_the_composition(gpu_decoder, monkeypatch):
    r = renderer(gpu_decoder, "B")
    # two objects side by side (scale 1: a third of the width each), rectangles disjoint
    left, right = pose(1, (-1.5, 0.2, 15.0), 1.0), pose(2, (1.6, -0.3, 15.0), 1.0)
    a = r.render([(left, code(1))], normals=True)
    b = r.render([(left, code(1))], normals=True)
    for k in ("depth", "instance", "normals"):
        assert same_bytes(a[k], b[k]), k
    ra = a["objects"][0]["rect"]
    assert a["objects"][0]["n_hit"] > 20
    pair = r.render([(left, code(1)), (right, code(2))], normals=True)
    rb = pair["objects"][1]["rect"]
    assert ra == pair["objects"][0]["rect"] and (ra[2] < rb[0] or rb[2] < ra[0])       # disjoint
    assert pair["objects"][1]["n_hit"] > 20
    sl = rect_slice(ra)
    for k in ("depth", "instance", "normals"):
        assert same_bytes(np.ascontiguousarray(a[k][sl]), np.ascontiguousarray(pair[k][sl])), k
    alone = r.render([(right, code(2))], normals=True)
    sl = rect_slice(rb)
    assert same_bytes(np.ascontiguousarray(alone["depth"][sl]), np.ascontiguousarray(pair["depth"][sl]))
    assert np.array_equal(alone["instance"][sl] + (alone["instance"][sl] >= 0), pair["instance"][sl])
    assert same_bytes(np.ascontiguousarray(alone["normals"][sl]), np.ascontiguousarray(pair["normals"][sl]))
    # three objects (two of them overlapping): all in one pass against one object per pass
    objs = [(left, code(1)), (right, code(2)), (pose(3, (1.2, 0.1, 14.0), 1.0), code(3))]
    one = r.render(objs, normals=True)
    assert r.stats()["n_passes"] == 1
    monkeypatch.setenv("DSR_TEST_HOOKS", "1")
    monkeypatch.setenv("DSR_RENDER_PASS_OBJ", "1")
    split = r.render(objs, normals=True)
    assert r.stats()["n_passes"] == 3
    monkeypatch.delenv("DSR_TEST_HOOKS")
    again = r.render(objs, normals=True)
    assert r.stats()["n_passes"] == 1                   # the hook is ignored without DSR_TEST_HOOKS=1
    for k in ("depth", "instance", "normals"):
        assert same_bytes(one[k], split[k]) and same_bytes(one[k], again[k]), k
    assert [o["n_hit"] for o in one["objects"]] == [o["n_hit"] for o in split["objects"]]
    assert [o["n_visible"] for o in one["objects"]] == [o["n_visible"] for o in split["objects"]]
    assert len(set(np.unique(one["instance"]).tolist()) - {-1}) == 3


def test_occlusion(gpu_decoder):
    """two objects on one line of sight, tz = 12 and tz = 18"""
    r = renderer(gpu_decoder, "B")
    near, far = pose(1, (0.0, 0.0, 12.0)), pose(2, (0.0, 0.0, 18.0))
    n_alone = r.render([(near, code(1))])
    f_alone = r.render([(far, code(2))])
    ab = r.render([(near, code(1)), (far, code(2))])
    ba = r.render([(far, code(2)), (near, code(1))])
    hn, hf = n_alone["instance"] == 0, f_alone["instance"] == 0
    both = hn & hf
    assert both.sum() > 50
    assert np.all(n_alone["depth"][both] < f_alone["depth"][both])
    assert np.all(ab["instance"][both] == 0) and same_bytes(ab["depth"][both], n_alone["depth"][both])
    only_f = hf & ~hn
    assert np.all(ab["instance"][only_f] == 1) and same_bytes(ab["depth"][only_f], f_alone["depth"][only_f])
    assert np.all(ab["instance"][~hn & ~hf] == -1)
    # swapping the input order changes only the indices
    assert same_bytes(ab["depth"], ba["depth"])
    hit = ab["instance"] >= 0
    assert np.array_equal(ab["instance"][hit], 1 - ba["instance"][hit]) and np.array_equal(hit, ba["instance"] >= 0)
    for out in (ab, ba):
        assert sum(o["n_visible"] for o in out["objects"]) == int((out["instance"] >= 0).sum())
        for k, o in enumerate(out["objects"]):
            assert o["n_visible"] == int((out["instance"] == k).sum()) and o["n_visible"] <= o["n_hit"]
    assert ab["objects"][1]["n_visible"] < ab["objects"][1]["n_hit"]          # the far object is occluded
    # the same object twice: the tie goes to the lower index
    tie = r.render([(near, code(1)), (near, code(1))])
    assert np.all(tie["instance"][tie["instance"] >= 0] == 0) and tie["objects"][1]["n_visible"] == 0


def device_points(cam, T, depth, u, v):
    """o + lam d in float32 with the device's association (dsr_render.hpp: rt_dir, rt_point)"""
    f = np.float32
    toc = RO.pose(T)[0].astype(f)
    rx = (u.astype(f) - f(cam.cx)) / f(cam.fx)
    ry = (v.astype(f) - f(cam.cy)) / f(cam.fy)
    d = np.stack([(rx * toc[k, 0] + ry * toc[k, 1]) + toc[k, 2] for k in range(3)], axis=1)
    lam = depth[v, u].astype(f)
    return np.stack([toc[k, 3] + lam * d[:, k] for k in range(3)], axis=1), toc


def check_normals(out, cam, T, odec, z, code_len=64):
    v, u = np.nonzero(out["instance"] == 0)
    assert v.size > 50
    x, toc = device_points(cam, T, out["depth"], u, v)
    zz = np.broadcast_to(np.asarray(z[:code_len], np.float32), (x.shape[0], code_len))
    _, g = odec.forward_jac(np.concatenate([zz, x], axis=1))
    n_ref = g[:, -3:].astype(np.float64) @ toc[:3, :3].astype(np.float64)      # R_oc^T g, row-wise
    n_ref /= np.linalg.norm(n_ref, axis=1, keepdims=True)
    n = out["normals"]
    assert n.dtype == np.float32 and n.shape == (H, W, 3)
    assert_jac_close(n[v, u], n_ref)
    assert np.abs(np.linalg.norm(n[v, u].astype(np.float64), axis=1) - 1.0).max() <= 1e-5
    assert np.all(n[out["instance"] < 0] == 0.0)
    # a surface seen from outside faces the camera: n . r < 0 (the sdf grows outwards)
    r = np.stack([(u - cam.cx) / cam.fx, (v - cam.cy) / cam.fy, np.ones(u.size)], axis=1)
    assert ((n[v, u] * r).sum(1) < 0).mean() > 0.95


@pytest.mark.parametrize("cam", ["A", "C"])
def test_normals_at_the_gpu_hit_points(gpu_decoder, oracle_dec, cam):
    r = renderer(gpu_decoder, cam)
    out = r.render([(pose(1), code(1))], normals=True)
    plain = r.render([(pose(1), code(1))])
    assert same_bytes(out["depth"], plain["depth"]) and same_bytes(out["instance"], plain["instance"])
    check_normals(out, CAMS[cam], pose(1), oracle_dec, code(1))


def test_skipped_objects_leave_the_others_unchanged(gpu_decoder):
    r = renderer(gpu_decoder, "B")
    a, b = pose(1, (-1.5, 0.2, 15.0), 1.0), pose(2, (1.2, 0.1, 14.0), 1.0)
    base = r.render([(a, code(1)), (b, code(2))], normals=True)
    off, nearp = pose(3, (40.0, 0.0, 15.0), 1.0), pose(0, (0.0, 0.0, 0.4), 1.0)
    mixed = r.render([(off, code(3)), (a, code(1)), (nearp, code(0)), (b, code(2)), (off, code(0))], normals=True)
    st = [o["status"] for o in mixed["objects"]]
    assert st == [1, 0, 2, 0, 1]
    for k in (0, 2, 4):
        o = mixed["objects"][k]
        assert o["n_rays"] == o["n_ball"] == o["n_hit"] == o["n_visible"] == 0 and tuple(o["rect"]) == (0, 0, -1, -1)
    remap = np.full(6, -1, np.int32)
    remap[1], remap[3] = 0, 1
    assert same_bytes(mixed["depth"], base["depth"]) and same_bytes(mixed["normals"], base["normals"])
    assert np.array_equal(remap[mixed["instance"]], base["instance"])
    for k, kb in ((1, 0), (3, 1)):
        assert dict(mixed["objects"][k]) == dict(base["objects"][kb])
    # only skipped objects, and no objects at all: an empty image
    for objs in ([(off, code(3)), (nearp, code(0))], []):
        e = r.render(objs, normals=True)
        assert np.all(e["depth"] == 0.0) and np.all(e["instance"] == -1) and np.all(e["normals"] == 0.0)
        assert r.stats()["decoded"] == 0 and r.stats()["steps_run"] == 0 and r.stats()["n_obj"] == len(objs)


def test_argument_errors(gpu_decoder):
    from reconstruct import _libdsr as L
    from reconstruct.optimizer import SdfRenderer

    for bad in ((0, 36, 100.0, 100.0), (48, -1, 100.0, 100.0), (48, 36, 0.0, 100.0), (48, 36, 100.0, -5.0)):
        with pytest.raises(L.DsrError):
            SdfRenderer(gpu_decoder, bad[0], bad[1], bad[2], bad[3], 23.5, 17.5)
    r = renderer(gpu_decoder, "C")
    good = [(pose(1), code(1))]
    ref = r.render(good)
    for kw in (dict(max_steps=257), dict(max_steps=-1), dict(hit_eps=-1e-4)):
        with pytest.raises(L.DsrError):
            r.render(good, **kw)
    row = pose(1)
    row[3, 3] = 2.0
    mirror = pose(1)
    mirror[:3, 0] *= -1.0
    flat = pose(1)
    flat[:3, :3] = 0.0
    for t in (row, mirror, flat):
        with pytest.raises(L.DsrError):
            r.render([(pose(2), code(2)), (t, code(1))])
    with pytest.raises(ValueError):
        r.render([(pose(1), code(1)[:63])])
    with pytest.raises(TypeError):
        r.render(good, steps=3)
    # null arguments at the C level
    ctx = gpu_decoder.ctx
    assert ctx.lib.dsr_renderer_render(r._h, None, 0, None, None, None, None, None) < 0
    assert ctx.lib.dsr_renderer_create(ctx.handle, gpu_decoder.handle, None, None) < 0
    assert same_bytes(r.render(good)["depth"], ref["depth"])          # the renderer survives its errors


def test_code32_decoder_renders():
    from deep_sdf.workspace import decoder_from_state
    from oracle.dsr_oracle import Decoder
    from test_gpu_code32 import SPECS32

    state = S.make_decoder(1234, SPECS32)
    dec = decoder_from_state(state, SPECS32)
    o64 = Decoder.from_state(state, SPECS32, dtype=np.float64)
    z = code(1, 32)
    tr = RO.trace_object(RO.decoder_sdf(o64, z), CAMS["C"], pose(1))
    out = renderer(dec, "C", code_len=32).render([(pose(1), z)], normals=True)
    check_against_trace(out, tr, o64, z, "code32 camera C")
    check_normals(out, CAMS["C"], pose(1), Decoder.from_state(state, SPECS32), z, code_len=32)


def test_use_tanh_decoder_renders_through_the_variant_kernels():
    from deep_sdf.workspace import decoder_from_state
    from oracle.dsr_oracle import Decoder
    from test_oracle_golden import _variant_specs

    specs = _variant_specs("tanh")
    state = S.make_decoder(1234, specs)
    dec = decoder_from_state(state, specs)
    assert not dec.info["lite_eligible"]                # a variant decoder: its own kernel instantiations
    o64 = Decoder.from_state(state, specs, dtype=np.float64)
    z = code(1)
    tr = RO.trace_object(RO.decoder_sdf(o64, z), CAMS["C"], pose(1))
    out = renderer(dec, "C").render([(pose(1), z)], normals=True)
    check_against_trace(out, tr, o64, z, "use_tanh camera C")
    check_normals(out, CAMS["C"], pose(1), Decoder.from_state(state, specs), z)


def test_stats(gpu_decoder, dec64):
    r = renderer(gpu_decoder, "B")
    objs = [(pose(1), code(1)), (pose(2, (0.3, 0.0, 17.0)), code(2))]
    one = r.render(objs, max_steps=1)
    s1 = r.stats()
    n_ball = sum(o["n_ball"] for o in one["objects"])
    live1 = sum(o["n_unconverged"] for o in one["objects"])            # still marching after step 0
    assert s1["decoded"] == n_ball and s1["steps_run"] == 1 and s1["max_live_last"] == n_ball and s1["n_passes"] == 1
    two = r.render(objs, max_steps=2)
    s2 = r.stats()
    assert s2["decoded"] == n_ball + live1 and s2["steps_run"] == 2 and s2["max_live_last"] == live1
    assert [o["n_ball"] for o in two["objects"]] == [o["n_ball"] for o in one["objects"]]
    out = r.render(objs)
    s = r.stats()
    assert s["n_obj"] == 2 and 2 < s["steps_run"] <= 48
    for o in out["objects"]:
        assert o["n_ball"] >= o["n_hit"] + o["n_unconverged"]
        assert o["n_rays"] >= o["n_ball"] > 0
    # decoded = the sum over steps of the live rays: the restatement's count, up to the rays whose
    # fp32 march differs from the fp64 one (the hit-mask cap, 2 %)
    ref = sum(sum(RO.trace_object(RO.decoder_sdf(dec64, z), CAMS["B"], t).live_per_step) for t, z in objs)
    assert abs(s["decoded"] - ref) <= 0.02 * ref, (s["decoded"], ref)
    assert n_ball <= s["decoded"] <= n_ball * s["steps_run"]
    assert s["setup_ms"] > 0 and s["march_ms"] > 0 and s["resolve_ms"] > 0
    few = r.render(objs, max_steps=4)
    assert r.stats()["steps_run"] == 4 and sum(o["n_unconverged"] for o in few["objects"]) > 0
    assert sum(o["n_hit"] for o in few["objects"]) <= sum(o["n_hit"] for o in out["objects"])


def test_passes_split_by_ray_capacity(gpu_decoder):
    """three objects whose rectangles are the whole image: the ray buffers (2 W H) hold two, so the
    third runs in a second pass against the persisting pixel keys; the composite is the per-pixel
    nearest of the three objects rendered alone"""
    r = renderer(gpu_decoder, "A")
    objs = [(pose(1, (0.1, -0.05, 15.0)), code(1)), (pose(2, (-0.2, 0.1, 14.0)), code(2)), (pose(3, (0.3, 0.0, 13.5)), code(3))]
    out = r.render(objs)
    assert r.stats()["n_passes"] == 2 and [o["n_rays"] for o in out["objects"]] == [1728] * 3
    alone = [r.render([o]) for o in objs]
    assert all(r_["objects"][0]["n_hit"] > 100 for r_ in alone)
    d = np.stack([np.where(a_["instance"] == 0, a_["depth"], np.inf) for a_ in alone])
    win = d.argmin(0)
    hit = np.isfinite(d.min(0))
    assert np.array_equal(out["instance"] >= 0, hit) and np.array_equal(out["instance"][hit], win[hit])
    assert same_bytes(out["depth"][hit], d.min(0)[hit].astype(np.float32))
    assert [o["n_hit"] for o in out["objects"]] == [a_["objects"][0]["n_hit"] for a_ in alone]
