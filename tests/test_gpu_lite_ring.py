"""The lite kernel's pinned B ring (DSR_LITE_VARIANT 3544, dsr_mlp_lite.hpp: gemm_lite_r) against
the schedule it replaces (1496, gemm_lite_x): the same MFMAs on the same operands in the same k
order, so every lite value, and with it every class, count and record, is bitwise equal.

The batch API hands out no copy of a batch's `dense` buffer, so the lite values themselves are
compared where the library does expose them: the mesher's sign pass runs the same kernel
(lite_schedule()) over a grid and dsr_mesher_peek returns its output.  The batch cases compare the
records and the counters that depend on the lite values only (samples decoded, band and audit
samples, the largest observed |lite - exact|).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import synthetic as S

pytestmark = pytest.mark.gpu

OLD, NEW = "1496", "3544"


def _params(iters, M=None):
    from reconstruct import _libdsr as L

    cfg = dict(S.KITTI_OPTIM, joint_optim=dict(S.KITTI_OPTIM["joint_optim"], num_iterations=iters))
    if M is not None:
        cfg["num_depth_samples"] = M
    return L.optim_params(cfg)


def _run(dec, params, objs):
    """One batch over objs = [(t_cam_obj, pts, rays, depth)]: (records as uint32, lite counters)."""
    from reconstruct import _libdsr as L

    lib, ctx = dec.ctx.lib, dec.ctx
    n = len(objs)
    keep, ins = [], (L.ObjectIn * n)()
    for i, (t, pts, rays, depth) in enumerate(objs):
        arrs = [np.ascontiguousarray(a, np.float32) for a in (pts, rays, depth)]
        keep += arrs
        r = L.ObjectIn()
        r.t_cam_obj[:] = np.asarray(t, np.float32).reshape(-1).tolist()
        r.pts, r.n_pts = L.fptr(arrs[0]), arrs[0].shape[0]
        r.rays, r.n_rays = L.fptr(arrs[1]), arrs[1].shape[0]
        r.depth, r.n_depth = L.fptr(arrs[2]), arrs[2].shape[0]
        r.code = None
        r.pose_is_obj_cam = 0
        ins[i] = r
    h = C.c_void_p()
    ctx.check(lib.dsr_batch_create(ctx.handle, dec.handle, C.byref(params), n, ins, C.byref(h)), "create")
    try:
        outs = (L.ObjectOut * n)()
        ctx.check(lib.dsr_batch_run(h), "run")
        ctx.check(lib.dsr_batch_download(h, outs), "download")
        st = L.Stats()
        ctx.check(lib.dsr_batch_stats(h, C.byref(st)), "stats")
        rec = np.array([list(o.t_cam_obj) + list(o.code) + [o.loss, o.is_good, o.iters_done] for o in outs],
                       np.float32)
        assert st.lite_broken_blocks == 0, L.lite_diag(lib, h)
        return rec.view(np.uint32), dict(lite=st.lite, variant=st.lite_variant, groups=st.n_groups,
                                         fwd=st.fwd_points, refine=st.refine_points, audit=st.audit_points,
                                         err=st.lite_max_err)
    finally:
        lib.dsr_batch_destroy(h)


def _both(dec, monkeypatch, params, objs, **env):
    out = {}
    monkeypatch.setenv("DSR_TEST_HOOKS", "1")       # kernel switches are test hooks
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for v in (OLD, NEW):
        monkeypatch.setenv("DSR_LITE_VARIANT", v)
        out[v] = _run(dec, params, objs)
        assert out[v][1]["lite"] == 1 and out[v][1]["variant"] == int(v), out[v][1]
    return out


def _kitti(i, n_pts):
    o = S.kitti_object(i, n_pts=n_pts)
    return (o.t_cam_obj, o.pts, o.rays, o.depth)


def test_ring_records_bitwise_one_object(gpu_decoder, monkeypatch):
    """One object of 256 points, 3 GN iterations, KITTI parameters: the records and every counter
    the lite values decide are those of the previous schedule, bit for bit."""
    out = _both(gpu_decoder, monkeypatch, _params(3), [_kitti(0, 256)])
    (ro, so), (rn, sn) = out[OLD], out[NEW]
    print("\n1496:", so, "\n3544:", sn)
    assert so["fwd"] > 0 and so["refine"] > 0
    assert np.array_equal(ro, rn)
    assert {k: v for k, v in so.items() if k != "variant"} == {k: v for k, v in sn.items() if k != "variant"}


@pytest.mark.parametrize("d", [2, 5, 6, 9])
def test_ring_dense_bitwise_on_grids(gpu_decoder, monkeypatch, d):
    """The lite values themselves (the kernel's `dense` output) on d^3-point grids of three codes:
    8 and 125 points are one partial tile, 216 = 128 + 88 and 729 = 5 x 128 + 89 end in one; every
    tile runs lin4 (14 k steps) and the 16-step layers, so the shortened last k step is covered at
    both depths."""
    from reconstruct.optimizer import MeshExtractor

    mex = MeshExtractor(gpu_decoder, 64, d)
    codes = [(s * np.random.default_rng(100 + i).standard_normal(64)).astype(np.float32)
             for i, s in enumerate((0.0, 0.1, 0.3))]
    vols = {}
    monkeypatch.setenv("DSR_TEST_HOOKS", "1")
    for v in (OLD, NEW):
        monkeypatch.setenv("DSR_LITE_VARIANT", v)
        mex.extract_meshes_from_codes(codes)
        st = mex.stats()
        assert st["sign_pass"] == 1 and st["lite_broken_blocks"] == 0, st
        assert st["lite_tiles"] == 3 * ((d ** 3 + 127) // 128), st
        vols[v] = [mex.peek(s) for s in range(3)]
    for s in range(3):
        lo, fo, _ = vols[OLD][s]
        ln, fn, _ = vols[NEW][s]
        assert np.isfinite(lo).all()
        assert lo.tobytes() == ln.tobytes(), (d, s)
        assert fo.tobytes() == fn.tobytes(), (d, s)


def _tiny(n_rays, n_fg=16, scale=2.0, tz=15.0):
    """An object whose every ray carries exactly one in-ball sample at 3 depth samples: the rays
    pass the object centre at 0.2 object units (the end samples, at depth tz -+ scale, lie at
    radius sqrt(1.04) > 1; the middle one at 0.2), so the ray count is the sample count."""
    o = S.make_object(77, n_pts=64, n_bg=0, scale=scale, tz=tz, upright=True, perturb=0.0)
    ang = np.linspace(0.0, 2.0 * np.pi, n_rays, endpoint=False)
    off = 0.2 * scale / tz
    rays = np.stack([off * np.cos(ang), off * np.sin(ang), np.ones(n_rays)], axis=1).astype(np.float32)
    depth = np.full(min(n_fg, n_rays), tz - 0.5 * scale, np.float32)
    return (o.t_cam_obj, o.pts, rays, depth)


@pytest.mark.parametrize("n", [1, 127, 128, 129])
def test_ring_partial_tiles(gpu_decoder, monkeypatch, n):
    """Tiles of 127, 128 and 128 + 1 samples, reached through the ray count of a tiny object (one
    in-ball sample per ray, one GN iteration, so samples decoded == rays), and the 1-sample
    object, which the render pass rejects for fewer than 10 in-ball samples before any decode:
    equal records and counters, no broken block."""
    out = _both(gpu_decoder, monkeypatch, _params(1, M=3), [_tiny(n)])
    (ro, so), (rn, sn) = out[OLD], out[NEW]
    print("\nrays %d 1496: %s\n          3544: %s" % (n, so, sn))
    assert so["fwd"] == (n if n >= 10 else 0), so
    assert np.array_equal(ro, rn)
    assert {k: v for k, v in so.items() if k != "variant"} == {k: v for k, v in sn.items() if k != "variant"}


def test_ring_object_groups(gpu_decoder, monkeypatch):
    """8 objects of 128 points on 2 and on 4 object groups (concurrent streams, so several lite
    grids at once): records bitwise those of the one-group run, old and new schedule alike.
    (The number of samples decoded belongs to the group count — one-group batches run their
    render passes over ray chunks, DESIGN.md §3.8 — so the counters are compared between the
    two schedules at each group count, not across group counts.)"""
    objs = [_kitti(i, 128) for i in range(8)]
    p = _params(3)
    ref = None
    for g in ("1", "2", "4"):
        out = _both(gpu_decoder, monkeypatch, p, objs, DSR_STREAMS=g)
        (ro, so), (rn, sn) = out[OLD], out[NEW]
        assert so["groups"] == sn["groups"] == int(g), (so, sn)
        if ref is None:
            ref = ro
        assert np.array_equal(ro, ref), g
        assert np.array_equal(rn, ref), g
        assert so["fwd"] > 0 and so["refine"] > 0
        assert {k: v for k, v in so.items() if k != "variant"} == {k: v for k, v in sn.items() if k != "variant"}, g
