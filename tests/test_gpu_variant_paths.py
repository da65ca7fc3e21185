"""The variant decoders (use_tanh / xyz_in_all / LayerNorm: their own instantiations of the
split-fp16 kernels, and for LayerNorm the per-object-group Jacobian workspaces ``ctx->lnws[g]``)
through the entry points that so far only saw the shipped topology: multi-object batches on one
and several object groups, graph capture and replay, ``SceneSdf``, ``SdfRenderer``, the batch
mesher and ``reconstruct_objects_views``.  Shapes and helpers are the existing modules' own.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import decoder_check as DC
import scene_oracle as SO
import synthetic as S
from conftest import make_cfg

pytestmark = pytest.mark.gpu

_DECS = {}


def gpu_dec(name):
    from deep_sdf.workspace import decoder_from_state

    if name not in _DECS:
        _DECS[name] = decoder_from_state(DC.decoder_state(name), DC.decoder_specs(name))
        assert not _DECS[name].info["lite_eligible"]        # a variant decoder never takes the lite pass
    return _DECS[name]


def _opt(dec, optim, data_type, iters):
    from reconstruct.optimizer import Optimizer

    return Optimizer(dec, make_cfg(dict(optim, joint_optim=dict(optim["joint_optim"], num_iterations=iters)), data_type))


def _five_objects():
    objs = []
    for i in range(5):
        o = S.make_object(300 + i, n_pts=200 + 97 * i, n_bg=50 + 10 * i, scale=1.0, tz=3.0, upright=False)
        objs.append((o.t_cam_obj, o.pts, o.rays, o.depth, None))
    return objs


@pytest.mark.parametrize("streams", ["1", "4"])
@pytest.mark.parametrize("name", ["ln", "xyz", "tanh"])
def test_batch_equals_single(name, streams, monkeypatch):
    """test_gpu_parity.py's test_batch_equals_single on a variant decoder: five objects, one and
    four object groups (LayerNorm: a Jacobian workspace per group), batch == singles, bitwise."""
    monkeypatch.setenv("DSR_STREAMS", streams)
    monkeypatch.setenv("DSR_TEST_HOOKS", "1")
    monkeypatch.setenv("DSR_RENDER_PASSES", "16,24")
    opt = _opt(gpu_dec(name), S.REDWOOD_OPTIM, "Redwood", 2)
    objs = _five_objects()
    batch, tr = opt.reconstruct_objects(objs, trace=True)
    assert any(r["is_good"] for r in batch)
    for i, ob in enumerate(objs):
        (single,), tr1 = opt.reconstruct_objects([ob], trace=True)
        assert batch[i]["is_good"] == single["is_good"]
        if single["is_good"]:
            assert np.array_equal(batch[i]["t_cam_obj"], single["t_cam_obj"])
            assert np.array_equal(batch[i]["code"], single["code"])
            assert batch[i]["loss"] == single["loss"]
        for key in ("H", "b", "loss", "n_valid", "k"):
            assert np.array_equal(tr[i][key], tr1[0][key]), (i, key)


def test_layernorm_graph_replay_bitwise(monkeypatch):
    """test_gpu_parity.py's test_graph_replay_bitwise on the LayerNorm decoder: an eager run, the
    captured run and a replay give the same records and counters, and so does DSR_GRAPH=0."""
    import bench
    from reconstruct import _libdsr as L

    dec = gpu_dec("ln")
    lib, ctx = dec.ctx.lib, dec.ctx
    params = L.optim_params(dict(S.REDWOOD_OPTIM, joint_optim=dict(S.REDWOOD_OPTIM["joint_optim"], num_iterations=2)))
    sig = []
    for graph in ("1", "0"):
        monkeypatch.setenv("DSR_GRAPH", graph)
        h, keep = bench.make_batch(dec, params, 6, 4000, n_pts=512)
        try:
            for run in range(3 if graph == "1" else 1):
                outs = (L.ObjectOut * 6)()
                ctx.check(lib.dsr_batch_run(h), "run")
                ctx.check(lib.dsr_batch_download(h, outs), "download")
                st = L.Stats()
                ctx.check(lib.dsr_batch_stats(h, ctypes.byref(st)), "stats")
                replay = graph == "1" and run > 0
                assert (st.fwd_launches == 0) if replay else (st.fwd_ms > 0 and st.jac_ms > 0)
                sig.append((np.array([list(o.t_cam_obj) + list(o.code) + [o.loss, o.is_good] for o in outs], np.float32),
                            st.fwd_points, st.jac_points, st.inball_points))
        finally:
            lib.dsr_batch_destroy(h)
    assert sig[0][0][:, -1].any()
    for s in sig[1:]:
        assert np.array_equal(s[0], sig[0][0]) and s[1:] == sig[0][1:]


@pytest.mark.parametrize("name", ["ln", "xyz"])
def test_scene_sdf(name):
    """400 points, four objects, grad=True: the composite against the fp64 restatement
    (test_gpu_scene.check_against_oracle), values bitwise sdf_eval's on the same tiles, and the
    world gradient held like a Jacobian's xyz columns by tests/decoder_check.py's rule — scaled by
    the largest |fp64 entry|, no floor of 1, every winner judged, a point with near units against
    its admissible ReLU assignments — within r_J of the family times the fp32 numpy oracle's own
    worst error on the same points (its transform s A^T g in fp32 as well, as the device's)."""
    import test_gpu_scene as TS
    from reconstruct.optimizer import sdf_eval

    dec = gpu_dec(name)
    d32, d64 = DC.oracle_pair(name)
    objs, pts = SO.scene_objects(), SO.scene_points(400)
    ref = SO.query([SO.decoder_sdf(d64, z) for _, z in objs], [t for t, _ in objs], pts,
                   [SO.decoder_grad(d64, z) for _, z in objs])
    assert tuple(r.n_in for r in ref.objects) == SO.COUNTS[400]
    d = np.sort(ref.d_all, axis=0)
    two = np.isfinite(d[1])
    assert (d[1][two] - d[0][two]).min() >= 2 * TS.F_TOL * max(SO.SCALES)
    sc = TS.scene(dec)
    sc.set_objects(objs)
    out = sc.query(pts, grad=True)
    peeks = [sc.peek(i) for i in range(4)]
    TS.check_against_oracle(out, peeks, ref, f"{name} scene")
    hit = out["obj"] >= 0
    assert np.all(out["grad"][~hit] == 0.0)
    scale = float(np.abs(ref.grad[hit]).max())
    worst, worst32, n_kink = 0.0, 0.0, 0
    for i, (t, z) in enumerate(objs):
        idx, x, f = peeks[i]
        assert TS.same_bytes(f, sdf_eval(dec, z, x))                     # the same tiles, so the same values
        mine = np.nonzero(out["obj"][idx] == i)[0]
        T = DC.Truth(d32, d64, DC.make_inp(z, x))
        A, _, s = SO.pose(t)
        pos = {int(p): a for a, p in enumerate(T.kink_idx)}
        g32 = np.float32(s) * (T.J32[:, -3:] @ A.astype(np.float32))
        got = out["grad"][idx]
        for a in mine:
            if T.left_out[a]:
                continue
            cands = [T.J[a, -3:]]
            if a in pos:
                n_kink += 1
                cands += [T.alt_J[c, pos[a], -3:] for c in range(1, 1 << DC.K_MAX) if not np.isnan(T.alt_y[c, pos[a]])]
            world = [s * (g @ A) for g in cands]
            worst = max(worst, min(np.abs(got[a] - w).max() for w in world) / scale)
            worst32 = max(worst32, min(np.abs(g32[a] - w).max() for w in world) / scale)
    r_J = DC.R[DC.family(name)][1]
    print(f"{name} scene gradient: winners {int(hit.sum())} ({n_kink} with near units), scale {scale:.3f}, worst "
          f"{worst:.2e}, fp32 oracle {worst32:.2e}, ratio {worst / worst32:.2f} (bound {r_J})")
    assert worst <= r_J * worst32


@pytest.mark.parametrize("name", ["ln", "xyz"])
def test_renderer(name):
    """Camera C with normals, as test_gpu_render.py's use_tanh case."""
    import render_oracle as RO
    import test_gpu_render as TR

    dec = gpu_dec(name)
    d32, d64 = DC.oracle_pair(name)
    z = TR.code(1)
    tr = RO.trace_object(RO.decoder_sdf(d64, z), TR.CAMS["C"], TR.pose(1))
    out = TR.renderer(dec, "C").render([(TR.pose(1), z)], normals=True)
    TR.check_against_trace(out, tr, d64, z, f"{name} camera C")
    TR.check_normals(out, TR.CAMS["C"], TR.pose(1), d32, z)


@pytest.mark.parametrize("name", ["ln", "xyz"])
def test_batch_mesher(name):
    """d = 16, three codes: every mesh bitwise the per-code mesher's; no sign pass for a decoder
    that is not lite-eligible."""
    import test_gpu_mesh_batch as MB

    dec = gpu_dec(name)
    mex = MB.mex_for(dec, 16)
    meshes = mex.extract_meshes_from_codes(MB.make_codes(3))
    st = mex.stats()
    assert st["n_codes"] == 3 and st["sign_pass"] == 0 and st["exact_tiles"] == st["all_tiles"]
    assert any(m.vertices.shape[0] > 0 for m in meshes)
    MB.assert_same(meshes, dec, 16, 0.0)


def test_layernorm_one_view_is_the_single_view_path_bitwise():
    opt = _opt(gpu_dec("ln"), S.REDWOOD_OPTIM, "Redwood", 2)
    single, tied = [], []
    for i in range(4):
        o = S.make_object(300 + i, n_pts=200 + 97 * i, n_bg=50 + 10 * i, scale=1.0, tz=3.0, upright=False)
        single.append((o.t_cam_obj, o.pts, o.rays, o.depth, None))
        tied.append((o.t_cam_obj, [(np.eye(4), o.pts, o.rays, o.depth)], None))
    r0, t0 = opt.reconstruct_objects(single, trace=True)
    r1, t1 = opt.reconstruct_objects_views(tied, trace=True)
    assert any(r["is_good"] for r in r0)
    for i in range(4):
        assert r0[i]["is_good"] == r1[i]["is_good"]
        if r0[i]["is_good"]:
            assert r1[i]["fail_view"] == -1
            assert np.array_equal(r1[i]["t_cam_obj"], r0[i]["t_cam_obj"])
            assert np.array_equal(r1[i]["code"], r0[i]["code"])
            assert r1[i]["loss"] == r0[i]["loss"] and r1[i]["iters_done"] == r0[i]["iters_done"] == 2
        for key in ("H", "b", "loss", "n_valid", "k"):
            assert np.array_equal(t1[i][key], t0[i][key]), (i, key)
