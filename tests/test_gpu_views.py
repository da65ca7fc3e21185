"""Joint reconstruction of one object from several views (dsr_reconstruct_views, include/dsr.h;
DESIGN.md "Several views of one object") on the device.

One code and one pose are fitted to the pooled residuals of V cameras: every view is an ordinary
batch member, k_solve_views pools the members' normal-equation sums and k_views_pose re-derives
their poses from the reference view's.  Checked here: one view is the old path bit for bit; a
step equals the numpy restatement (tests/views_oracle.py) in fp64 within the single-view bounds
of test_gpu_parity.py::test_trajectory_shadowing_and_final; objects of a tied batch do not
interact, however the batch is split over streams; the trajectory obeys the one update rule;
the reference's failures per object; an audit violation in a view redoes the object exactly;
bad arguments are errors.

Shapes: 3 views of 130 / 143 / 156 points (two or three 64-point Jacobian tiles with ragged
tails) and 40 background rays each; seeds 700-702.
"""
from __future__ import annotations

import numpy as np
import pytest

import synthetic as S
from conftest import make_cfg
from views_oracle import gn_step_views, oracle_views

pytestmark = pytest.mark.gpu

REDWOOD = dict(scale=1.0, tz=3.0, upright=False)
KITTI = dict(scale=2.0, tz=15.0, upright=True)
CASES = {"Redwood": (S.REDWOOD_OPTIM, REDWOOD), "KITTI": (S.KITTI_OPTIM, KITTI)}
EPS32 = 2.0 ** -24


def _opt(dec, optim, data_type, iters):
    from reconstruct.optimizer import Optimizer

    optim = dict(optim, joint_optim=dict(optim["joint_optim"], num_iterations=iters))
    return Optimizer(dec, make_cfg(optim, data_type))


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-30))


def step_err(dx, dx_ref, H):
    """GN step error in the H-norm (test_gpu_parity.py)."""
    d = np.asarray(dx, np.float64) - dx_ref
    H = np.asarray(H, np.float64)
    return float(np.sqrt(max(d @ H @ d, 0.0) / max(dx_ref @ H @ dx_ref, 1e-300)))


@pytest.fixture(scope="module")
def dec64(oracle_dec):
    return type(oracle_dec)(oracle_dec.layers, dtype=np.float64)


_objects = {}


def views_object(seed, kind, n_views=3):
    key = (seed, kind, n_views)
    if key not in _objects:
        _objects[key] = S.make_object_views(seed, n_views, n_pts=130, n_bg=40, **CASES[kind][1])
    return _objects[key]


def assert_step_matches(tg, e, dec64, optim, T, z, views, what=""):
    """Iteration e of a GPU trace against gn_step_views in fp64 from the state (T, z), with the
    single-view bounds of test_trajectory_shadowing_and_final: the counts within 2 per view
    (the trace holds their sums), sdf_loss 5e-5 relative, render_loss 1e-5 relative plus 0.09 / K
    per render point that flips, rel(H) 5e-3, the step 2e-2 in the H-norm."""
    from oracle import dsr_oracle as O

    P = O.OptimParams.from_cfg(optim)
    V = len(views)
    tro, Tn, zn = gn_step_views(dec64, P, np.asarray(T, np.float64), np.asarray(z, np.float64),
                                [(v[0], v[1].astype(np.float64), v[2].astype(np.float64),
                                  v[3].astype(np.float64), v[4]) for v in views])
    assert Tn is not None, what
    K, nv = sum(tro.k), sum(tro.n_valid)
    dk, dn = abs(int(tg["k"][e]) - K), abs(int(tg["n_valid"][e]) - nv)
    flips = max(dk, 2)
    es = abs(tg["sdf_loss"][e] - tro.sdf_loss) / abs(tro.sdf_loss)
    er = abs(tg["render_loss"][e] - tro.render_loss)
    rh, se = rel(tg["H"][e], tro.H), step_err(tg["dx"][e], tro.dx, tro.H)
    print(f"{what} e={e}: K {int(tg['k'][e])}/{K} per view {tro.k}, n_valid {int(tg['n_valid'][e])}/{nv} "
          f"per view {tro.n_valid}, sdf rel {es:.2e}, render abs {er:.2e} (bound "
          f"{1e-5 * abs(tro.render_loss) + flips * 0.09 / K:.2e}), rel(H) {rh:.2e}, step_err {se:.2e}")
    assert dk <= 2 * V and dn <= 2 * V, what
    assert es <= 5e-5, what
    assert er <= 1e-5 * abs(tro.render_loss) + flips * 0.09 / K, what
    assert rh <= 5e-3, what
    assert se <= 2e-2, what
    return tro


def test_one_view_is_the_single_view_path_bitwise(gpu_decoder):
    opt = _opt(gpu_decoder, S.REDWOOD_OPTIM, "Redwood", 3)
    single, tied = [], []
    for i in range(4):
        o = S.make_object(300 + i, n_pts=200 + 97 * i, n_bg=50 + 10 * i, **REDWOOD)
        single.append((o.t_cam_obj, o.pts, o.rays, o.depth, None))
        tied.append((o.t_cam_obj, [(np.eye(4), o.pts, o.rays, o.depth)], None))
    r0, t0 = opt.reconstruct_objects(single, trace=True)
    r1, t1 = opt.reconstruct_objects_views(tied, trace=True)
    for i in range(4):
        assert r0[i]["is_good"] and r1[i]["is_good"] and r1[i]["fail_view"] == -1
        assert np.array_equal(r1[i]["t_cam_obj"], r0[i]["t_cam_obj"])
        assert np.array_equal(r1[i]["code"], r0[i]["code"])
        assert r1[i]["loss"] == r0[i]["loss"] and r1[i]["iters_done"] == r0[i]["iters_done"] == 3
        for key in ("H", "b", "loss", "n_valid", "k"):
            assert np.array_equal(t1[i][key], t0[i][key]), (i, key)


@pytest.mark.parametrize("kind", ["Redwood", "KITTI"])
@pytest.mark.parametrize("seed", [700, 701, 702])
def test_one_step_matches_the_fp64_restatement(gpu_decoder, dec64, seed, kind):
    optim = CASES[kind][0]
    ob = views_object(seed, kind)
    opt = _opt(gpu_decoder, optim, kind, 1)
    (r,), (t,) = opt.reconstruct_objects_views([(ob.t_cam_obj, ob.views, None)], trace=True)
    assert r["is_good"] and r["iters_done"] == 1 and r["fail_view"] == -1
    T0 = np.linalg.inv(ob.t_cam_obj.astype(np.float64))
    # the start state, in the reference view (an fp32 inverse: n eps cond, cond of these poses < 300)
    assert rel(t["t_obj_cam"][0], T0) <= 1e-4
    tro = assert_step_matches(t, 0, dec64, optim, t["t_obj_cam"][0], t["z"][0], oracle_views(ob),
                              f"{kind} {seed}")
    assert len(tro.k) == 3 and min(tro.k) > 0                   # every view contributes render points


def test_upright_prior_acts_once_in_the_reference_view(gpu_decoder, dec64):
    """make_object's start poses are exactly upright (the prior's residual is 0 there), so tilt
    one by 0.03 rad about the object's x axis: with k4 = 1e7 the prior then dominates b[3:6], and
    the step still matches the restatement, which evaluates it once, at the reference view's T."""
    from oracle import dsr_oracle as O

    ob = views_object(701, "KITTI")
    c, s = np.cos(0.03), np.sin(0.03)
    tilt = np.array([[1, 0, 0, 0], [0, c, -s, 0], [0, s, c, 0], [0, 0, 0, 1]], np.float64)
    t_cam_obj = (ob.t_cam_obj.astype(np.float64) @ tilt).astype(np.float32)
    opt = _opt(gpu_decoder, S.KITTI_OPTIM, "KITTI", 1)
    (r,), (t,) = opt.reconstruct_objects_views([(t_cam_obj, ob.views, None)], trace=True)
    assert r["is_good"]
    j_rot, r_rot = O.compute_rotation_loss_sim3(np.asarray(t["t_obj_cam"][0], np.float64))
    assert r_rot > 1e-5 and np.abs(j_rot).max() > 1e-3
    assert_step_matches(t, 0, dec64, S.KITTI_OPTIM, t["t_obj_cam"][0], t["z"][0], oracle_views(ob), "tilted")


def test_trajectory_shadows_the_restatement(gpu_decoder, dec64):
    ob = views_object(700, "Redwood")
    opt = _opt(gpu_decoder, S.REDWOOD_OPTIM, "Redwood", 3)
    opt1 = _opt(gpu_decoder, S.REDWOOD_OPTIM, "Redwood", 1)
    (r,), (t,) = opt.reconstruct_objects_views([(ob.t_cam_obj, ob.views, None)], trace=True)
    assert r["is_good"] and r["iters_done"] == 3
    assert np.isfinite(t["loss"]).all()
    for e in (0, 2):
        T, z = t["t_obj_cam"][e], t["z"][e]
        (rg,), (tg,) = opt1.reconstruct_objects_views([(T, ob.views, z)], trace=True, pose_is_obj_cam=True)
        assert rg["is_good"]
        assert tg["loss"][0] == t["loss"][e]                    # re-running a state is deterministic
        assert np.array_equal(tg["H"][0], t["H"][e]) and int(tg["k"][0]) == int(t["k"][e])
        assert_step_matches(tg, 0, dec64, S.REDWOOD_OPTIM, T, z, oracle_views(ob), f"shadow {e}")


@pytest.mark.parametrize("streams", ["1", "2", "3", "4"])
def test_tied_batch_equals_objects_alone(gpu_decoder, streams, monkeypatch):
    """Objects with 3, 1, 2 and 3 views in one batch (9 members) equal each object run alone,
    bitwise, however the members are split into object groups on concurrent streams: group
    boundaries fall on object boundaries, so a tie never straddles two streams."""
    monkeypatch.setenv("DSR_STREAMS", streams)
    monkeypatch.setenv("DSR_TEST_HOOKS", "1")
    monkeypatch.setenv("DSR_RENDER_PASSES", "16,24")            # (as test_batch_equals_single pins it)
    opt = _opt(gpu_decoder, S.REDWOOD_OPTIM, "Redwood", 3)
    objs = []
    for seed, nv in ((700, 3), (701, 1), (702, 2), (701, 3)):
        ob = views_object(seed, "Redwood", nv)
        objs.append((ob.t_cam_obj, ob.views, None))
    batch, tr = opt.reconstruct_objects_views(objs, trace=True)
    assert opt.last_stats.n_groups == min(int(streams), 4)
    for i, ob in enumerate(objs):
        (single,), (tr1,) = opt.reconstruct_objects_views([ob], trace=True)
        assert batch[i]["is_good"] and single["is_good"]
        assert np.array_equal(batch[i]["t_cam_obj"], single["t_cam_obj"])
        assert np.array_equal(batch[i]["code"], single["code"])
        assert batch[i]["loss"] == single["loss"]
        for key in ("H", "b", "loss", "k"):
            assert np.array_equal(tr[i][key], tr1[key]), (i, key)


def test_views_follow_the_one_update(gpu_decoder):
    """T_{e+1} = exp_sim3(lr dx_e) T_e for the traced states and the returned pose: the views'
    poses are derived from this T every iteration, never updated on their own.  Bound: the fp32
    exp_sim3 and 4x4 product against the oracle's in fp64 — 16 unit roundoffs of the product's
    terms |dT| |T| (each entry of dT carries a handful of roundings, the product 4 + 3 more)."""
    from oracle import dsr_oracle as O

    ob = views_object(702, "Redwood")
    opt = _opt(gpu_decoder, S.REDWOOD_OPTIM, "Redwood", 3)
    (r,), (t,) = opt.reconstruct_objects_views([(ob.t_cam_obj, ob.views, None)], trace=True)
    assert r["is_good"]
    lr = S.REDWOOD_OPTIM["joint_optim"]["learning_rate"]
    for e in range(3):
        T = np.asarray(t["t_obj_cam"][e], np.float64)
        dT = O.exp_sim3(lr * np.asarray(t["dx"][e][:7], np.float64))
        ref = dT @ T
        tol = 16 * EPS32 * (np.abs(dT) @ np.abs(T))
        if e < 2:
            assert (np.abs(t["t_obj_cam"][e + 1] - ref) <= tol).all(), e
            assert np.abs(t["z"][e + 1] - (t["z"][e] + np.float32(lr) * t["dx"][e][7:])).max() <= 2 * EPS32
        else:
            # the returned t_cam_obj is the fp32 inverse of the last T (optimizer.py:202): as a
            # residual, |X T - I| within 16 unit roundoffs of |X| |T| (LU of a 4x4)
            X = np.asarray(r["t_cam_obj"], np.float64)
            assert (np.abs(X @ ref - np.eye(4)) <= 16 * EPS32 * (np.abs(X) @ np.abs(ref)) + tol.max()).all()
            assert np.abs(r["code"] - (t["z"][e] + np.float32(lr) * t["dx"][e][7:])).max() <= 2 * EPS32


def test_failures_are_the_references_per_object(gpu_decoder, dec64):
    from reconstruct import _libdsr as L

    ob = views_object(701, "Redwood")
    good = (ob.t_cam_obj, ob.views, None)
    opt = _opt(gpu_decoder, S.REDWOOD_OPTIM, "Redwood", 1)
    # view 1's rays all miss the unit ball: fewer than 10 in-ball samples (loss.py:86-88)
    miss = list(ob.views)
    miss[1] = (miss[1][0], miss[1][1], miss[1][2] + np.float32([5.0, 0.0, 0.0]), miss[1][3])
    # no surface points in any view: the sdf loss is a mean of nothing
    nopts = [(v[0], v[1][:0], v[2], v[3]) for v in ob.views]
    # one view without points beside two with
    one = list(ob.views)
    one[2] = nopts[2]
    (ra, rb, rc, rd), tr = opt.reconstruct_objects_views(
        [(ob.t_cam_obj, miss, None), (ob.t_cam_obj, nopts, None), (ob.t_cam_obj, one, None), good], trace=True)
    assert not ra["is_good"] and ra["fail_reason"] == L.FAIL_REASONS[2] and ra["fail_view"] == 1
    assert ra["loss"] == 0.0 and ra["t_cam_obj"] is None and ra["code"] is None
    assert not rb["is_good"] and rb["fail_reason"] == L.FAIL_REASONS[1] and rb["loss"] == 0.0
    assert rc["is_good"] and rc["fail_view"] == -1
    ov = oracle_views(ob)
    ov[2] = (ov[2][0], ov[2][1][:0], ov[2][2], ov[2][3], ov[2][4])
    assert_step_matches(tr[2], 0, dec64, S.REDWOOD_OPTIM, tr[2]["t_obj_cam"][0], tr[2]["z"][0], ov, "no points in view 2")
    # the good object beside the failing ones is the good object alone
    (alone,), (tr1,) = opt.reconstruct_objects_views([good], trace=True)
    assert rd["is_good"] and alone["is_good"]
    assert np.array_equal(rd["t_cam_obj"], alone["t_cam_obj"]) and np.array_equal(rd["code"], alone["code"])
    assert rd["loss"] == alone["loss"]
    for key in ("H", "b", "loss", "k"):
        assert np.array_equal(tr[3][key], tr1[key]), key


def test_audit_violation_in_a_view_redoes_the_object_exactly(gpu_decoder, monkeypatch):
    """As test_gpu_lite_audit.py::test_audit_guard_fires_and_redoes_exactly, across a tie: every
    lite value off by +-0.015 makes the audit fire, k_solve_views discards the iteration for all
    views of the object and the spare iteration decodes every sample exactly — the counts are
    those of the exact run and the normal equations agree like that test's lite-vs-exact steps
    (rel 1e-4: the redo keeps the exact pass's ReLU masks, the DSR_LITE=0 run re-forwards)."""
    objs = [(ob.t_cam_obj, ob.views, None) for ob in (views_object(700, "KITTI"), views_object(701, "KITTI", 2))]
    opt = _opt(gpu_decoder, S.KITTI_OPTIM, "KITTI", 1)
    monkeypatch.setenv("DSR_LITE", "0")
    r0, t0 = opt.reconstruct_objects_views(objs, trace=True)
    assert opt.last_stats.lite == 0
    monkeypatch.setenv("DSR_LITE", "1")
    monkeypatch.setenv("DSR_TEST_HOOKS", "1")
    monkeypatch.setenv("DSR_LITE_PERTURB", "0.015")
    r1, t1 = opt.reconstruct_objects_views(objs, trace=True)
    st = opt.last_stats
    assert st.test_hooks == 1 and st.lite == 1 and st.audit_points > 0
    assert st.lite_audit_violations > 0 and st.lite_redo_objects > 0
    for i in range(len(objs)):
        assert r0[i]["is_good"] and r1[i]["is_good"] and r1[i]["iters_done"] == 1
        rh, rb = rel(t1[i]["H"][0], t0[i]["H"][0]), rel(t1[i]["b"][0], t0[i]["b"][0])
        print(f"object {i}: k {int(t1[i]['k'][0])}/{int(t0[i]['k'][0])}, rel(H) {rh:.2e}, rel(b) {rb:.2e}")
        assert int(t1[i]["k"][0]) == int(t0[i]["k"][0])
        assert int(t1[i]["n_valid"][0]) == int(t0[i]["n_valid"][0])
        assert rh <= 1e-4 and rb <= 1e-4


def test_argument_errors(gpu_decoder):
    from reconstruct import _libdsr as L

    ob = views_object(700, "Redwood")
    opt = _opt(gpu_decoder, S.REDWOOD_OPTIM, "Redwood", 1)
    with pytest.raises(L.DsrError, match="n_views"):
        opt.reconstruct_objects_views([(ob.t_cam_obj, [], None)])
    scaled = list(ob.views)
    t = np.array(scaled[1][0])
    t[:3, :3] *= 1.1
    scaled[1] = (t,) + tuple(scaled[1][1:])
    with pytest.raises(L.DsrError, match="rigid"):
        opt.reconstruct_objects_views([(ob.t_cam_obj, scaled, None)])
    bad_row = list(ob.views)
    t = np.array(bad_row[2][0])
    t[3, 0] = 0.5
    bad_row[2] = (t,) + tuple(bad_row[2][1:])
    with pytest.raises(L.DsrError, match="rigid"):
        opt.reconstruct_objects_views([(ob.t_cam_obj, bad_row, None)])
    r = opt.reconstruct_object_views(ob.t_cam_obj, ob.views)     # the context is still usable
    assert r["is_good"] and r["fail_view"] == -1
