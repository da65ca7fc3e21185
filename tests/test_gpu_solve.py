"""k_solve / k_solve_views held to each iteration's traced system (tests/solve_check.py,
DESIGN.md §5.5): the fp64 Cholesky against the exact solution of the traced fp32 (H, b), the
fp32 LU fallback against three fp32 CPU solves of it, and the code / Sim(3) update, the result's
inverse and the loss bookkeeping against the traced state.

The solve is a fixed 71 x 71, so the shapes that matter are the kinds of system and the
instantiation (solve_check.single_cases / views_cases): positive definite with the upright
prior inactive (Redwood) and active (KITTI; a start pose tilted by 0.3 rad gives cond 3.5e6, the
stiffest the configuration produces), learning_rate 0.5, a 32-D code in the 64-D layout, the
tied-views instantiation, and three indefinite systems (negative k3 or scale_damping, which
dsr_reconstruct_batch passes on unvalidated) that only the LU fallback can solve.  Objects of
130 points and 40 background rays; every case runs once, in ``runs``, because the pose bounds'
E32 is the fp32 oracle's worst error over all of their steps.
"""
from __future__ import annotations

import numpy as np
import pytest

import solve_check as C
from conftest import make_cfg

pytestmark = pytest.mark.gpu

SINGLE = C.single_cases()
VIEWS = C.views_cases()


def run_cases(gpu_decoder):
    """name -> (optim, rule, result, trace) of every case, on the device."""
    from deep_sdf.workspace import decoder_from_state
    from reconstruct.optimizer import Optimizer

    import synthetic as S

    decs = {"bench": gpu_decoder, "code32": decoder_from_state(S.make_decoder(1234, C.SPECS32), C.SPECS32)}
    out = {}
    for name, (optim, kind, rule, ob, dec) in SINGLE.items():
        (r,), (t,) = Optimizer(decs[dec], make_cfg(optim, kind)).reconstruct_objects([ob], trace=True)
        out[name] = (optim, rule, r, t)
    for name, (optim, kind, rule, ob) in VIEWS.items():
        (r,), (t,) = Optimizer(gpu_decoder, make_cfg(optim, kind)).reconstruct_objects_views(
            [(ob.t_cam_obj, ob.views, None)], trace=True)
        assert r["fail_view"] == -1
        out[name] = (optim, rule, r, t)
    return out


def pose_bounds(runs):
    """(E32_T, E32_inv): the fp32 oracle's worst errors over every traced step of every case."""
    et, ei = [], []
    for name, (optim, _, r, t) in runs.items():
        lr = optim["joint_optim"]["learning_rate"]
        for e in range(int(r["iters_done"])):
            if np.isfinite(t["dx"][e]).all():
                a, b = C.oracle_pose_errors([(t["t_obj_cam"][e], t["dx"][e])], lr)
                et.append(a)
                ei.append(b)
    print(f"E32_T {max(et):.3e} (median {np.median(et):.2e}), E32_inv {max(ei):.3e} (median {np.median(ei):.2e}), "
          f"{len(et)} steps")
    return max(et), max(ei)


def judge(name, run, E32, r_c=None, r_lu=None, r_t=None):
    """Both rules on one case; returns (rule, rho of the solve, rho_T, E / |x|inf per iteration)."""
    optim, rule, r, t = run
    jo = optim["joint_optim"]
    n = jo["num_iterations"]
    assert r["is_good"], (name, r["fail_reason"], r["iters_done"])
    rho, es = -np.inf, []
    for e in range(n):
        what = f"{name} e={e}"
        if rule == "chol":
            a, E, _ = C.cholesky_rule(t["H"][e], t["b"][e], t["dx"][e], r_c, what)
        else:
            a, E = C.lu_rule(t["H"][e], t["b"][e], t["dx"][e], r_lu, what, strict=name not in C.LU_NOT_STRICT)
        rho = max(rho, a)
        es.append(E)
    rho_t = C.update_rule(t, r, jo["learning_rate"], n, jo["k1"], jo["k2"], E32, r_t, name)
    return rule, rho, rho_t, es


@pytest.fixture(scope="module")
def runs(gpu_decoder):
    return run_cases(gpu_decoder)


@pytest.fixture(scope="module")
def E32(runs):
    return pose_bounds(runs)


def test_bounds_are_measured():
    assert None not in (C.R_C, C.R_LU, C.R_T), "solve_check.R_* are not measured yet"


@pytest.mark.parametrize("name", [k for k, v in SINGLE.items() if v[2] == "chol"] + list(VIEWS))
def test_cholesky_and_update(runs, E32, name):
    judge(name, runs[name], E32, C.R_C, C.R_LU, C.R_T)


def test_prior_is_active_in_the_kitti_cases(runs):
    """The upright prior's residual is past its dead zone (1e-7) where the cases say it acts."""
    from oracle import dsr_oracle as O

    for name, its in (("kitti_300", (1, 2)), ("kitti_302", (1, 2)), ("kitti_tilted", (0,)), ("kitti_flat", (0, 1)),
                      ("views_kitti", (1,))):
        t = runs[name][3]
        for e in its:
            _, res = O.compute_rotation_loss_sim3(t["t_obj_cam"][e].astype(np.float64))
            assert res > 1e-7, (name, e, res)
    t = runs["kitti_tilted"][3]
    lo, hi = C.eig_range(t["H"][0])
    print(f"kitti_tilted: cond {hi / lo:.3e}")
    assert hi / lo > 1e6


def test_code32_padded_block_is_inert(runs):
    """A 32-D code in the 64-D layout: the padded dimensions 39..70 carry k3 on the diagonal and
    nothing else, and their step is exactly 0 — through the Cholesky's panels 4..8 too."""
    optim, _, r, t = runs["code32"]
    k3 = np.float32(optim["joint_optim"]["k3"])
    assert r["code"].shape == (32,)
    for e in range(2):
        H, b, dx = t["H"][e], t["b"][e], t["dx"][e]
        assert (H[39:, :39] == 0).all() and (H[:39, 39:] == 0).all()
        assert np.array_equal(H[39:, 39:], np.diag(np.full(32, k3)))
        assert (b[39:] == 0).all()
        assert (dx[39:] == 0).all(), dx[39:]
        assert np.abs(dx[:39]).max() > 0
    assert (t["z"][0] == 0).all()


@pytest.mark.parametrize("name", [k for k, v in SINGLE.items() if v[2] == "lu"])
def test_lu_fallback_and_update(runs, E32, name):
    """An H with a negative eigenvalue: the Cholesky meets a non-positive pivot and the fp32 LU
    with partial pivoting, explicit inverse and mat-vec solves a finite system."""
    optim, _, r, t = runs[name]
    assert r["is_good"] and np.isfinite(t["dx"][0]).all(), (r["fail_reason"], t["dx"][0])
    assert np.abs(t["b"][0][7:]).min() > 0            # the start code reaches b
    judge(name, runs[name], E32, C.R_C, C.R_LU, C.R_T)
