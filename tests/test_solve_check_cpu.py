"""The rules of tests/solve_check.py have teeth: on the fp32 numpy oracle's own
systems at the shapes of tests/test_gpu_solve.py, the kernel's Cholesky schedule restated in
fp64 (``chol_blocked``) passes the Cholesky rule at the shipped R_C and every mutation of it, and
any fp32 solve, fails; the restatement refuses every indefinite system; the LU rule accepts the
three fp32 CPU solves and rejects an elimination without pivoting; the update rule accepts the
oracle's own update and rejects three wrong ones."""
from __future__ import annotations

import numpy as np
import pytest

import solve_check as C

CASES = {**C.single_cases(), **C.views_cases()}
SPD = [k for k, v in CASES.items() if v[2] == "chol"]
LU = [k for k, v in CASES.items() if v[2] == "lu"]


@pytest.fixture(scope="module")
def runs():
    """name -> (result, trace) of every case by the fp32 oracle, computed once."""
    decs = {"bench": C.oracle_decoder("bench"), "code32": C.oracle_decoder("code32")}
    return {k: C.oracle_run(v, decs[v[4]] if len(v) == 5 else decs["bench"]) for k, v in CASES.items()}


@pytest.fixture(scope="module")
def E32(runs):
    steps = [(k, e) for k, (r, t) in runs.items() for e in range(r["iters_done"])]
    errs = [C.oracle_pose_errors([(runs[k][1]["t_obj_cam"][e], runs[k][1]["dx"][e])],
                                 CASES[k][0]["joint_optim"]["learning_rate"]) for k, e in steps]
    return max(a for a, _ in errs), max(b for _, b in errs)


def systems(runs, names):
    return [(f"{k} e={e}", runs[k][1]["H"][e], runs[k][1]["b"][e]) for k in names for e in range(runs[k][0]["iters_done"])]


def test_exact_solve_converges_and_solves_exactly(runs):
    """On every system, the cond 3.5e6 one included: the convergence assertion inside
    exact_solve holds and the rational residual of hi + lo is below 2^-90 |b|inf."""
    from fractions import Fraction

    conds = []
    for what, H, b in systems(runs, list(CASES)):
        hi, lo = C.exact_solve(H, b)
        x = [Fraction(float(h)) + Fraction(float(l)) for h, l in zip(hi, lo)]
        res = max(abs(Fraction(float(b[i])) - sum(Fraction(float(H[i, j])) * x[j] for j in range(C.NPAR)))
                  for i in range(C.NPAR))
        assert float(res) <= 2.0 ** -90 * float(np.abs(b).max()), (what, float(res))
        lo_, hi_ = C.eig_range(H)
        conds.append(abs(hi_ / lo_))
    assert max(conds) > 1e6, max(conds)             # the tilted KITTI start pose


def test_restatement_passes_the_cholesky_rule(runs):
    for what, H, b in systems(runs, SPD):
        dx = C.chol_blocked(H, b)
        assert dx is not None, what
        C.cholesky_rule(H, b, dx, C.R_C, what)


def test_restatement_refuses_indefinite_systems(runs):
    for what, H, b in systems(runs, LU):
        lo, hi = C.eig_range(H)
        assert lo < -C.INDEFINITE * hi, what
        assert C.chol_blocked(H, b) is None, what


@pytest.mark.parametrize("mutation", C.MUTATIONS + ("inv32", "oracle_dx"))
def test_cholesky_rule_rejects(runs, mutation):
    """Every mutation fails the rule at the shipped R_C on every positive definite system it
    touches (a 32-D code's padded block has no off-diagonal entries and no right-hand side, so
    the two mutations that act on rows 64..71 alone leave its dx as it is)."""
    for k in SPD:
        if k == "code32" and mutation in ("b_skips_last_panel", "row64_lane63"):
            continue
        for e in range(runs[k][0]["iters_done"]):
            H, b = runs[k][1]["H"][e], runs[k][1]["b"][e]
            if mutation == "inv32":
                dx = np.linalg.inv(H) @ b
            elif mutation == "oracle_dx":
                dx = runs[k][1]["dx"][e]
            else:
                dx = C.chol_blocked(H, b, mutation)
                if dx is None:        # the mutation drove a pivot negative: the kernel's next stop
                    dx = C.lu_references(H, b)["torch.inverse@b"]          # is the fp32 fallback
            rho, _, _ = C.cholesky_rule(H, b, dx, None, f"{k} e={e} {mutation}")
            assert rho > 1e3 * C.R_C, (k, e, mutation, rho)


def lu_no_pivot32(H, b):
    """Gaussian elimination in fp32 without row interchanges, then the two substitutions."""
    A = np.array(H, np.float32)
    y = np.array(b, np.float32)
    n = y.shape[0]
    for k in range(n - 1):
        m = A[k + 1:, k] / A[k, k]
        A[k + 1:, k + 1:] -= np.outer(m, A[k, k + 1:])
        y[k + 1:] -= m * y[k]
    x = np.zeros(n, np.float32)
    for i in range(n - 1, -1, -1):
        x[i] = (y[i] - A[i, i + 1:] @ x[i + 1:]) / A[i, i]
    return x


def test_lu_rule_accepts_the_references_and_rejects_no_pivoting(runs):
    for k in LU:
        H, b = runs[k][1]["H"][0], runs[k][1]["b"][0]
        for name, dx in C.lu_references(H, b).items():
            C.lu_rule(H, b, dx, C.R_LU, f"{k} {name}", strict=k not in C.LU_NOT_STRICT)
        C.lu_rule(H, b, runs[k][1]["dx"][0], C.R_LU, f"{k} oracle", strict=k not in C.LU_NOT_STRICT)
    H, b = runs["lu_scale_damping"][1]["H"][0], runs["lu_scale_damping"][1]["b"][0]
    rho, _ = C.lu_rule(H, b, lu_no_pivot32(H, b), None, "lu_scale_damping no pivoting")
    assert rho > C.R_LU, rho


def case_args(k):
    jo = CASES[k][0]["joint_optim"]
    return jo["learning_rate"], jo["num_iterations"], jo["k1"], jo["k2"]


def test_update_rule_accepts_the_oracle(runs, E32):
    for k, (r, t) in runs.items():
        rho = C.update_rule(t, r, *case_args(k), E32, C.R_T, k)
        assert rho <= 1.0            # E32 is the oracle's own worst


def exp_sim3_no_s(x):
    """exp_sim3 with the translation Jacobian taken at s = 0 (exp_se3's), the rotation block as is."""
    from oracle import dsr_oracle as O

    out = O.exp_sim3(x)
    out[:3, 3] = O.exp_se3(x[:6])[:3, 3]
    return out


@pytest.mark.parametrize("mutation", ["no_s_term", "T_dT", "lr_not_on_code"])
def test_update_rule_rejects(runs, E32, mutation):
    """The first update of a trace replaced by a wrong one (fp64, so nothing but the mutation
    differs): every case with a second traced state must fail; lr must differ from 1 for the
    third."""
    from oracle import dsr_oracle as O

    names = ["redwood_lr05"] if mutation == "lr_not_on_code" else [k for k, (r, _) in runs.items() if r["iters_done"] > 1]
    assert names
    for k in names:
        r, t = runs[k]
        lr = case_args(k)[0]
        t = {key: np.array(v) for key, v in t.items()}
        T, x = t["t_obj_cam"][0].astype(np.float64), lr * t["dx"][0][:7].astype(np.float64)
        if mutation == "no_s_term":
            t["t_obj_cam"][1] = (exp_sim3_no_s(x) @ T).astype(np.float32)
        elif mutation == "T_dT":
            t["t_obj_cam"][1] = (T @ O.exp_sim3(x)).astype(np.float32)
        else:
            L = t["z"].shape[1]
            t["z"][1] = t["z"][0] + t["dx"][0][7:7 + L]
        with pytest.raises(AssertionError, match="ulp from z" if mutation == "lr_not_on_code" else "E32_T from exp_sim3"):
            C.update_rule(t, r, *case_args(k), E32, C.R_T, f"{k} {mutation}")
