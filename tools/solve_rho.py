"""rho = (GPU worst) / E under tests/solve_check.py's rules, per case of tests/test_gpu_solve.py:
the measurement behind ``solve_check.R_C / R_LU / R_T`` and DESIGN.md §5.5's table.  Nothing is
asserted on the three bounds; the preconditions and the exact parts of the rules are.

    python tools/solve_rho.py
"""
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "tests"), os.path.join(REPO, "dsp-slam-rgbd_amd"), REPO]
import numpy as np  # noqa: E402

import solve_check as C  # noqa: E402
import synthetic as S  # noqa: E402
import test_gpu_solve as G  # noqa: E402
from deep_sdf.workspace import decoder_from_state  # noqa: E402

runs = G.run_cases(decoder_from_state(S.make_decoder(1234), S.DEFAULT_SPECS))
for name, (_, rule, r, t) in runs.items():
    print(f"{name}: {rule}, is_good {r['is_good']}, iterations {r['iters_done']}, K {t['k']}, max|dx| {np.abs(t['dx']).max():.4g}")
E32 = G.pose_bounds(runs)
table = {name: G.judge(name, run, E32) for name, run in runs.items()}
print("\ncase: rule, rho of the solve, rho_T, E / |x|inf per iteration")
for name, (rule, rho, rho_t, es) in table.items():
    print(f"{name:18s} {rule:4s} rho {rho:10.3f}  rho_T {rho_t:.3f}  E {' '.join(f'{e:.2e}' for e in es)}")
half = lambda rho: math.ceil(3 * rho) / 2   # noqa: E731
rc = max(v[1] for v in table.values() if v[0] == "chol")
rl = max(v[1] for v in table.values() if v[0] == "lu")
rt = max(v[2] for v in table.values())
print(f"rho_c {rc:.3f}, rho_lu {rl:.3f}, rho_T {rt:.3f}; E32_T {E32[0]:.2e}, E32_inv {E32[1]:.2e}")
print(f"1.5 x rho rounded up to a half-integer: R_C {max(half(rc), 0.5)} (never below 0.5), R_LU {half(rl)}, R_T {half(rt)}; "
      f"shipped {C.R_C}, {C.R_LU}, {C.R_T}")
