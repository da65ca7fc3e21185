"""rho = (GPU worst) / (fp32 numpy oracle's worst) under tests/decoder_check.py's rule, per kernel
family and decoder, over the cases of tests/test_gpu_decoder_pointwise.py and several point seeds:
the measurement behind ``decoder_check.R`` and DESIGN.md §5.4's table.  Nothing is asserted on the
rule (infinite bounds); what the bitwise and 1e-6 assertions would have raised is listed.

    python tools/decoder_rho.py [seeds, default 5,6,7] [decoders, default all] [records.json]
"""
import json
import math
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "tests"), os.path.join(REPO, "dsp-slam-rgbd_amd"), REPO]
import numpy as np  # noqa: E402

import decoder_check as DC  # noqa: E402
import test_gpu_decoder_pointwise as P  # noqa: E402
from deep_sdf.workspace import decoder_from_state  # noqa: E402
from reconstruct.optimizer import sdf_eval  # noqa: E402

seeds = [int(s) for s in sys.argv[1].split(",")] if len(sys.argv) > 1 else [5, 6, 7]
names = sys.argv[2].split(",") if len(sys.argv) > 2 else list(DC.DECODERS)
c = P.n_cu()
inf = {k: (np.inf, np.inf) for k in DC.R}
out, not_held = [], []
for name in names:
    dec = decoder_from_state(DC.decoder_state(name), DC.decoder_specs(name))
    for seed in seeds:
        for cl in P.CODES:
            soft = []
            P.run_case(name, cl, c, lambda z, x, jac: sdf_eval(dec, z, x, with_jac=jac), bounds=inf, seed=seed,
                       out=out, soft=soft)
            not_held += [(name, seed, cl, repr(w)) for w in soft]
            P._TRUTH.clear()
if len(sys.argv) > 3:
    with open(sys.argv[3], "w") as f:
        json.dump(dict(records=out, not_held=not_held), f)

print("\nfamily decoder: largest rho_f, rho_J (worst / E32 at it)")
for fam in DC.R:
    rs = [r for r in out if r["family"] == fam]
    if not rs:
        continue
    for name in sorted({r["name"] for r in rs}):
        f = max((r for r in rs if r["name"] == name), key=lambda r: r["rho_f"])
        j = max((r for r in rs if r["name"] == name), key=lambda r: r["rho_J"])
        print(f"{fam:5s} {name:6s}: rho_f {f['rho_f']:.3f} ({f['worst_f']:.2e} / {f['e32_f']:.2e}; {f['kind']} {f['label']} "
              f"code {f['code']} seed {f['seed']} n {f['n']})  rho_J {j['rho_J']:.3f} ({j['worst_J']:.2e} / {j['e32_J']:.2e}; "
              f"{j['label']} code {j['code']} seed {j['seed']} n {j['n']})")
    mf, mj = max(r["rho_f"] for r in rs), max(r["rho_J"] for r in rs)
    print(f"  {fam}: bounds 1.5 x rho rounded up to a half-integer: ({math.ceil(3 * mf) / 2}, {math.ceil(3 * mj) / 2}); "
          f"shipped {DC.R[fam]}")
print("assertions not held:", not_held)
