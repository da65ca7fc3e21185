"""Every decoder kernel held pointwise to the fp64 oracle, ReLU kinks attributed
(tests/decoder_check.py): ``sdf_eval`` forward-only and forward+Jacobian, on the
bench decoder, code-32 and the four F17 variant decoders, under every kernel selection that is
fp32-class by design (the one-product kernels, variant 8, are not and stay out).

Point set per (decoder, code): ``decoder_check.points`` — 13 special points (origin, the cube's
corners, four at |x| = 1.5), uniform ones in [-1, 1]^3, the special points again — of
64 (2 C) + 64 + 17 points, C the device's CU count: more than 2 C tiles, so that every workgroup
of ``dsr_sdf_eval``'s min(C, tiles) runs a second tile, one a third, and the last tile is ragged.
The sizes n = 1, 63, 64, 65, 129 are the leading n points of the same set and are judged by the
same rows of its truth, scales and E32 (E32 of one point alone would be no measure).  Codes: zero,
0.2 N(0,1), and 1.0 N(0,1) at the large size only.

Bitwise: the split-fp16 kernels scale a tile's activations by the tile's own maximum, padding
lanes included, so a row's bits depend on its tile's other rows and on nothing else.  Held
therefore: a run of n points equals the leading rows of a longer run on every tile they share in
full ((n // 64) * 64 rows; ragged-tile rows are held by the rule only), and every row of the
large run — second and third tiles of a workgroup — equals the same tile evaluated in a run of
at most C tiles, where it is some workgroup's first.

Measured rho = (GPU worst under the rule) / (fp32 numpy oracle's worst under the rule), MI355X,
point seeds 5, 6, 7, every size, code and kernel selection of a family; bound = 1.5 x the largest
rho, rounded up to a half-integer (``decoder_check.R``); m_kink = 4e-6 throughout:

    family  kernels                                     decoder  rho_f  rho_J   (r_f, r_J)
    split   k_mlp_fwd16 / k_mlp_jac16, default, v12,    bench    1.01   0.98
            rings 0, 2, 3, 4                            code32   1.12   1.04
                                                        plain    1.00   1.00    (2.0, 2.0)
    fp32    k_mlp_fwd<0, 2, 6> / k_mlp_jac (v0)         bench    1.49   1.97
                                                        code32   1.61   1.72
                                                        plain    1.41   1.47    (2.5, 3.0)
    tanh    the variant instantiations                  tanh     0.90   1.00    (1.5, 1.5)
    xyz                                                 xyz      0.93   1.02    (1.5, 2.0)
    ln                                                  ln       0.92   1.26    (1.5, 2.0)

E32_f 3.7e-7 .. 7.6e-7 and E32_J 5.6e-7 .. 9.2e-7 over these sets (LayerNorm: 3.0e-6 .. 4.1e-6 and
1.5e-6 .. 3.2e-6).  No rho above 8; no GPU error needed a flip beyond m_kink (the largest margin of a
unit a passing assignment flips is printed per run), so m_kink stays at its starting value.
"""
from __future__ import annotations

import os

import numpy as np
import pytest

import decoder_check as DC

pytestmark = pytest.mark.gpu

SMALL = (1, 63, 64, 65, 129)
CODES = {"zero": 0.0, "0.2": 0.2, "1.0": 1.0}
HOOKS = ("DSR_FWD_VARIANT", "DSR_JAC_VARIANT", "DSR_SPLIT_RING")

# (label, environment under DSR_TEST_HOOKS=1, family) — forward-only and Jacobian selections are
# paired by label: a pair computes the same forward
_RINGS = [(f"ring{r}", {"DSR_FWD_VARIANT": "12", "DSR_JAC_VARIANT": "12", "DSR_SPLIT_RING": str(r)}, "split")
          for r in (0, 2, 3, 4)]
FWD_SELECTIONS = [("default", {}, "split"),
                  ("v0", {"DSR_FWD_VARIANT": "0"}, "fp32"), ("v2", {"DSR_FWD_VARIANT": "2"}, "fp32"),
                  ("v6", {"DSR_FWD_VARIANT": "6"}, "fp32"), ("v12", {"DSR_FWD_VARIANT": "12"}, "split")] + _RINGS
JAC_SELECTIONS = [("default", {}, "split"), ("v0", {"DSR_JAC_VARIANT": "0"}, "fp32"),
                  ("v12", {"DSR_JAC_VARIANT": "12"}, "split")] + _RINGS


def selections(name):
    if DC.family(name) != "split":                       # a variant decoder: its one instantiation
        return [("default", {}, name)], [("default", {}, name)]
    return FWD_SELECTIONS, JAC_SELECTIONS


def n_cu():
    import torch

    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def large_n(c):
    return 64 * (2 * c) + 64 + 17


class Env:
    """Kernel selections through the process environment (read by the library at every call)."""

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in HOOKS + ("DSR_TEST_HOOKS",)}
        return self

    def select(self, env):
        for k in HOOKS:
            os.environ.pop(k, None)
        os.environ["DSR_TEST_HOOKS"] = "1"
        os.environ.update(env)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_TRUTH = {}


def truth(name, code_label, c, seed=5):
    """The fp64 truth, its alternatives and E32 of one (decoder, code, point set): computed once."""
    key = (name, code_label, c, seed)
    if key not in _TRUTH:
        d32, d64 = DC.oracle_pair(name)
        z = DC.code(CODES[code_label], 100 + seed, d32.code_len)
        T = DC.Truth(d32, d64, DC.make_inp(z, DC.points(large_n(c), seed)))
        T.z, T.x = z, np.ascontiguousarray(T.inp[:, -3:])
        _TRUTH[key] = T
    return _TRUTH[key]


def same_bytes(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _hold(cond, what, soft):
    if soft is None:
        assert cond, what
    elif not cond:
        soft.append(what)


def run_case(name, code_label, c, evaluate, bounds=None, seed=5, out=None, soft=None):
    """One (decoder, code): every kernel selection, every size, the rule and the bitwise
    properties.  ``evaluate(z, x, with_jac)`` is sdf_eval on the decoder; ``bounds`` maps a family
    to (r_f, r_J) (default: the shipped ``decoder_check.R``).  For a measuring run (how the table
    above was made: infinite bounds, three seeds) ``out`` collects every run's figures and ``soft``
    what the bitwise and 1e-6 assertions would have raised."""
    bounds = DC.R if bounds is None else bounds
    T = truth(name, code_label, c, seed)
    s = T.shares()
    print(f"\n{name} code {code_label} seed {seed}: n {T.n} ({-(-T.n // 64)} tiles on {c} CUs), m_kink {T.m_kink:.1e}, "
          f"kink share {s['kink']:.4f}, left out {s['left_out']:.5f}, k histogram {s['k_hist']}, "
          f"E32 f {T.e32_f:.2e} J {T.e32_J:.2e}, S_z {T.sz:.3f} S_x {T.sx:.3f}")
    T.assert_caps()
    assert -(-T.n // 64) > 2 * c
    sizes = (SMALL if code_label != "1.0" else ()) + (T.n,)
    fwd_sel, jac_sel = selections(name)
    chunk = 64 * c
    fwd_y = {}
    with Env() as env:
        for kind, sels in (("fwd", fwd_sel), ("jac", jac_sel)):
            for label, e, fam in sels:
                env.select(e)
                runs = {}
                for n in sizes:
                    r = evaluate(T.z, T.x[:n], kind == "jac")
                    y, J = r if kind == "jac" else (r, None)
                    runs[n] = (y, J)
                    tag = f"{name} code {code_label} {kind} {label} [{fam}] n {n}"
                    res = T.check(y, J, bounds[fam], tag, rows=slice(0, n), quiet=n != T.n)
                    if out is not None:
                        out.append(dict(name=name, code=code_label, seed=seed, kind=kind, label=label, family=fam, n=n,
                                        rho_f=res["rho_f"], rho_J=res["rho_J"], worst_f=res["worst_f"],
                                        worst_J=res["worst_J"], e32_f=T.e32_f, e32_J=T.e32_J,
                                        n_attributed=res["n_attributed"], margin_used=res["margin_used"]))
                # a shorter run is the leading rows of a longer one, on the tiles they share in full
                for a, b in zip(sizes[:-1], sizes[1:]):
                    full = (a // 64) * 64
                    for k in (0, 1):
                        if runs[a][k] is not None:
                            _hold(same_bytes(runs[a][k][:full], runs[b][k][:full]), ("prefix", kind, label, a, b, k), soft)
                # second and third tiles of a workgroup against the same tiles as first tiles
                yl, Jl = runs[T.n]
                for h in range(0, T.n, chunk):
                    r = evaluate(T.z, T.x[h:h + chunk], kind == "jac")
                    y, J = r if kind == "jac" else (r, None)
                    _hold(same_bytes(y, yl[h:h + chunk]), ("first tile", kind, label, h, "sdf"), soft)
                    _hold(J is None or same_bytes(J, Jl[h:h + chunk]), ("first tile", kind, label, h, "jac"), soft)
                if kind == "fwd":
                    fwd_y[label] = yl
                elif label in fwd_y:                     # the forward-only kernel of the same selection
                    d = float(np.abs(fwd_y[label] - yl).max())
                    print(f"{name} code {code_label} {label}: forward-only against forward+Jacobian sdf {d:.2e}")
                    _hold(d <= 1e-6, ("forward-only against forward+Jacobian", label, d), soft)


@pytest.fixture(scope="module")
def decs():
    from deep_sdf.workspace import decoder_from_state

    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = decoder_from_state(DC.decoder_state(name), DC.decoder_specs(name))
        return cache[name]

    return get


@pytest.mark.parametrize("code_label", list(CODES))
@pytest.mark.parametrize("name", DC.DECODERS)
def test_pointwise_against_fp64(decs, name, code_label):
    from reconstruct.optimizer import sdf_eval

    dec = decs(name)
    run_case(name, code_label, n_cu(), lambda z, x, jac: sdf_eval(dec, z, x, with_jac=jac))
