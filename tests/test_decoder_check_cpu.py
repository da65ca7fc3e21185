"""The pointwise decoder check (tests/decoder_check.py) tried on the CPU: the fp32 numpy oracle
passes it against fp64 on every decoder with no point left out beyond the cap, and candidates
that are wrong the way a kernel goes wrong — built from the fp64 oracle, so each differs from the
truth by its mutation alone — fail it at the shipped bounds ``decoder_check.R`` and M_KINK.
"""
from __future__ import annotations

import numpy as np
import pytest

import decoder_check as DC

N = 64 * 64 + 17          # 65 tiles, the last one ragged


@pytest.fixture(scope="module")
def truths():
    cache = {}

    def get(name):
        if name not in cache:
            d32, d64 = DC.oracle_pair(name)
            z = DC.code(0.2, 5, d32.code_len)
            cache[name] = (DC.Truth(d32, d64, DC.make_inp(z, DC.points(N, 5)), keep_pres=True), d64)
        return cache[name]

    return get


def _r(name):
    """The loosest shipped bounds any kernel of this decoder is held to."""
    fams = [DC.family(name)] + (["fp32"] if DC.family(name) == "split" else [])
    return (max(DC.R[f][0] for f in fams), max(DC.R[f][1] for f in fams))


def _backward(dec, inp, skip_xyz_layer=None, ln_no_mean=False):
    """The oracle's forward_jac restated with two switchable faults: layer ``skip_xyz_layer``'s
    contribution to d/dxyz left out (xyz_in_all), the LayerNorm backward without its mean term."""
    dt = dec.dtype
    inp = np.asarray(inp, dt)
    lnk = {}
    y, masks, t = dec.forward(inp, keep_masks=True, keep_pre=True, keep_ln=lnk)
    nl, L3 = len(dec.layers), inp.shape[-1]
    g = (1 - y * y)[:, None]
    if dec.use_tanh:
        g = g * (1 - t * t)[:, None]
    grad_in = np.zeros_like(inp)
    for i in range(nl - 1, -1, -1):
        W, _ = dec.layers[i]
        if i < nl - 1 and i in lnk:
            xh, rstd = lnk[i]
            gx = g * dec.norms[i][0]
            mean = 0.0 if ln_no_mean else gx.mean(-1, keepdims=True)
            g = rstd * (gx - mean - xh * (gx * xh).mean(-1, keepdims=True))
        g = g @ W
        if i in dec.latent_in:
            grad_in = grad_in + g[:, -L3:]
            g = g[:, :-L3]
        elif i != 0 and dec.xyz_in_all:
            if i != skip_xyz_layer:
                grad_in[:, -3:] = grad_in[:, -3:] + g[:, -3:]
            g = g[:, :-3]
        if i > 0:
            g = np.where(masks[i - 1], g, dt(0))
    return y, g + grad_in


def _fp16_layer(dec, layer, rows=slice(None)):
    """``dec`` with rows ``rows`` of one layer's weights rounded to fp16: one GEMM's (one output
    unit's) lo products dropped."""
    layers = [(W.copy(), b) for W, b in dec.layers]
    W = layers[layer][0]
    W[rows] = W[rows].astype(np.float16).astype(np.float64)
    return type(dec)(layers, dec.code_len, dec.latent_in, np.float64, dec.xyz_in_all, dec.use_tanh, dec.norms)


@pytest.mark.parametrize("name", DC.DECODERS)
def test_fp32_oracle_passes_and_caps_hold(truths, name):
    T, _ = truths(name)
    s = T.shares()
    print(f"\n{name}: n {T.n}, m_kink {T.m_kink:.1e}: kink share {s['kink']:.4f}, left out {s['left_out']:.5f} "
          f"(cap {DC.LEFT_OUT_CAP}), k histogram {s['k_hist']}, S_z {T.sz:.3f} S_x {T.sx:.3f}")
    T.assert_caps()
    plain_J = T._e_jac(T.J32, T.J)
    print(f"{name}: fp32 oracle plain comparison worst e_J {plain_J.max():.2e}, on its k = 0 points "
          f"{plain_J[T.k == 0].max():.2e}; under the rule E32_J {T.e32_J:.2e}, E32_f {T.e32_f:.2e}")
    res = T.check(T.y32, T.J32, (1.0, 1.0), f"{name} fp32 oracle")
    assert res["n_judged"] == T.n - int(T.left_out.sum())
    # fp32-class on every point, kinks included: nothing like the plain comparison's 1e-2 tail
    # (nine 512-term fp32 sums deep: 64 eps = 7.6e-6 leaves 3x over the LayerNorm decoder's 2.5e-6)
    assert T.e32_J <= 64 * np.finfo(np.float32).eps and T.e32_f <= 64 * np.finfo(np.float32).eps
    # the fp64 truth itself passes at any bound
    assert not T.fails(T.y, T.J, (1e-3, 1e-3))
    # a prefix or a tile-aligned slice of the set is judged by the same rows of the truth
    assert not T.fails(T.y32[:65], T.J32[:65], (1.0, 1.0), rows=slice(0, 65))
    assert not T.fails(T.y32[128:], None, (1.0, 1.0), rows=slice(128, None))


@pytest.mark.parametrize("name", DC.DECODERS)
def test_mutants_fail(truths, name):
    T, d64 = truths(name)
    r = _r(name)
    inp64 = T.inp.astype(np.float64)
    yb, Jb = _backward(d64, inp64)
    assert np.array_equal(yb, T.y) and np.array_equal(Jb, T.J)     # the restatement is the oracle's
    caught = {}
    # one hidden layer's weights in fp16 (one GEMM's lo products dropped)
    ym, Jm = _fp16_layer(d64, 3).forward_jac(inp64)
    print(f"\n{name}: layer 3 in fp16: sdf error up to {np.abs(ym - T.y).max():.2e}")
    caught["layer_fp16_fwd"] = T.fails(ym, None, r)
    caught["layer_fp16_jac"] = T.fails(ym, Jm, r)
    # two neighbouring points' rows swapped
    y, J = T.y.copy(), T.J.copy()
    y[[200, 201]], J[[200, 201]] = y[[201, 200]], J[[201, 200]]
    caught["rows_swapped"] = T.fails(y, J, r)
    caught["rows_swapped_fwd"] = T.fails(y, None, r)
    # the last point of the ragged tile with a zero Jacobian
    J = T.J.copy()
    J[-1] = 0
    caught["ragged_last_zero_jac"] = T.fails(T.y, J, r)
    # one unit with an fp64 margin near 1e-3 flipped at one point: no kink, an error
    best = None
    for l, p in enumerate(T.pres[1:], 1):
        d = np.abs(np.abs(p) - 1e-3)
        pt, u = np.unravel_index(np.argmin(d), d.shape)
        if best is None or d[pt, u] < best[0]:
            best = (d[pt, u], int(pt), l, int(u), abs(p[pt, u]), bool(p[pt, u] > 0))
    _, pt, l, u, marg, on = best
    yf, Jf = d64.forward_jac(inp64[pt:pt + 1], force=[(0, l, u, int(not on))])
    y, J = T.y.copy(), T.J.copy()
    y[pt], J[pt] = yf[0], Jf[0]
    print(f"{name}: unit ({l}, {u}) flipped at point {pt}, fp64 margin {marg:.2e}: e_J "
          f"{T._e_jac(J[pt], T.J[pt]):.2e} (E32_J {T.e32_J:.2e})")
    caught["flip_at_margin_1e-3"] = T.fails(y, J, r)
    if d64.xyz_in_all:
        _, J = _backward(d64, inp64, skip_xyz_layer=6)
        caught["xyz_layer_omitted"] = T.fails(T.y, J, r)
    if any(n is not None for n in d64.norms):
        _, J = _backward(d64, inp64, ln_no_mean=True)
        caught["ln_backward_without_mean"] = T.fails(T.y, J, r)
    print(f"{name}: bounds {r}: " + ", ".join(f"{k} {'caught' if v else 'MISSED'}" for k, v in caught.items()))
    assert all(caught.values()), caught


def test_how_fine_the_net_is(truths):
    """Not an assertion of the rule, a reading of it: one weight row of one layer in fp16 (one
    hidden unit whose lo products are lost) moves the sdf by a few 1e-6 at most — whether the
    shipped r_f still catches that is printed for every family's bound."""
    T, d64 = truths("bench")
    ym, Jm = _fp16_layer(d64, 3, slice(0, 1)).forward_jac(T.inp.astype(np.float64))
    res = T.judge(ym, None, 1.0, 1.0)
    resj = T.judge(ym, Jm, 1.0, 1.0)
    print(f"\none row of layer 3 in fp16: sdf error up to {np.abs(ym - T.y).max():.2e}, {res['rho_f']:.1f} E32_f under "
          f"the rule; with its Jacobian {resj['rho_J']:.0f} E32_J (the unit's own decision moves at margins up to 1e-4)")
    for fam, r in DC.R.items():
        print(f"  {fam} bounds {r}: sdf alone {'caught' if T.fails(ym, None, r) else 'not caught'}, "
              f"sdf and Jacobian {'caught' if T.fails(ym, Jm, r) else 'not caught'}")
    assert res["rho_f"] > 1.0                                # beyond the fp32 oracle's own error
