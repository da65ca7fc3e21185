"""Pointwise decoder check against the fp64 oracle, ReLU kinks attributed.

A candidate (y, J) — a GPU kernel's sdf and d sdf / d[code, xyz] at points ``inp`` — is judged
against the fp64 oracle of the same decoder (oracle/dsr_oracle.py), point by point, with no
tolerance fixed in advance and no excused share of points:

* near(p): the hidden units whose fp64 ReLU input at p has magnitude <= M_KINK.  Any two
  finite-precision implementations may decide such a unit either way, so p's admissible
  assignments are the 2^k on/off settings of its k near units (forward and backward under the
  forced mask, ``Decoder.forward_jac(force=...)``).  k = 0 for almost every point: the plain
  comparison.  Points with k > K_MAX are left out; their share is capped (LEFT_OUT_CAP) and
  asserted for the oracle alone (``Truth.assert_caps``) before any candidate is judged.
* e_f = |y - y_c|;  e_J = max(max|J_z - J_c,z| / S_z, max|J_x - J_c,x| / S_x), S_z / S_x the
  largest |fp64 entry| of the code / xyz columns over the point set (no floor of 1: the code
  columns are 10-13 times smaller than the xyz ones and get their own scale).
* a point passes if ONE admissible assignment c gives e_f <= r_f E32_f and e_J <= r_J E32_J,
  where E32_f / E32_J are the fp32 numpy oracle's own worst errors under this same rule on this
  same point set (``Truth`` computes them from the two oracles alone).  r_f, r_J per kernel
  family: ``R`` below, from the measured rho = (GPU worst) / E32 (table: DESIGN.md §5.4 and
  tests/test_gpu_decoder_pointwise.py).

"Worst under the rule" needs one assignment per point although the pass condition is joint:
it is the assignment minimising max(e_f / u_f, e_J / u_J), (u_f, u_J) = E32 for a candidate
and the fp32 oracle's worst over its k = 0 points while E32 itself is being computed.

A failure lists every offending point with its tile and lane (index // 64, index % 64), its
smallest fp64 margin, k, and both errors in units of E32, so that a tile-edge or lane bug reads
as one.
"""
from __future__ import annotations

import numpy as np

import synthetic as S

M_KINK = 4e-6          # see DESIGN.md §5.4: ~6x the largest margin at which numpy fp32 decides
#                        a unit differently from fp64 (6.9e-7 over the decoders below)
M_KINK_MAX = 1.6e-5    # a flip of a unit with a larger margin is an error, never a kink
K_MAX = 3
LEFT_OUT_CAP = 1e-3
TILE = 64

# (r_f, r_J) per kernel family: 1.5 x the largest measured rho, rounded up to a half-integer
# (measured table: DESIGN.md §5.4, tests/test_gpu_decoder_pointwise.py)
R = {
    "split": (2.0, 2.0),     # k_mlp_fwd16 / k_mlp_jac16, every ring depth: rho 1.12 / 1.04
    "fp32": (2.5, 3.0),      # k_mlp_fwd<0,2,6> / k_mlp_jac: rho 1.61 / 1.97
    "tanh": (1.5, 1.5),      # the variant instantiations, use_tanh: rho 0.90 / 1.00
    "xyz": (1.5, 2.0),       # xyz_in_all: rho 0.93 / 1.02
    "ln": (1.5, 2.0),        # LayerNorm: rho 0.92 / 1.26
}

SPECS32 = dict(S.DEFAULT_SPECS, CodeLength=32)
DECODERS = ("bench", "code32", "tanh", "xyz", "plain", "ln")


def decoder_specs(name):
    from test_oracle_golden import _variant_specs

    if name == "bench":
        return S.DEFAULT_SPECS
    if name == "code32":
        return SPECS32
    return _variant_specs(name)


def decoder_state(name):
    return S.make_decoder(1234, decoder_specs(name))


def oracle_pair(name):
    """(fp32 oracle, fp64 oracle) of one of DECODERS."""
    from oracle.dsr_oracle import Decoder

    state, specs = decoder_state(name), decoder_specs(name)
    return Decoder.from_state(state, specs), Decoder.from_state(state, specs, dtype=np.float64)


def family(name):
    """The kernel family a decoder runs on by default (plain Linear layers and a 32-D code are
    the shipped topology: the split-fp16 kernels)."""
    return name if name in ("tanh", "xyz", "ln") else "split"


def points(n, seed):
    """n >= 26 points: the origin, the cube's eight corners and four points at |x| = 1.5, then
    uniform ones in [-1, 1]^3, then the same 13 special points again — so that both the first
    tile (and every prefix of the set from 13 points on) and the ragged last tile hold them."""
    rng = np.random.default_rng(seed)
    corners = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float32)
    far = np.array([[1.5, 0, 0], [0, -1.5, 0], [0, 0, 1.5], [0.9, -0.8, 0.9]], np.float32)
    far[3] *= np.float32(1.5 / np.linalg.norm(far[3]))
    special = np.concatenate([np.zeros((1, 3), np.float32), corners, far])
    u = rng.uniform(-1, 1, (n - 2 * special.shape[0], 3)).astype(np.float32)
    return np.concatenate([special, u, special])


def code(scale, seed, code_len=64):
    return (scale * np.random.default_rng(seed).standard_normal(code_len)).astype(np.float32)


def make_inp(z, x):
    return np.concatenate([np.broadcast_to(z, (x.shape[0], z.shape[0])), x], 1).astype(np.float32)


class Truth:
    """The fp64 oracle's (y, J), near sets and admissible alternatives at ``inp``, and the fp32
    oracle's worst errors E32 under the rule — everything a check needs, computed once per
    (decoder, point set) from the two oracles alone."""

    def __init__(self, dec32, dec64, inp, m_kink=M_KINK, keep_pres=False):
        assert 0 < m_kink <= M_KINK_MAX
        inp = np.asarray(inp, np.float32)
        self.inp, self.m_kink, self.dec64 = inp, m_kink, dec64
        self.n, self.L = inp.shape[0], inp.shape[1] - 3
        inp64 = inp.astype(np.float64)
        pres = []
        self.y, self.J = dec64.forward_jac(inp64, keep_relu_in=pres)
        self.sz = float(np.abs(self.J[:, :self.L]).max())
        self.sx = float(np.abs(self.J[:, self.L:]).max())
        self.margin = np.min([np.abs(p).min(1) for p in pres], axis=0)
        rows = []
        for l, p in enumerate(pres):
            pt, u = np.nonzero(np.abs(p) <= m_kink)
            rows.append(np.stack([pt, np.full_like(pt, l), u, (p[pt, u] > 0).astype(np.int64)], 1))
        rows = np.concatenate(rows)
        rows = rows[np.argsort(rows[:, 0], kind="stable")]
        self.k = np.bincount(rows[:, 0], minlength=self.n)
        self.left_out = self.k > K_MAX
        self.kink_idx = np.nonzero((self.k > 0) & ~self.left_out)[0]
        nk = self.kink_idx.size
        pos = np.full(self.n, -1, np.int64)
        pos[self.kink_idx] = np.arange(nk)
        rows = rows[pos[rows[:, 0]] >= 0]
        start = np.concatenate([[0], np.cumsum(self.k[self.kink_idx])])[:-1]
        rank = np.arange(rows.shape[0]) - np.repeat(start, self.k[self.kink_idx])
        # alternatives 1..7 of the kink points: near unit j of a point flipped iff bit j of c
        n_alt = 1 << K_MAX
        self.alt_y = np.full((n_alt, nk), np.nan)
        self.alt_J = np.full((n_alt, nk, self.L + 3), np.nan)
        self.alt_margin = np.zeros((n_alt, nk))            # largest margin among c's flipped units
        rmargin = np.array([abs(pres[l][p, u]) for p, l, u, _ in rows]) if rows.size else np.zeros(0)
        self.pres = pres if keep_pres else None             # per hidden layer, what its ReLU sees
        del pres
        kk = self.k[self.kink_idx]
        for c in range(1, n_alt):
            sel = np.nonzero((1 << kk) > c)[0]
            if sel.size == 0:
                continue
            sub = np.full(nk, -1, np.int64)
            sub[sel] = np.arange(sel.size)
            rsel = sub[pos[rows[:, 0]]] >= 0
            r = rows[rsel].copy()
            flip = (c >> rank[rsel]) & 1
            r[:, 3] ^= flip
            np.maximum.at(self.alt_margin[c], pos[r[:, 0]], np.where(flip == 1, rmargin[rsel], 0.0))
            r[:, 0] = sub[pos[r[:, 0]]]
            ya, Ja = dec64.forward_jac(inp64[self.kink_idx[sel]], force=r)
            self.alt_y[c, sel], self.alt_J[c, sel] = ya, Ja
        # the fp32 oracle under the rule
        y32, J32 = dec32.forward_jac(inp)
        self.y32, self.J32 = y32, J32
        EF, EJ = self._tables(y32, J32)
        clean = self.k == 0
        tiny = np.finfo(np.float64).tiny
        uf, uJ = max(float(EF[0, clean].max()), tiny), max(float(EJ[0, clean].max()), tiny)
        ef, eJ, _ = self._best(EF, EJ, uf, uJ)
        judged = ~self.left_out
        self.e32_f, self.e32_J = max(float(ef[judged].max()), tiny), max(float(eJ[judged].max()), tiny)

    # -- statistics of the point set (the oracle alone) ---------------------------------------
    def shares(self):
        return {"left_out": float(self.left_out.mean()), "kink": float((self.k > 0).mean()),
                "k_hist": np.bincount(self.k, minlength=K_MAX + 2).tolist()}

    def assert_caps(self):
        s = self.shares()
        assert s["left_out"] <= LEFT_OUT_CAP, s

    # -- errors of a candidate ------------------------------------------------------------------
    def _e_jac(self, J, Jc):
        d = np.abs(np.asarray(J, np.float64) - Jc)
        return np.maximum(d[..., :self.L].max(-1) / self.sz, d[..., self.L:].max(-1) / self.sx)

    def _tables(self, y, J, rows=None):
        """(EF, EJ): (8, n) errors against assignment c of every point; inf where c is not one
        of the point's assignments.  ``rows``: the candidate holds these rows of the set only."""
        idx = np.arange(self.n) if rows is None else np.arange(self.n)[rows]
        y = np.asarray(y, np.float64)
        assert y.shape == (idx.size,), (y.shape, idx.size)
        n_alt = 1 << K_MAX
        EF = np.full((n_alt, idx.size), np.inf)
        EJ = np.full((n_alt, idx.size), np.inf)
        EF[0] = np.abs(y - self.y[idx])
        if J is not None:
            assert np.shape(J) == (idx.size, self.L + 3), np.shape(J)
            EJ[0] = self._e_jac(J, self.J[idx])
        else:
            EJ[0] = 0.0
        pos = np.full(self.n, -1, np.int64)
        pos[self.kink_idx] = np.arange(self.kink_idx.size)
        at = np.nonzero(pos[idx] >= 0)[0]                 # candidate rows that are kink points
        kp = pos[idx[at]]
        for c in range(1, n_alt):
            ok = ~np.isnan(self.alt_y[c, kp])
            a, q = at[ok], kp[ok]
            EF[c, a] = np.abs(y[a] - self.alt_y[c, q])
            EJ[c, a] = self._e_jac(np.asarray(J)[a], self.alt_J[c, q]) if J is not None else 0.0
        return EF, EJ

    @staticmethod
    def _best(EF, EJ, uf, uJ):
        c = np.argmin(np.maximum(EF / uf, EJ / uJ), axis=0)
        i = np.arange(EF.shape[1])
        return EF[c, i], EJ[c, i], c

    def judge(self, y, J, r_f, r_J, rows=None):
        """Judge a candidate; ``rows`` (a slice) if it holds only those rows of the point set.
        Returns a dict of figures and ``bad``, the offending rows' indices into the point set."""
        idx = np.arange(self.n) if rows is None else np.arange(self.n)[rows]
        EF, EJ = self._tables(y, J, rows)
        judged = ~self.left_out[idx]
        ok = ((EF <= r_f * self.e32_f) & (EJ <= r_J * self.e32_J)).any(0)
        ef, eJ, c = self._best(EF, EJ, self.e32_f, self.e32_J)
        plain_ok = (EF[0] <= r_f * self.e32_f) & (EJ[0] <= r_J * self.e32_J)
        attributed = judged & ok & ~plain_ok
        pos = np.full(self.n, -1, np.int64)
        pos[self.kink_idx] = np.arange(self.kink_idx.size)
        used = self.alt_margin[c[attributed], pos[idx[attributed]]] if attributed.any() else np.zeros(0)
        w_f = float(ef[judged].max()) if judged.any() else 0.0
        w_J = float(eJ[judged].max()) if judged.any() else 0.0
        return {"worst_f": w_f, "worst_J": w_J, "rho_f": w_f / self.e32_f, "rho_J": w_J / self.e32_J,
                "n_attributed": int(attributed.sum()), "margin_used": float(used.max()) if used.size else 0.0,
                "n_judged": int(judged.sum()), "bad": idx[judged & ~ok], "ef": ef, "eJ": eJ, "idx": idx}

    def report(self, res, limit=40):
        lines = []
        where = {int(i): a for a, i in enumerate(res["idx"])}
        for i in res["bad"][:limit]:
            a = where[int(i)]
            lines.append(f"  point {int(i)} (tile {int(i) // TILE}, lane {int(i) % TILE}): fp64 margin "
                         f"{self.margin[i]:.2e}, k {int(self.k[i])}, e_f {res['ef'][a]:.2e} "
                         f"({res['ef'][a] / self.e32_f:.1f} E32_f), e_J {res['eJ'][a]:.2e} "
                         f"({res['eJ'][a] / self.e32_J:.1f} E32_J)")
        if len(res["bad"]) > limit:
            lines.append(f"  ... and {len(res['bad']) - limit} more")
        return "\n".join(lines)

    def check(self, y, J, r, label, rows=None, quiet=False):
        """Assert the rule for a candidate at bounds r = (r_f, r_J); prints and returns its figures."""
        res = self.judge(y, J, r[0], r[1], rows)
        if not quiet:
            print(f"{label}: n {res['n_judged']} E32 f {self.e32_f:.2e} J {self.e32_J:.2e} | worst f "
                  f"{res['worst_f']:.2e} J {res['worst_J']:.2e} | rho f {res['rho_f']:.2f} J {res['rho_J']:.2f} "
                  f"(bounds {r[0]}, {r[1]}) | kink-attributed {res['n_attributed']}, largest margin used "
                  f"{res['margin_used']:.2e}")
        assert len(res["bad"]) == 0, (f"{label}: {len(res['bad'])} of {res['n_judged']} points beyond "
                                      f"r_f {r[0]} x E32_f {self.e32_f:.2e} or r_J {r[1]} x E32_J "
                                      f"{self.e32_J:.2e} under every admissible ReLU assignment "
                                      f"(m_kink {self.m_kink:.1e}):\n" + self.report(res))
        return res

    def fails(self, y, J, r, rows=None):
        return len(self.judge(y, J, r[0], r[1], rows)["bad"]) > 0
