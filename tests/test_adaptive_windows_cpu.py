"""The window rule of the per-object render passes (choose_windows, dsr_kernels.hpp; DESIGN.md
§3.3), restated in numpy and run on the termination ranks the oracle produces along the golden
F4 trajectory (kitti0, every 4th ray): the tables it chooses are well formed, every sample the
result needs is decoded exactly once, and from the second adapted iteration on fewer samples
are decoded than under the fixed windows."""
from __future__ import annotations

import numpy as np
import pytest

import synthetic as S
from conftest import golden

FIXED = [0, 8, 12, 16, 20, 24, 32, 50]      # the large-batch default schedule, M = 50
INF = 0x3FFFFFFF


def histogram(first, M):
    """ObjState.hist as k_refine_scan fills it: rays by the in-ball rank of their first
    certainly-full sample; rays that never terminate in bin M - 1."""
    t = np.where(first >= 0, np.minimum(first, M - 1), M - 1)
    return np.bincount(t, minlength=M).astype(np.int64)


def choose_windows(hist, cur, M):
    """choose_windows, statement for statement: counts smeared to ranks t - 1 .. t + 2, the P
    windows of least summed over-decode by dynamic programming, ties to the smaller boundary."""
    P = len(cur) - 1
    h0 = np.where(np.arange(64) < M - 1, np.pad(hist, (0, 64 - M)), 0)
    hs = np.zeros(64, np.int64)
    for j in range(64):
        hs[j] = sum(h0[k] for k in (j + 1, j, j - 1, j - 2) if 0 <= k < 64) if j < M else 0
    C = np.concatenate([[0], np.cumsum(hs)])            # C[j]: counts of ranks < j
    W = np.concatenate([[0], np.cumsum(hs * np.arange(64))])
    Ct, Wt = int(C[64]), int(W[64])
    if Ct == 0 or Ct > (1 << 22):
        return list(cur)
    f = [int((j - 1) * C[j] - W[j]) if cur[1] <= j < M else INF for j in range(64)]
    arg = {}
    for p in range(2, P):
        g, arg[p] = [INF] * 64, [0] * 64
        for j in range(M):
            for i in range(1, min(j, M - 1)):
                v = f[i] + (j - 1) * int(C[j] - C[i]) - int(W[j] - W[i])
                if f[i] < INF and v < g[j]:
                    g[j], arg[p][j] = v, i
        f = g
    best, bi = INF, 0
    for i in range(1, M):
        v = f[i] + (M - 1) * (Ct - int(C[i])) - (Wt - int(W[i]))
        if f[i] < INF and v < best:
            best, bi = v, i
    if best >= INF:
        return list(cur)
    w = list(cur)
    for p in range(P - 1, 0, -1):
        w[p] = bi
        if p >= 2:
            bi = arg[p][bi]
    return w


def run_passes(w, nin, first):
    """The render passes with early ray termination on per-ray in-ball counts and first
    certainly-full ranks (-1: none): how often each (ray, rank) is decoded."""
    times = np.zeros((nin.shape[0], 64), np.int32)
    dead = np.zeros(nin.shape[0], bool)
    for ra, rb in zip(w[:-1], w[1:]):
        for r in np.nonzero(~dead)[0]:
            hi = min(rb, nin[r])
            times[r, ra:hi] += 1
            if ra <= first[r] < hi:
                dead[r] = True
    return times


@pytest.fixture(scope="module")
def ranks():
    """Per iteration of the golden trajectory: (in-ball samples per ray, in-ball rank of each
    ray's first certainly-full sample or -1), margins as the lite pass sets them (th in the
    first iteration, the floor 0.002 after)."""
    from deep_sdf.workspace import fold_state
    from oracle import dsr_oracle as O

    dec = O.Decoder(fold_state(S.make_decoder(1234), S.DEFAULT_SPECS))
    P = O.OptimParams.from_cfg(S.KITTI_OPTIM)
    f = golden("f4_traj_kitti0.npz")
    rays, M, th = f["obj_rays"][::4], P.num_depth_samples, P.cut_off
    out = []
    for e in range(int(f["n_iters_run"])):
        T = f["it_t_obj_cam"][e].astype(np.float32)
        obj = O.transform_points(rays[:, None, :] * f["it_depths"][e][:, None], T)
        inb = np.sqrt(np.sum(obj * obj, axis=-1)) < 1.0
        sdf = np.full(inb.shape, np.nan, np.float32)
        sdf[inb] = O.decode_sdf(dec, f["it_z"][e], obj[inb])
        full = inb & (sdf <= -th - (th if e == 0 else 0.002))
        rank = np.cumsum(inb, 1) - 1
        first = np.where(full.any(1), rank[np.arange(rays.shape[0]), full.argmax(1)], -1)
        out.append((inb.sum(1), first))
    return M, out


def test_rule_on_the_golden_trajectory(ranks):
    M, its = ranks
    assert M == FIXED[-1] and len(its) >= 4
    w = list(FIXED)
    dec_fixed, dec_adapt, need_all = [], [], []
    for e, (nin, first) in enumerate(its):
        # the table is well formed
        assert w[0] == 0 and w[-1] == M and len(w) == len(FIXED)
        assert all(a < b for a, b in zip(w[:-1], w[1:])), w
        assert w[1] >= FIXED[1]
        if e == 0:
            assert w == FIXED
        # every sample up to a ray's first certainly-full one (all in-ball ones of a ray that
        # never terminates) is decoded exactly once, none twice
        times = run_passes(w, nin, first)
        need = np.where(first >= 0, first + 1, nin)
        for r in range(nin.shape[0]):
            assert (times[r, :need[r]] == 1).all(), (e, r)
        assert times.max() <= 1
        dec_adapt.append(int(times.sum()))
        dec_fixed.append(int(run_passes(FIXED, nin, first).sum()))
        need_all.append(int(need.sum()))
        w = choose_windows(histogram(first, M), w, M)
    print("decoded / needed per iteration: fixed",
          [round(a / b, 4) for a, b in zip(dec_fixed, need_all)], "adaptive",
          [round(a / b, 4) for a, b in zip(dec_adapt, need_all)])
    assert dec_adapt[0] == dec_fixed[0]
    for e in range(2, len(its)):
        assert dec_adapt[e] <= dec_fixed[e], (e, dec_adapt, dec_fixed)
    assert sum(dec_adapt[2:]) < sum(dec_fixed[2:])


def test_no_history_keeps_the_table():
    assert choose_windows(np.zeros(50, np.int64), FIXED, 50) == FIXED
    never = np.zeros(50, np.int64)
    never[49] = 1000                       # rays that never terminate are no history either
    assert choose_windows(never, FIXED, 50) == FIXED


def test_rule_is_the_least_over_decode_of_the_smeared_counts():
    """Against brute force over all tables, two windows to four, on random small histograms."""
    from itertools import combinations

    rng = np.random.default_rng(5)
    M = 12
    for trial in range(20):
        P = 2 + trial % 3
        cur = [0] + sorted(rng.choice(np.arange(2, M), P - 1, replace=False).tolist()) + [M]
        hist = rng.integers(0, 30, M)
        w = choose_windows(hist, cur, M)
        h0 = np.where(np.arange(M) < M - 1, hist, 0)
        hs = np.array([sum(h0[k] for k in (j + 1, j, j - 1, j - 2) if 0 <= k < M) for j in range(M)])

        def cost(t):
            return sum(hs[r] * (b - 1 - r) for a, b in zip(t[:-1], t[1:]) for r in range(a, b))

        best = min(cost([0, *c, M]) for c in combinations(range(cur[1], M), P - 1))
        assert w[0] == 0 and w[-1] == M and w[1] >= cur[1] and all(a < b for a, b in zip(w[:-1], w[1:]))
        assert cost(w) == best, (cur, w, best)
