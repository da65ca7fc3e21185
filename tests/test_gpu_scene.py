"""Scene SDF queries on the GPU (dsr_scene_*, SceneSdf) against the numpy
restatement of the algorithm (tests/scene_oracle.py) over the float64 oracle decoder, and bitwise
against what the build already has (dsr_scene_bin_host, sdf_eval).

Scene (tests/scene_oracle.py): four objects, scales 2.0 / 1.5 / 1.0 / 2.5, and n = 1500 or 400
points uniform in a box around them.  Per-object candidate counts 480 / 194 / 56 / 598 (none a
multiple of 64, one under a tile, three over several tiles; 1038 points in a ball, 275 in two or
more) and 141 / 53 / 17 / 152.  Confirmed with the oracle alone (fp32 numpy against fp64): the
smallest |r^2 - 1| is 3.4e-4, so membership cannot flip, and no point has its two nearest distances
within 1e-4 of each other, so the winner cannot flip within the 2e-5 s bound.  The tests re-assert
these conditions on the oracle side before they judge the GPU.
"""
from __future__ import annotations

import numpy as np
import pytest

import scene_oracle as SO
import synthetic as S
from conftest import assert_jac_close

pytestmark = pytest.mark.gpu

F_TOL = 2e-5                 # the exact kernel against fp64 on f (tests/test_gpu_parity.py)
MAX_OBJ, MAX_PTS = 8, 2048
_SCENES = {}
_ORACLE = {}


def scene(dec, code_len=64, key=0):
    """one SceneSdf per (decoder, key), kept for the module"""
    from reconstruct.optimizer import SceneSdf

    k = (id(dec), key)
    if k not in _SCENES:
        _SCENES[k] = (dec, SceneSdf(dec, MAX_OBJ, MAX_PTS, code_len=code_len))
    return _SCENES[k][1]


@pytest.fixture(scope="module")
def dec64(full_layers):
    from oracle.dsr_oracle import Decoder

    return Decoder(full_layers, 64, (4,), dtype=np.float64)


def oracle(dec64, n):
    """the float64 restatement of the four-object scene at n points, computed once"""
    if n not in _ORACLE:
        objs = SO.scene_objects()
        _ORACLE[n] = SO.query([SO.decoder_sdf(dec64, z) for _, z in objs], [t for t, _ in objs], SO.scene_points(n),
                              [SO.decoder_grad(dec64, z) for _, z in objs])
    return _ORACLE[n]


def same_bytes(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_scene_conditions(ref, n):
    """what makes the exact comparisons below legitimate; a changed recipe fails here"""
    assert tuple(r.n_in for r in ref.objects) == SO.COUNTS[n]
    r2 = np.stack([r.r2 for r in ref.objects])
    assert np.abs(r2 - 1.0).min() > 1e-4
    d = np.sort(ref.d_all, axis=0)
    two = np.isfinite(d[1])
    assert two.sum() > 20
    gap = (d[1][two] - d[0][two]).min()
    assert gap >= 2 * F_TOL * max(SO.SCALES), gap
    if n == 1500:
        assert int(np.isfinite(d[0]).sum()) == 1038 and int(two.sum()) == 275
        assert int((ref.dist < 0).sum()) == 153


def check_against_oracle(out, peeks, ref, label):
    s = np.array([r.s for r in ref.objects])
    hit = ref.obj >= 0
    assert np.array_equal(out["obj"], ref.obj)
    assert np.all(np.isposinf(out["dist"][~hit]))
    err = np.abs(out["dist"][hit].astype(np.float64) - ref.dist[hit]) / s[ref.obj[hit]]
    print(f"{label}: in a ball {int(hit.sum())}, worst |dist - dist64| / s {err.max():.3e}")
    assert err.max() <= F_TOL
    assert sum(o["n_win"] for o in out["objects"]) == int(hit.sum())
    for i, (o, r) in enumerate(zip(out["objects"], ref.objects)):
        idx, _, f = peeks[i]
        assert o["n_in"] == r.n_in and np.array_equal(idx, r.idx)                   # membership, exact
        assert o["n_win"] == r.n_win and o["n_nan"] == 0
        assert np.abs(f.astype(np.float64) - r.f).max() <= F_TOL
        close = int((np.abs(r.f) <= F_TOL).sum())
        assert abs(o["n_neg"] - r.n_neg) <= close, (o["n_neg"], r.n_neg, close)
        em = abs(o["sum_sdf"] / o["n_in"] - r.sum_sdf / r.n_in)
        ea = abs(o["sum_abs"] / o["n_in"] - r.sum_abs / r.n_in)
        print(f"{label} object {i}: n_in {o['n_in']} n_win {o['n_win']} n_neg {o['n_neg']}/{r.n_neg} "
              f"mean err {em:.3e} abs-mean err {ea:.3e}")
        assert em <= F_TOL and ea <= F_TOL
        assert o["mean_sdf"] == o["sum_sdf"] / o["n_in"]


@pytest.mark.parametrize("n", [1500, 400])
def test_against_the_fp64_restatement(gpu_decoder, dec64, n):
    ref = oracle(dec64, n)
    assert_scene_conditions(ref, n)
    sc = scene(gpu_decoder)
    sc.set_objects(SO.scene_objects())
    out = sc.query(SO.scene_points(n))
    assert out["grad"] is None and out["dist"].dtype == np.float32 and out["obj"].dtype == np.int32
    check_against_oracle(out, [sc.peek(i) for i in range(4)], ref, f"n {n}")
    st = sc.stats()
    assert st["n_obj"] == 4 and st["n_pts"] == n and st["n_passes"] == 1 and st["pairs"] == 4 * n
    assert st["decoded"] == sum(SO.COUNTS[n]) and st["winners"] == int((ref.obj >= 0).sum())
    assert st["bin_ms"] > 0 and st["decode_ms"] > 0 and st["resolve_ms"] > 0 and st["grad_ms"] == 0


def host_grad(t, g):
    """s * (A_0k g_0 + A_1k g_1 + A_2k g_2) in float64 and its magnitude sum"""
    A, _, s = SO.pose(t)
    g = g.astype(np.float64)
    return s * (g @ A), s * (np.abs(g) @ np.abs(A))


def test_bitwise_against_bin_host_and_sdf_eval(gpu_decoder):
    from reconstruct.optimizer import scene_bin, sdf_eval

    objs = SO.scene_objects()
    pts = SO.scene_points(1500)
    sc = scene(gpu_decoder)
    sc.set_objects(objs)
    out = sc.query(pts, grad=True)
    assert sc.stats()["grad_ms"] > 0
    dist = np.full(1500, np.inf, np.float32)
    for i, (t, z) in enumerate(objs):
        idx, x, f = sc.peek(i)
        hidx, hx, s = scene_bin(objs, pts, i)
        assert same_bytes(idx, hidx) and same_bytes(x, hx)
        assert same_bytes(f, sdf_eval(gpu_decoder, z, x))           # the same tiles, so the same values
        mine = out["obj"][idx] == i
        assert same_bytes(out["dist"][idx[mine]], (np.float32(s) * f)[mine])
        dist[idx] = np.minimum(dist[idx], np.float32(s) * f)
        # the winners, in point order, through the Jacobian query
        assert mine.sum() > 20
        _, j = sdf_eval(gpu_decoder, z, x[mine], with_jac=True)
        want, mag = host_grad(t, j[:, -3:])
        got = out["grad"][idx[mine]].astype(np.float64)
        assert np.all(np.abs(got - want) <= 1e-6 * mag + 1e-30), float((np.abs(got - want) / (mag + 1e-30)).max())
    assert same_bytes(out["dist"], dist)
    # identity pose: the query is sdf_eval
    p = np.random.default_rng(11).standard_normal((200, 3))
    p = (p / np.linalg.norm(p, axis=1, keepdims=True) * 0.9 * np.random.default_rng(12).uniform(0, 1, (200, 1)) ** (1 / 3))
    p = p.astype(np.float32)
    z = SO.scene_code(1)
    sc.set_objects([(np.eye(4, dtype=np.float32), z)])
    one = sc.query(p)
    assert np.all(one["obj"] == 0) and one["objects"][0]["n_in"] == 200
    assert same_bytes(one["dist"], sdf_eval(gpu_decoder, z, p))


def test_gradient_against_fp64(gpu_decoder, dec64):
    ref = oracle(dec64, 1500)
    assert_scene_conditions(ref, 1500)
    sc = scene(gpu_decoder)
    sc.set_objects(SO.scene_objects())
    out = sc.query(SO.scene_points(1500), grad=True)
    plain = sc.query(SO.scene_points(1500))
    assert same_bytes(out["dist"], plain["dist"]) and same_bytes(out["obj"], plain["obj"])
    hit = out["obj"] >= 0
    assert np.array_equal(out["obj"], ref.obj) and hit.sum() == 1038
    assert out["grad"].dtype == np.float32 and out["grad"].shape == (1500, 3)
    assert_jac_close(out["grad"][hit], ref.grad[hit], tol=1e-4)
    assert np.all(out["grad"][~hit] == 0.0)


def record(sc, i):
    return tuple(a.tobytes() for a in sc.peek(i))


def sums(o):
    return (o["n_in"], o["n_neg"], o["n_nan"], o["sum_sdf"], o["sum_abs"])


def test_independent_of_the_other_objects_and_reproducible(gpu_decoder, monkeypatch):
    objs = SO.scene_objects()
    pts = SO.scene_points(1500)
    sc = scene(gpu_decoder)
    sc.set_objects(objs)
    four = sc.query(pts, grad=True)
    peeks = [record(sc, i) for i in range(4)]
    assert sc.stats()["n_passes"] == 1
    # two consecutive queries
    again = sc.query(pts, grad=True)
    for k in ("dist", "obj", "grad"):
        assert same_bytes(four[k], again[k]), k
    assert [dict(o) for o in four["objects"]] == [dict(o) for o in again["objects"]]
    # each object alone
    for i in range(4):
        sc.set_objects([objs[i]])
        alone = sc.query(pts)
        assert record(sc, 0) == peeks[i] and sums(alone["objects"][0]) == sums(four["objects"][i])
        assert alone["objects"][0]["n_win"] == alone["objects"][0]["n_in"]
    # the four in reversed order: the same distances, the indices mirrored
    sc.set_objects(objs[::-1])
    rev = sc.query(pts, grad=True)
    for i in range(4):
        assert record(sc, 3 - i) == peeks[i] and sums(rev["objects"][3 - i]) == sums(four["objects"][i])
        assert rev["objects"][3 - i]["n_win"] == four["objects"][i]["n_win"]        # (no ties in this scene)
    hit = four["obj"] >= 0
    assert same_bytes(rev["dist"], four["dist"]) and same_bytes(rev["grad"], four["grad"])
    assert np.array_equal(rev["obj"][hit], 3 - four["obj"][hit]) and np.all(rev["obj"][~hit] == -1)
    # one and three objects per pass against all in one pass
    sc.set_objects(objs)
    monkeypatch.setenv("DSR_TEST_HOOKS", "1")
    for k_pass, n_pass in (("1", 4), ("3", 2)):
        monkeypatch.setenv("DSR_SCENE_PASS_OBJ", k_pass)
        split = sc.query(pts, grad=True)
        assert sc.stats()["n_passes"] == n_pass
        for k in ("dist", "obj", "grad"):
            assert same_bytes(four[k], split[k]), (k_pass, k)
        assert [dict(o) for o in four["objects"]] == [dict(o) for o in split["objects"]]
        assert [record(sc, i) for i in (2, 0, 3, 1)] == [peeks[i] for i in (2, 0, 3, 1)]   # earlier passes too
    monkeypatch.delenv("DSR_TEST_HOOKS")
    sc.query(pts)
    assert sc.stats()["n_passes"] == 1                   # the hook is ignored without DSR_TEST_HOOKS=1
    # a second SceneSdf
    other = scene(gpu_decoder, key=1)
    other.set_objects(objs)
    second = other.query(pts, grad=True)
    for k in ("dist", "obj", "grad"):
        assert same_bytes(four[k], second[k]), k
    assert [dict(o) for o in four["objects"]] == [dict(o) for o in second["objects"]]
    assert [record(other, i) for i in range(4)] == peeks


def test_edges(gpu_decoder):
    from reconstruct import _libdsr as L

    objs = SO.scene_objects()
    pts = SO.scene_points(400)
    sc = scene(gpu_decoder)
    sc.set_objects(objs)
    base = sc.query(pts, grad=True)
    base_peeks = [record(sc, i) for i in range(4)]
    # a fifth object nobody is inside of
    far = (SO.scene_pose(0, scale=1.0, centre=(50.0, 50.0, 50.0)), SO.scene_code(2))
    sc.set_objects(objs + [far])
    five = sc.query(pts, grad=True)
    assert sums(five["objects"][4]) == (0, 0, 0, 0.0, 0.0) and five["objects"][4]["n_win"] == 0
    assert np.isnan(five["objects"][4]["mean_sdf"]) and sc.peek(4)[0].size == 0
    for k in ("dist", "obj", "grad"):
        assert same_bytes(base[k], five[k]), k
    assert [dict(o) for o in five["objects"][:4]] == [dict(o) for o in base["objects"]]
    with pytest.raises(L.DsrError):
        sc.peek(5)
    # a NaN and an inf point: in no ball; the balls that held neither are bitwise unchanged
    sc.set_objects(objs)
    members = [set(np.frombuffer(p[0], np.int32).tolist()) for p in base_peeks]
    only0 = sorted(members[0] - members[1] - members[2] - members[3])
    a, b = only0[0], only0[1]
    bad = pts.copy()
    bad[a, 1] = np.nan
    bad[b, 0] = np.inf
    out = sc.query(bad, grad=True)
    for p in (a, b):
        assert np.isposinf(out["dist"][p]) and out["obj"][p] == -1 and np.all(out["grad"][p] == 0.0)
    assert out["objects"][0]["n_in"] == base["objects"][0]["n_in"] - 2
    for i in (1, 2, 3):
        assert record(sc, i) == base_peeks[i] and sums(out["objects"][i]) == sums(base["objects"][i])
    won_elsewhere = np.nonzero(base["obj"] != 0)[0]      # (a and b were won by object 0)
    for k in ("dist", "obj", "grad"):
        assert same_bytes(out[k][won_elsewhere], base[k][won_elsewhere]), k
    # no points, no objects
    e = sc.query(np.zeros((0, 3), np.float32), grad=True)
    assert e["dist"].shape == (0,) and e["obj"].shape == (0,) and e["grad"].shape == (0, 3)
    assert [o["n_in"] for o in e["objects"]] == [0] * 4 and sc.stats()["n_passes"] == 0
    sc.set_objects([])
    e = sc.query(pts, grad=True)
    assert np.all(np.isposinf(e["dist"])) and np.all(e["obj"] == -1) and np.all(e["grad"] == 0.0) and e["objects"] == []
    with pytest.raises(L.DsrError):
        sc.peek(0)
    # set_objects twice with different codes: the second is used
    swapped = [(objs[i][0], objs[(i + 1) % 4][1]) for i in range(4)]
    sc.set_objects(swapped)
    other = sc.query(pts)
    assert not same_bytes(other["dist"], base["dist"])
    sc.set_objects(objs)
    back = sc.query(pts, grad=True)
    for k in ("dist", "obj", "grad"):
        assert same_bytes(base[k], back[k]), k
    # the same pose and code twice: the lower index wins every point
    sc.set_objects([objs[3], objs[3]])
    tie = sc.query(pts)
    assert np.all(tie["obj"][tie["obj"] >= 0] == 0) and tie["objects"][1]["n_win"] == 0
    assert tie["objects"][0]["n_win"] == tie["objects"][0]["n_in"] == tie["objects"][1]["n_in"] == 152
    assert sums(tie["objects"][0]) == sums(tie["objects"][1])


def test_argument_errors(gpu_decoder):
    from reconstruct import _libdsr as L
    from reconstruct.optimizer import SceneSdf

    for bad in ((0, 16), (4, 0), (4, (1 << 24) + 1)):
        with pytest.raises(L.DsrError):
            SceneSdf(gpu_decoder, *bad)
    fresh = SceneSdf(gpu_decoder, 2, 64)
    pts = SO.scene_points(400)
    with pytest.raises(L.DsrError, match="before dsr_scene_set_objects"):
        fresh.query(pts[:10])
    objs = SO.scene_objects()
    with pytest.raises(L.DsrError, match="max_obj"):
        fresh.set_objects(objs[:3])
    fresh.set_objects(objs[:2])
    with pytest.raises(L.DsrError, match="max_pts"):
        fresh.query(pts[:65])
    ref = fresh.query(pts[:64])
    row, mirror, nanp = SO.scene_pose(1), SO.scene_pose(1), SO.scene_pose(1)
    row[3, 3] = 2.0
    mirror[:3, 0] *= -1.0
    nanp[0, 3] = np.nan
    for t in (row, mirror, nanp):
        with pytest.raises(L.DsrError, match="t_world_obj"):
            fresh.set_objects([objs[0], (t, objs[1][1])])
    zbad = objs[1][1].copy()
    zbad[5] = np.inf
    with pytest.raises(L.DsrError, match="code must be finite"):
        fresh.set_objects([objs[0], (objs[1][0], zbad)])
    with pytest.raises(ValueError):
        fresh.set_objects([(objs[0][0], objs[0][1][:63])])
    # a refused set_objects returns before the device: the map set before it is still the one queried
    assert same_bytes(fresh.query(pts[:64])["dist"], ref["dist"])
    fresh.set_objects(objs[:2])
    assert same_bytes(fresh.query(pts[:64])["dist"], ref["dist"])     # the scene survives its errors
    ctx = gpu_decoder.ctx
    assert ctx.lib.dsr_scene_query(fresh._h, 4, None, None, None, None, None) < 0
    n = np.zeros(1, np.int32)
    assert ctx.lib.dsr_scene_peek(fresh._h, 0, 0, None, None, None, L.iptr(n)) == -5 and n[0] > 0
    fresh.close()
    with pytest.raises(L.DsrError):
        fresh.query(pts[:4])


def test_code32_decoder_queries():
    from deep_sdf.workspace import decoder_from_state
    from oracle.dsr_oracle import Decoder
    from test_gpu_code32 import SPECS32

    state = S.make_decoder(1234, SPECS32)
    dec = decoder_from_state(state, SPECS32)
    o64 = Decoder.from_state(state, SPECS32, dtype=np.float64)
    objs = SO.scene_objects(code_len=32)
    pts = SO.scene_points(400)
    ref = SO.query([SO.decoder_sdf(o64, z) for _, z in objs], [t for t, _ in objs], pts,
                   [SO.decoder_grad(o64, z) for _, z in objs])
    assert tuple(r.n_in for r in ref.objects) == SO.COUNTS[400]
    d = np.sort(ref.d_all, axis=0)
    two = np.isfinite(d[1])
    assert (d[1][two] - d[0][two]).min() >= 2 * F_TOL * max(SO.SCALES)
    sc = scene(dec, code_len=32)
    sc.set_objects(objs)
    out = sc.query(pts, grad=True)
    check_against_oracle(out, [sc.peek(i) for i in range(4)], ref, "code32")
    hit = out["obj"] >= 0
    assert_jac_close(out["grad"][hit], ref.grad[hit], tol=1e-4)
