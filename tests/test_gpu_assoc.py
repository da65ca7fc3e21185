"""Data association on the GPU (dsr_scene_associate_points / _frame, SceneSdf.associate_*; DESIGN.md
§3.6d) against the float64 restatement (tests/assoc_oracle.py over tests/scene_oracle.py), against
SceneSdf.query / peek on the same points, and the frame form against the points form on the host
twin's rows.  Scene (tests/assoc_cases.py): four objects, six detections at max_pts = 65; candidate
counts 116 / 44 / 53 / 94, the smallest ||f| - 0.05| 5.4e-3 and the smallest |r^2 - 1| 4.6e-4, both
far above the exact kernel's 2e-5, so no membership and no class can flip: the GPU tables must
equal the oracle's, without a tolerance.  The tests re-assert these conditions on the oracle side
before they judge the GPU."""
from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import assoc_cases as AC
import assoc_oracle as AO
import scene_oracle as SO
import synthetic as S
from conftest import PKG, REPO

pytestmark = pytest.mark.gpu

RW, RH = 100, 75
RCAM = dict(width=RW, height=RH, fx=165.0, fy=165.0, cx=49.5, cy=37.0)
SUB = dict(max_pts=65, min_mask_area=10, far=100.0)        # sub-sampled: two tiles per rendered object, the second of one row
ALL = dict(max_pts=4096, min_mask_area=10, far=100.0)      # every valid pixel
LABELS = (0, 1, 7, 8, 9, 55, 0)                            # 55 is absent; label 0 twice
MAX_OBJ, MAX_PTS = 8, len(LABELS) * ALL["max_pts"]
_SCENES = {}


def scene(dec):
    """one SceneSdf per decoder, kept for the module"""
    from reconstruct.optimizer import SceneSdf

    if id(dec) not in _SCENES:
        _SCENES[id(dec)] = (dec, SceneSdf(dec, MAX_OBJ, MAX_PTS))
    return _SCENES[id(dec)][1]


@pytest.fixture(scope="module")
def dec64(full_layers):
    from oracle.dsr_oracle import Decoder

    return Decoder(full_layers, 64, (4,), dtype=np.float64)


def tables(out):
    return tuple(out[k].tobytes() for k in ("n_in", "n_hit", "n_neg")) + tuple(out[k].shape for k in ("n_in", "n_hit", "n_neg"))


def records(out):
    return [dict(r) for r in out["records"]]


def peeks(sc, n_obj):
    return [tuple(a.tobytes() for a in sc.peek(i)) for i in range(n_obj)]


def vote_over_query(sc, pts, n_det, max_pts, n_obj, **kw):
    """the numpy vote over SceneSdf.query + peek on the strided points: (n_in, n_hit, n_neg), the peeks' bytes"""
    sc.query(pts)
    got = [sc.peek(i) for i in range(n_obj)]
    return AO.vote([(idx, f) for idx, _, f in got], n_det, max_pts, **kw), [tuple(a.tobytes() for a in p) for p in got]


BIG = 64.0


def device_points(sc, call, n_slots):
    """The world points a call writes into the scene's point buffer, read back exactly.  The map is
    one object with the pose diag(64, 64, 64, 1), whose ball covers every row of these tests; its
    inverse is exactly 2^-6 on the diagonal, so peek returns every non-NaN slot's index and
    x_k = fmaf(2^-6, w_k, 0) = w_k / 64 without a rounding, and w = 64 x bitwise.  The slots peek does
    not return are in no ball: with this object, the NaN fill.  The points do not depend on the map."""
    sc.set_objects([(np.diag([BIG, BIG, BIG, 1.0]).astype(np.float32), SO.scene_code(1))])
    out = call()
    idx, x, _ = sc.peek(0)
    assert idx.shape[0] == sum(r.n_pts for r in out["records"]) == int(out["n_in"].sum())
    pts = np.full((n_slots, 3), np.nan, np.float32)
    pts[idx] = x * np.float32(BIG)
    return pts


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def rigid(seed, t):
    T = np.eye(4)
    T[:3, :3] = SO.rotation(seed)
    T[:3, 3] = t
    return T


# ------------------------------------------------------------------ 1. the points form against the fp64 oracle
def test_points_equal_the_fp64_oracle_and_the_query(gpu_decoder, dec64):
    want_recs = AC.assert_conditions(dec64)
    pts, n_rows, ref, (n_in, n_hit, n_neg) = AC.oracle(dec64)
    sc = scene(gpu_decoder)
    sc.set_objects(SO.scene_objects())
    out = sc.associate_points(AC.detections(dec64), max_pts=AC.MAX_PTS)
    print("n_hit", out["n_hit"].tolist())
    print("n_in", out["n_in"].tolist())
    print("n_neg", out["n_neg"].tolist(), "oracle", n_neg.tolist())
    for k, want in (("n_in", n_in), ("n_hit", n_hit), ("n_neg", n_neg)):
        assert out[k].dtype == np.int32 and out[k].shape == (AC.N_DET, AC.N_OBJ)
        assert np.array_equal(out[k], want), k                         # no tolerance, no allowance
    assert records(out) == want_recs
    st = sc.stats()
    assert st["n_obj"] == 4 and st["n_pts"] == AC.N_DET * AC.MAX_PTS and st["n_passes"] == 1
    assert st["decoded"] == sum(AC.COUNTS)
    after = peeks(sc, 4)                                                # the call's own candidates
    for i, r in enumerate(ref.objects):
        idx, _, f = sc.peek(i)
        assert np.array_equal(idx, r.idx) and np.abs(f.astype(np.float64) - r.f).max() <= AC.F_TOL
    # the same strided points through query / peek: the values and indices reproduce the tables bitwise
    (q_in, q_hit, q_neg), q_peeks = vote_over_query(sc, pts, AC.N_DET, AC.MAX_PTS, 4)
    assert q_peeks == after
    assert np.array_equal(q_in, out["n_in"]) and np.array_equal(q_hit, out["n_hit"]) and np.array_equal(q_neg, out["n_neg"])
    # other thresholds are taken literally
    tight = sc.associate_points(AC.detections(dec64), max_pts=AC.MAX_PTS, min_hits=22, inlier_tol=0.01)
    t_tabs, _ = vote_over_query(sc, pts, AC.N_DET, AC.MAX_PTS, 4, inlier_tol=0.01)
    assert all(np.array_equal(a, tight[k]) for a, k in zip(t_tabs, ("n_in", "n_hit", "n_neg")))
    assert records(tight) == AO.pick(*t_tabs, n_rows, inlier_tol=0.01, min_hits=22)
    assert tight["records"][5].status == AO.NEW


# ------------------------------------------------------------------ 2. camera-frame rows and t_world_cam
def test_camera_rows_go_to_the_world_as_the_host_twin_says(gpu_decoder, dec64):
    import lidar_oracle as LO

    rows = AC.detections(dec64)
    t_cam_world = rigid(5, (0.3, -0.7, 1.9))
    t_world_cam = np.linalg.inv(t_cam_world).astype(np.float32)
    cam_rows = [(r.astype(np.float64) @ t_cam_world[:3, :3].T + t_cam_world[:3, 3]).astype(np.float32) for r in rows]
    before = LO.SUSPECTS
    twin, n_rows = AO.strided(cam_rows, AC.MAX_PTS, t_world_cam)        # the host twin's world points
    assert LO.SUSPECTS == before
    assert np.abs(twin[~np.isnan(twin)] - AO.strided(rows, AC.MAX_PTS)[0][~np.isnan(twin)]).max() < 1e-5
    sc = scene(gpu_decoder)
    sc.set_objects(SO.scene_objects())
    out = sc.associate_points(cam_rows, t_world_cam, max_pts=AC.MAX_PTS)
    dev = peeks(sc, 4)                           # indices, object-frame coordinates and values of the device's points
    tabs, host = vote_over_query(sc, twin, AC.N_DET, AC.MAX_PTS, 4)
    assert dev == host                           # bitwise: the device's world points are the twin's
    assert all(np.array_equal(a, out[k]) for a, k in zip(tabs, ("n_in", "n_hit", "n_neg")))
    assert records(out) == AO.pick(*tabs, n_rows)
    assert [r.status for r in out["records"]] == [d[0] for d in AC.DECISIONS]
    assert [r.obj for r in out["records"]] == [d[1] for d in AC.DECISIONS]
    # the point buffer itself, every slot: bitwise the host twin's, NaN fill included
    got = device_points(sc, lambda: sc.associate_points(cam_rows, t_world_cam, max_pts=AC.MAX_PTS), AC.N_DET * AC.MAX_PTS)
    assert np.abs(twin[~np.isnan(twin)]).max() < BIG / 2
    assert np.array_equal(bits(got), bits(twin))
    assert int(np.isnan(got).all(1).sum()) == AC.N_DET * AC.MAX_PTS - sum(AC.N_ROWS)


# ------------------------------------------------------------------ 3. objects per pass
CHILD = r"""
import json, sys
import numpy as np
sys.path[:0] = [sys.argv[2], sys.argv[3], sys.argv[4]]
import scene_oracle as SO
import synthetic as S
from deep_sdf.workspace import decoder_from_state
from reconstruct.optimizer import SceneSdf
z = np.load(sys.argv[1])
rows = [z["r%d" % j] for j in range(len(z.files))]
dec = decoder_from_state(S.make_decoder(1234), S.DEFAULT_SPECS)
sc = SceneSdf(dec, 4, 6 * 65)
sc.set_objects(SO.scene_objects())
out = sc.associate_points(rows, max_pts=65)
print(json.dumps(dict(n_in=out["n_in"].tolist(), n_hit=out["n_hit"].tolist(), n_neg=out["n_neg"].tolist(),
                      records=[dict(r) for r in out["records"]], n_passes=sc.stats()["n_passes"])))
sc.close()
"""


@pytest.mark.parametrize("k_pass,n_pass", [("1", 4), ("3", 2)])
def test_tables_do_not_depend_on_the_objects_per_pass(gpu_decoder, dec64, tmp_path, k_pass, n_pass):
    rows = AC.detections(dec64)
    sc = scene(gpu_decoder)
    sc.set_objects(SO.scene_objects())
    base = sc.associate_points(rows, max_pts=AC.MAX_PTS)
    assert sc.stats()["n_passes"] == 1
    path = str(tmp_path / "rows.npz")
    np.savez(path, **{f"r{j}": r for j, r in enumerate(rows)})
    env = dict(os.environ, DSR_TEST_HOOKS="1", DSR_SCENE_PASS_OBJ=k_pass)
    p = subprocess.run([sys.executable, "-c", CHILD, path, PKG, REPO, os.path.join(REPO, "tests")], env=env, cwd=REPO,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    assert got["n_passes"] == n_pass
    for k in ("n_in", "n_hit", "n_neg"):
        assert got[k] == base[k].tolist(), k
    assert got["records"] == records(base)


# ------------------------------------------------------------------ 4. a detection's result is its own
def test_independent_of_the_other_detections(gpu_decoder, dec64):
    rows = AC.detections(dec64)
    sc = scene(gpu_decoder)
    sc.set_objects(SO.scene_objects())
    base = sc.associate_points(rows, max_pts=AC.MAX_PTS)
    again = sc.associate_points(rows, max_pts=AC.MAX_PTS)
    assert tables(base) == tables(again) and records(base) == records(again)
    perm = (4, 2, 5, 0, 3, 1)
    out = sc.associate_points([rows[j] for j in perm], max_pts=AC.MAX_PTS)
    for new, old in enumerate(perm):
        for k in ("n_in", "n_hit", "n_neg"):
            assert np.array_equal(out[k][new], base[k][old]), (k, old)
        assert dict(out["records"][new]) == dict(base["records"][old]), old
    # another stride, fewer detections: the rows of the tables stay
    wide = sc.associate_points([rows[4], rows[0]], max_pts=200)
    for new, old in enumerate((4, 0)):
        for k in ("n_in", "n_hit", "n_neg"):
            assert np.array_equal(wide[k][new], base[k][old]), (k, old)
        assert dict(wide["records"][new]) == dict(base["records"][old]), old


# ------------------------------------------------------------------ 5. the frame form
def _valid(depth, inst, label, p=SUB):
    return (inst == label) & (depth > 0.01) & (depth < p["far"])


def _codes():
    return [((0.0, 0.1)[i] * np.random.default_rng(100 + i).standard_normal(64)).astype(np.float32) for i in range(2)]


@pytest.fixture(scope="module")
def frame(gpu_decoder):
    """(depth, instance, camera-frame Sim(3) of the two rendered objects): the recipe of
    tests/test_gpu_track_frame.py — two rendered objects, then label 7 = a 5 x 6 patch of object 1
    (30 valid pixels), label 8 = a 3 x 3 patch of it (at most min_mask_area pixels), label 9 = a
    4 x 4 patch without depth, and 40 pixels of object 0 pushed 0.3 object scales away along their
    rays."""
    from reconstruct.optimizer import SdfRenderer

    sim3 = []
    for i, t in enumerate(((-2.6, 0.1, 15.0), (2.6, -0.2, 15.5))):
        T = S.make_object(7 + i, n_pts=8, scale=2.0, tz=15, perturb=0).t_true.copy()
        T[:3, 3] = t
        sim3.append(T.astype(np.float32))
    ren = SdfRenderer(gpu_decoder, RW, RH, RCAM["fx"], RCAM["fy"], RCAM["cx"], RCAM["cy"])
    img = ren.render([(sim3[i], _codes()[i]) for i in range(2)])
    ren.close()
    depth, inst = img["depth"].copy(), img["instance"].copy()
    scales = [float(np.cbrt(np.linalg.det(T[:3, :3].astype(np.float64)))) for T in sim3]
    v1, u1 = np.nonzero(_valid(depth, inst, 1))
    cv, cu = int(np.median(v1)), int(np.median(u1))
    inst[cv:cv + 5, cu:cu + 6] = 7
    inst[cv - 9:cv - 6, cu - 2:cu + 1] = 8
    assert np.all(inst[0:4, 0:4] == -1)
    inst[0:4, 0:4] = 9
    depth[0:4, 0:4] = 0.0
    v0, u0 = np.nonzero(_valid(depth, inst, 0))
    pick = np.linspace(0, v0.shape[0] - 1, 40).astype(np.int64)
    rx, ry = (u0[pick] - RCAM["cx"]) / RCAM["fx"], (v0[pick] - RCAM["cy"]) / RCAM["fy"]
    depth[v0[pick], u0[pick]] += (0.3 * scales[0] / np.sqrt(rx * rx + ry * ry + 1.0)).astype(np.float32)
    assert _valid(depth, inst, 0).sum() > 65 and _valid(depth, inst, 1).sum() > 65
    assert _valid(depth, inst, 7).sum() == 30 == (inst == 7).sum()
    assert 0 < (inst == 8).sum() <= SUB["min_mask_area"]
    assert (inst == 9).sum() > SUB["min_mask_area"] and _valid(depth, inst, 9).sum() == 0
    assert not (inst == 55).any()
    return depth, inst, sim3


@pytest.mark.parametrize("params", [SUB, ALL], ids=["max_pts65", "max_pts4096"])
def test_frame_equals_the_points_form_on_the_host_rows(gpu_decoder, frame, params):
    from reconstruct import _libdsr as L
    from reconstruct import utils as U

    depth, inst, sim3 = frame
    t_world_cam = rigid(9, (1.5, 0.4, -2.0)).astype(np.float32)
    t64 = t_world_cam.astype(np.float64)
    far = SO.scene_pose(0, scale=1.0, centre=(50.0, 50.0, 50.0))
    objs = [((t64 @ sim3[i].astype(np.float64)).astype(np.float32), _codes()[i]) for i in range(2)] + [(far, SO.scene_code(2))]
    sc = scene(gpu_decoder)
    sc.set_objects(objs)
    out = sc.associate_frame(depth, inst, LABELS, RCAM, t_world_cam, **params)
    dev = peeks(sc, 3)
    host = [dict(label=k, t_cam_obj=np.eye(4, dtype=np.float32)) for k in LABELS]
    hobjs, hrecs = U.frame_inputs(depth, inst, host, RCAM, **params)
    want = sc.associate_points([o[1] for o in hobjs], t_world_cam, max_pts=params["max_pts"])
    assert tables(out) == tables(want)                                   # bitwise
    assert dev == peeks(sc, 3)                                           # the same points, candidates and values
    ingest = lambda r: dict(ingest_status=r.status, n_mask=r.n_mask, n_valid=r.n_valid)  # noqa: E731
    assert records(out) == [dict(dict(r), **ingest(h)) for r, h in zip(want["records"], hrecs)]
    print([(r.status, r.obj, r.n_pts, r.n_hit, r.n_in, r.n_neg, r.ingest_status) for r in out["records"]])
    # the points are the host twin's, and the decision is the numpy rule's
    twin, n_rows, trecs = U.assoc_points(depth, inst, LABELS, RCAM, t_world_cam, **params)
    assert trecs == U.frame_inputs(depth, inst, host, RCAM, **dict(params, max_bg=0, downsample=1, expand=0))[1]
    key = lambda r: (r.status, r.n_mask, r.n_valid, r.n_pts)  # noqa: E731
    assert [key(r) for r in trecs] == [key(r) for r in hrecs] and list(n_rows) == [r.n_pts for r in out["records"]]
    tabs, twin_peeks = vote_over_query(sc, twin.reshape(-1, 3), len(LABELS), params["max_pts"], 3)
    assert twin_peeks == dev
    assert all(np.array_equal(a, out[k]) for a, k in zip(tabs, ("n_in", "n_hit", "n_neg")))
    rule = AO.pick(*tabs, n_rows)
    recs = out["records"]
    assert [(r.status, r.obj, r.second, r.second_hit) for r in recs] == \
           [(r["status"], r["obj"], r["second"], r["second_hit"]) for r in rule]
    assert (recs[0].status, recs[0].obj) == (AO.MATCHED, 0) == (recs[6].status, recs[6].obj)
    assert (recs[1].status, recs[1].obj) == (AO.MATCHED, 1)
    assert recs[2].n_pts == 30 and recs[2].status in (AO.MATCHED, AO.NEW) and recs[2].status == rule[2]["status"]
    assert [recs[k].status for k in (3, 4, 5)] == [AO.NO_POINTS] * 3
    assert [recs[k].ingest_status for k in (3, 4, 5)] == [L.FRAME_SMALL_MASK, L.FRAME_NO_DEPTH, L.FRAME_NO_MASK]
    assert np.all(out["n_in"][:, 2] == 0)                               # nobody is inside the object out of view
    if params is SUB:
        assert recs[0].n_pts == recs[1].n_pts == 65
    else:
        assert recs[0].n_pts == hrecs[0].n_valid > 65 and recs[1].n_pts == hrecs[1].n_valid > 65
    # the point buffer itself, every slot: bitwise utils.assoc_points' strided world points
    got = device_points(sc, lambda: sc.associate_frame(depth, inst, LABELS, RCAM, t_world_cam, **params),
                        len(LABELS) * params["max_pts"])
    assert np.abs(twin[~np.isnan(twin)]).max() < BIG / 2
    assert np.array_equal(bits(got), bits(twin.reshape(-1, 3)))


# ------------------------------------------------------------------ 6. errors leave the handle usable
def test_errors_leave_the_handle_usable(gpu_decoder, dec64, frame):
    from reconstruct import _libdsr as L
    from reconstruct import utils as U
    from reconstruct.optimizer import SceneSdf

    rows = AC.detections(dec64)
    depth, inst, _ = frame
    twc = rigid(9, (1.5, 0.4, -2.0)).astype(np.float32)
    fresh = SceneSdf(gpu_decoder, 4, AC.N_DET * AC.MAX_PTS)
    try:
        with pytest.raises(L.DsrError, match="before dsr_scene_set_objects"):
            fresh.associate_points(rows, max_pts=AC.MAX_PTS)
        with pytest.raises(L.DsrError, match="before dsr_scene_set_objects"):
            fresh.associate_frame(depth, inst, [0, 1], RCAM, twc, **SUB)
        # a map of zero objects is no error
        fresh.set_objects([])
        none = fresh.associate_points(rows, max_pts=AC.MAX_PTS)
        assert none["n_hit"].shape == (AC.N_DET, 0)
        assert [r.status for r in none["records"]] == [AO.NO_POINTS if n == 0 else AO.NEW for n in AC.N_ROWS]
        assert records(none) == AO.pick(*(np.zeros((AC.N_DET, 0), np.int32),) * 3, AC.N_ROWS)
        nf = fresh.associate_frame(depth, inst, [0, 55], RCAM, twc, **SUB)
        assert [(r.status, r.obj, r.second, r.n_pts) for r in nf["records"]] == [(AO.NEW, -1, -1, 65), (AO.NO_POINTS, -1, -1, 0)]
        fresh.set_objects(SO.scene_objects())
        base = fresh.associate_points(rows, max_pts=AC.MAX_PTS)
        assert records(base) == AC.assert_conditions(dec64)
        fbase = fresh.associate_frame(depth, inst, [0, 1, 7], RCAM, twc, **SUB)

        def still_fine():
            assert tables(fresh.associate_points(rows, max_pts=AC.MAX_PTS)) == tables(base)

        shear, nanp, mirror, row = (twc.copy() for _ in range(4))
        shear[0, 1] += 0.01
        nanp[1, 3] = np.nan
        mirror[:3, 0] *= -1.0
        row[3, 3] = 2.0
        bad_points = [lambda: fresh.associate_points([], max_pts=AC.MAX_PTS),                       # n_det < 1
                      lambda: fresh.associate_points(rows, max_pts=AC.MAX_PTS + 1),                 # above the scene's max_pts
                      lambda: fresh.associate_points(rows, max_pts=64),                             # n_rows above max_pts
                      lambda: fresh.associate_points(rows, max_pts=0)]
        bad_points += [lambda t=t: fresh.associate_points(rows, t, max_pts=AC.MAX_PTS) for t in (shear, nanp, mirror, row)]
        bad_points += [lambda kw=kw: fresh.associate_points(rows, max_pts=AC.MAX_PTS, **kw)
                       for kw in (dict(inlier_tol=0.0), dict(inlier_tol=float("nan")), dict(inlier_tol=float("inf")),
                                  dict(min_hits=0), dict(min_pct=-1), dict(min_pct=100))]
        for k, call in enumerate(bad_points):
            with pytest.raises(L.DsrError):
                call()
            still_fine()
        bad_frame = [lambda: fresh.associate_frame(depth, inst, [], RCAM, twc, **SUB),
                     lambda: fresh.associate_frame(depth, inst, list(LABELS), RCAM, twc, **SUB),    # 7 x 65 above 6 x 65
                     lambda: fresh.associate_frame(depth, inst, [0, 1], RCAM, twc, **dict(SUB, max_pts=0)),
                     lambda: fresh.associate_frame(depth, inst, [0, 1], dict(RCAM, fx=0.0), twc, **SUB),
                     lambda: fresh.associate_frame(depth, inst, [0, 1], dict(RCAM, fy=float("nan")), twc, **SUB),
                     lambda: fresh.associate_frame(depth, inst, [0, 1], RCAM, shear, **SUB),
                     lambda: fresh.associate_frame(depth, inst, [0, 1], RCAM, twc, **dict(SUB, min_pct=100))]
        for call in bad_frame:
            with pytest.raises(L.DsrError):
                call()
            still_fine()
        with pytest.raises(ValueError):
            fresh.associate_frame(depth[:-1], inst[:-1], [0], RCAM, twc, **SUB)
        with pytest.raises(TypeError):
            fresh.associate_points(rows, max_pts=AC.MAX_PTS, max_bg=0)
        # raw ctypes: null pointers, an image size, a negative count
        lib = gpu_decoder.ctx.lib
        cam, fp, ap = U.frame_camera(RCAM), U.frame_params(**SUB), U.assoc_params()
        lab = np.asarray([0, 1, 7], np.int32)
        t16 = np.ascontiguousarray(twc.reshape(16))
        outs = (L.AssocOut * 6)()
        good = [fresh._h, cam, fp, ap, L.fptr(t16), L.fptr(depth), L.iptr(inst), 3, L.iptr(lab), outs, None]
        for k in (1, 2, 3, 4, 5, 6, 8, 9):
            args = list(good)
            args[k] = None
            assert lib.dsr_scene_associate_frame(*args) == -2, k
        for w, h in ((0, RH), (RW, 0), (-RW, RH)):
            assert lib.dsr_scene_associate_frame(*(good[:1] + [L.Camera(w, h, 165.0, 165.0, 49.5, 37.0)] + good[2:])) == -2
        assert lib.dsr_scene_associate_frame(*good) == 0
        assert [U.assoc_record(outs[j]) for j in range(3)] == fbase["records"]
        packed = np.zeros((AC.N_DET, AC.MAX_PTS, 3), np.float32)
        for j, r in enumerate(rows):
            packed[j, :r.shape[0]] = r
        n_rows = np.asarray(AC.N_ROWS, np.int32)
        table = np.zeros(3 * AC.N_DET * 4, np.int32)
        good = [fresh._h, ap, None, AC.N_DET, AC.MAX_PTS, L.iptr(n_rows), L.fptr(packed), outs, L.iptr(table)]
        for k in (1, 5, 6, 7):
            args = list(good)
            args[k] = None
            assert lib.dsr_scene_associate_points(*args) == -2, k
        neg = n_rows.copy()
        neg[2] = -1
        assert lib.dsr_scene_associate_points(*(good[:5] + [L.iptr(neg)] + good[6:])) == -2
        assert b"n_rows" in lib.dsr_last_error(gpu_decoder.ctx.handle)
        assert lib.dsr_scene_associate_points(*good) == 0
        assert table.tobytes() == b"".join(base[k].tobytes() for k in ("n_in", "n_hit", "n_neg"))
        still_fine()
        assert tables(fresh.associate_frame(depth, inst, [0, 1, 7], RCAM, twc, **SUB)) == tables(fbase)
    finally:
        fresh.close()
