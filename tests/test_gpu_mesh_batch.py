"""Batched mesh extraction on the GPU (dsr_mesher_run_batch): every mesh of a
batch is bitwise the per-code mesher's, the sign pass saves exact tiles and its audit holds, the
device's tile flags follow the rule restated in tests/test_mesh_batch_cpu.py, and the guard
redoes every code when the lite values are perturbed."""
from __future__ import annotations

import numpy as np
import pytest

import synthetic as S
from conftest import golden, make_cfg
from test_mesh_batch_cpu import MARGIN, mark_tiles, merge

pytestmark = pytest.mark.gpu

SCALES = (0.0, 0.1, 0.3)
TIMES = ("lite_ms", "exact_ms", "mc_ms")


def make_codes(n, code_len=64):
    """zero, 0.1 N(0,1), 0.3 N(0,1), ... with fixed seeds"""
    return [(SCALES[i % 3] * np.random.default_rng(100 + i).standard_normal(code_len)).astype(np.float32)
            for i in range(n)]


_MEX = {}
_REF = {}


def mex_for(dec, d, code_len=64):
    from reconstruct.optimizer import MeshExtractor

    key = (id(dec), d)
    if key not in _MEX:
        _MEX[key] = MeshExtractor(dec, code_len, d)
    return _MEX[key]


def ref_mesh(dec, d, i, level, code_len=64):
    """extract_mesh_from_code of code i, computed once per (decoder, grid, code, level)"""
    key = (id(dec), d, i, level)
    if key not in _REF:
        _REF[key] = mex_for(dec, d, code_len).extract_mesh_from_code(make_codes(i + 1, code_len)[i], level)
    return _REF[key]


def assert_same(meshes, dec, d, level, code_len=64):
    for i, m in enumerate(meshes):
        r = ref_mesh(dec, d, i, level, code_len)
        assert m.vertices.dtype == np.float32 and m.faces.dtype == np.int32
        assert m.vertices.shape == r.vertices.shape and m.faces.shape == r.faces.shape, (i, m.vertices.shape)
        assert m.vertices.tobytes() == r.vertices.tobytes(), i
        assert m.faces.tobytes() == r.faces.tobytes(), i


@pytest.fixture(autouse=True)
def _clean_env(monkeypatch):
    for k in ("DSR_MESH_LITE", "DSR_TEST_HOOKS", "DSR_LITE_PERTURB"):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("level", [0.0, 0.02])
@pytest.mark.parametrize("d,n", [(16, 1), (16, 3), (16, 17), (18, 3), (64, 3)])
def test_batch_meshes_equal_the_per_code_meshes_bitwise(gpu_decoder, d, n, level):
    """17 codes are more than one pass holds; 18^3 = 5832 ends in partial 64- and 128-point tiles;
    64 is the default grid."""
    mex = mex_for(gpu_decoder, d)
    meshes = mex.extract_meshes_from_codes(make_codes(n), level)
    assert len(meshes) == n
    st = mex.stats()
    print("\nd %d codes %d level %g: %s" % (d, n, level, st))
    assert st["n_codes"] == n and st["n_passes"] == (n + 15) // 16 and st["sign_pass"] == 1
    assert any(m.vertices.shape[0] > 0 for m in meshes)
    assert_same(meshes, gpu_decoder, d, level)


def test_sign_pass_saves_exact_tiles_and_the_audit_holds(gpu_decoder):
    mex = mex_for(gpu_decoder, 64)
    meshes = mex.extract_meshes_from_codes(make_codes(3))
    st = mex.stats()
    print("\nstats at 64^3:", st)
    print("decoded-tile share %.4f (audit %.4f), max lite error %.3e"
          % (st["exact_tiles"] / st["all_tiles"], st["audit_tiles"] / st["all_tiles"], st["max_lite_err"]))
    assert_same(meshes, gpu_decoder, 64, 0.0)
    assert st["sign_pass"] == 1 and abs(st["margin"] - MARGIN) < 1e-9
    assert st["all_tiles"] == 3 * 64 ** 3 // 64 and st["lite_tiles"] == 3 * 64 ** 3 // 128
    assert st["violations"] == 0 and st["redone_codes"] == 0 and st["redo_tiles"] == 0
    assert st["lite_broken_blocks"] == 0
    assert 0 < st["exact_tiles"] < st["all_tiles"]
    assert st["audit_tiles"] > 0


@pytest.mark.parametrize("level", [0.0, 0.02])
def test_peek_flags_and_merged_volume(gpu_decoder, level):
    d = 16
    mex = mex_for(gpu_decoder, d)
    codes = make_codes(3)
    mex.extract_meshes_from_codes(codes, level)
    st = mex.stats()
    assert st["redone_codes"] == 0
    n_flagged = 0
    for slot, code in enumerate(codes):
        lite, final, flags = mex.peek(slot)
        assert np.isfinite(lite).all()
        exact = mex.decode_grid(code)
        _, t_need, t_shell = mark_tiles(lite.reshape(d, d, d), level)
        assert np.array_equal(flags == 1, t_need), slot
        assert (flags[t_shell] == 2).all(), slot
        assert np.isin(flags[~t_need], (0, 2)).all(), slot            # (the hashed audit share)
        want = merge(lite, exact, flags != 0)
        assert final.tobytes() == want.tobytes(), slot
        assert np.array_equal(final < np.float32(level), exact < np.float32(level)), slot
        n_flagged += int((flags != 0).sum())
    assert n_flagged == st["exact_tiles"]
    with pytest.raises(Exception):
        mex.peek(3)


def _stats_without_times(st):
    return {k: v for k, v in st.items() if k not in TIMES}


def test_guard_redoes_every_code_under_a_perturbed_lite_pass(gpu_decoder, monkeypatch):
    d = 16
    mex = mex_for(gpu_decoder, d)
    codes = make_codes(3)
    mex.extract_meshes_from_codes(codes)
    clean = mex.stats()
    assert clean["test_hooks"] == 0 and clean["redone_codes"] == 0
    # without DSR_TEST_HOOKS the variable changes nothing
    monkeypatch.setenv("DSR_LITE_PERTURB", "0.05")
    meshes = mex.extract_meshes_from_codes(codes)
    assert _stats_without_times(mex.stats()) == _stats_without_times(clean)
    assert_same(meshes, gpu_decoder, d, 0.0)
    monkeypatch.setenv("DSR_TEST_HOOKS", "1")
    meshes = mex.extract_meshes_from_codes(codes)
    st = mex.stats()
    print("\nperturbed:", st)
    assert st["test_hooks"] == 1 and st["violations"] > 0 and st["redone_codes"] == 3
    assert st["max_lite_err"] > MARGIN / 4
    assert st["exact_tiles"] + st["redo_tiles"] == st["all_tiles"]
    assert_same(meshes, gpu_decoder, d, 0.0)


@pytest.mark.parametrize("level", [-2.0, 2.0])
def test_degenerate_levels_give_empty_meshes(gpu_decoder, level):
    mex = mex_for(gpu_decoder, 16)
    meshes = mex.extract_meshes_from_codes(make_codes(3), level)
    assert len(meshes) == 3
    for m in meshes:
        assert m.vertices.shape == (0, 3) and m.faces.shape == (0, 3)
    one = mex.extract_mesh_from_code(make_codes(1)[0], level)
    assert one.vertices.shape == (0, 3) and one.faces.shape == (0, 3)


def test_empty_batch(gpu_decoder):
    assert mex_for(gpu_decoder, 16).extract_meshes_from_codes([]) == []


def test_capacity_one_vertex_short(gpu_decoder):
    from reconstruct import _libdsr as L

    mex = mex_for(gpu_decoder, 16)
    codes = make_codes(3)
    ref = [ref_mesh(gpu_decoder, 16, i, 0.0) for i in range(3)]
    nv = [r.vertices.shape[0] for r in ref]
    nf = [r.faces.shape[0] for r in ref]
    tv, tf = sum(nv), sum(nf)
    cs = np.ascontiguousarray(np.stack(codes))
    ctx = gpu_decoder.ctx
    for vcap, fcap in ((tv - 1, tf), (tv, tf - 1)):
        verts = np.full((tv, 3), 7.0, np.float32)
        faces = np.full((tf, 3), -7, np.int32)
        voff = np.full(4, -1, np.int32)
        foff = np.full(4, -1, np.int32)
        rc = ctx.lib.dsr_mesher_run_batch(mex._h, 3, L.fptr(cs), 0.0, L.fptr(verts), vcap, L.iptr(faces), fcap,
                                          L.iptr(voff), L.iptr(foff))
        assert rc == -5
        assert voff.tolist() == np.concatenate([[0], np.cumsum(nv)]).tolist()
        assert foff.tolist() == np.concatenate([[0], np.cumsum(nf)]).tolist()
        assert (verts == 7.0).all() and (faces == -7).all()
    verts = np.zeros((tv, 3), np.float32)
    faces = np.zeros((tf, 3), np.int32)
    rc = ctx.lib.dsr_mesher_run_batch(mex._h, 3, L.fptr(cs), 0.0, L.fptr(verts), tv, L.iptr(faces), tf,
                                      L.iptr(voff), L.iptr(foff))
    assert rc == 0                                                    # the exact capacity is enough
    assert verts.tobytes() == b"".join(r.vertices.tobytes() for r in ref)
    # the Python wrapper grows its buffers after a -5 instead of holding the worst case
    small = type(mex)(gpu_decoder, 64, 16)
    small._bverts, small._bfaces = np.zeros((4, 3), np.float32), np.zeros((4, 3), np.int32)
    assert_same(small.extract_meshes_from_codes(codes), gpu_decoder, 16, 0.0)
    assert small._bverts.shape[0] == tv and small._bfaces.shape[0] == tf


def test_mesh_lite_switch_off(gpu_decoder, monkeypatch):
    mex = mex_for(gpu_decoder, 16)
    monkeypatch.setenv("DSR_MESH_LITE", "0")
    meshes = mex.extract_meshes_from_codes(make_codes(17), 0.02)
    st = mex.stats()
    assert st["sign_pass"] == 0 and st["lite_tiles"] == 0 and st["exact_tiles"] == st["all_tiles"]
    assert st["n_passes"] == 2 and st["audit_tiles"] == 0
    assert_same(meshes, gpu_decoder, 16, 0.02)


def test_lite_ineligible_decoder_decodes_every_tile(monkeypatch):
    from deep_sdf.workspace import decoder_from_state

    dec = decoder_from_state(S.fit_last_layer_to_sphere(S.make_decoder_state(1234, hidden_gain=5.0)),
                             S.DEFAULT_SPECS)
    assert not dec.info["lite_eligible"]
    mex = mex_for(dec, 16)
    meshes = mex.extract_meshes_from_codes(make_codes(3))
    st = mex.stats()
    assert st["sign_pass"] == 0 and st["exact_tiles"] == st["all_tiles"]
    assert_same(meshes, dec, 16, 0.0)


def test_code32_decoder():
    from deep_sdf.workspace import decoder_from_state

    specs = dict(S.DEFAULT_SPECS, CodeLength=32)
    dec = decoder_from_state(S.make_decoder(1234, specs), specs)
    mex = mex_for(dec, 16, 32)
    meshes = mex.extract_meshes_from_codes(make_codes(3, 32))
    assert any(m.vertices.shape[0] > 0 for m in meshes)
    assert_same(meshes, dec, 16, 0.0, 32)


def test_keyframe_attaches_the_batch_meshes(gpu_decoder):
    from reconstruct.optimizer import Optimizer

    optim = dict(S.REDWOOD_OPTIM, joint_optim=dict(S.REDWOOD_OPTIM["joint_optim"], num_iterations=3))
    opt = Optimizer(gpu_decoder, make_cfg(optim, "Redwood"))
    obs = [S.redwood_object(40 + i) for i in range(2)]
    dets = [(o.t_cam_obj, o.pts, o.rays, o.depth, None, False) for o in obs]
    f = golden("f6_fail.npz")                                  # a detection that fails (K = 0)
    dets.append((f["obj_t_cam_obj"], f["obj_pts"], f["obj_rays"], f["obj_depth"], f["bigcode"], True))
    mex = mex_for(gpu_decoder, 16)
    plain = opt.reconstruct_keyframe(dets)
    today = opt.reconstruct_keyframe_async(dets).wait()
    assert len(plain) == len(today) == 3
    for a, b in zip(plain, today):
        assert sorted(a.keys()) == sorted(b.keys()) and "vertices" not in a
        for k in a:
            assert np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k], k
    res = opt.reconstruct_keyframe(dets, mesher=mex)
    assert [r["is_good"] for r in res] == [r["is_good"] for r in plain] == [True, True, False]
    for r, p in zip(res, plain):
        if r["is_good"]:
            assert np.array_equal(r["code"], p["code"])
            m = mex.extract_mesh_from_code(r["code"])
            assert r["vertices"].shape[0] > 0
            assert r["vertices"].tobytes() == m.vertices.tobytes() and r["faces"].tobytes() == m.faces.tobytes()
        else:
            assert r["vertices"] is None and r["faces"] is None


def test_map_objects_files_are_byte_identical(gpu_decoder, tmp_path):
    from reconstruct.map_objects import extract_map_objects, write_map_objects

    class OneByOne:                                            # an extractor without the batch call
        def __init__(self, mex):
            self.extract_mesh_from_code = mex.extract_mesh_from_code

    mex = mex_for(gpu_decoder, 16)
    objs = [(3 + 5 * i, np.eye(4, dtype=np.float32), c) for i, c in enumerate(make_codes(3))]
    dirs = []
    for name, ex in (("batch", mex), ("single", OneByOne(mex))):
        p = tmp_path / name
        p.mkdir()
        write_map_objects(str(p / "MapObjects.txt"), objs)
        assert extract_map_objects(str(p), ex) == [3, 8, 13]
        dirs.append(p / "objects")
    for oid in (3, 8, 13):
        for ext in ("npy", "ply"):
            assert (dirs[0] / f"{oid}.{ext}").read_bytes() == (dirs[1] / f"{oid}.{ext}").read_bytes()
