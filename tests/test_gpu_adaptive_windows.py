"""Per-object render-pass windows (choose_windows): every object re-chooses its
in-ball-rank windows each iteration from where its rays terminated in the one before.  The
windows decide only which samples BEHIND a ray's first certainly-full one are decoded, so every
result must be bitwise what the fixed windows give, while fewer samples are decoded.

The objects here are small (456 rays, M = 50), far below the sample count at which a batch gets
the seven-pass default schedule, so the tests name that schedule (DSR_RENDER_PASSES) and switch
the windows with DSR_ADAPTIVE_WINDOWS beside it; both are test hooks."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import synthetic as S
from conftest import make_cfg

pytestmark = pytest.mark.gpu

SCHEDULE = "8,12,16,20,24,32"       # the large-batch default (render_passes, dsr_api.hip)
BOUNDS = [0, 8, 12, 16, 20, 24, 32, 50]
ITERS = 10


def _opt(dec, optim=S.KITTI_OPTIM, data_type="KITTI", iters=ITERS):
    from reconstruct.optimizer import Optimizer

    if iters is not None:
        optim = dict(optim, joint_optim=dict(optim["joint_optim"], num_iterations=iters))
    return Optimizer(dec, make_cfg(optim, data_type))


def _objects(n, seed0=40):
    return [(o.t_cam_obj, o.pts, o.rays, o.depth, None)
            for o in (S.kitti_object(seed0 + i, n_pts=256) for i in range(n))]


def _windows(monkeypatch, on, streams=None):
    monkeypatch.setenv("DSR_TEST_HOOKS", "1")
    monkeypatch.setenv("DSR_RENDER_PASSES", SCHEDULE)
    monkeypatch.setenv("DSR_ADAPTIVE_WINDOWS", "1" if on else "0")
    if streams is None:
        monkeypatch.delenv("DSR_STREAMS", raising=False)
    else:
        monkeypatch.setenv("DSR_STREAMS", streams)


def _assert_same_results(a, b, what):
    """Records and per-iteration traces of two runs, bitwise (decoded counts apart)."""
    (ra, ta), (rb, tb) = a, b
    assert len(ra) == len(rb)
    for i in range(len(ra)):
        x, y = ra[i], rb[i]
        assert x["is_good"] == y["is_good"] and x["iters_done"] == y["iters_done"], (what, i)
        assert x["fail_reason"] == y["fail_reason"], (what, i)
        assert np.float32(x["loss"]).tobytes() == np.float32(y["loss"]).tobytes(), (what, i)
        if x["is_good"]:
            assert x["t_cam_obj"].tobytes() == y["t_cam_obj"].tobytes(), (what, i)
            assert x["code"].tobytes() == y["code"].tobytes(), (what, i)
        for key in ("H", "b", "k", "n_valid", "n_refined", "loss"):
            assert ta[i][key].tobytes() == tb[i][key].tobytes(), (what, i, key)


@pytest.fixture(scope="module")
def runs(gpu_decoder):
    """The 4-object batch in two object groups (k_sample_pass) and a one-object batch (the chunked
    k_sample_scan / _count / _emit), each with the windows off, on, and on again."""
    mp = pytest.MonkeyPatch()
    out = {}
    try:
        opt = _opt(gpu_decoder)
        for name, objs, streams in (("multi", _objects(4), "2"), ("chunked", _objects(1, 44), None)):
            for tag, on in (("off", False), ("on", True), ("on2", True)):
                _windows(mp, on, streams)
                out[name, tag] = opt.reconstruct_objects(objs, trace=True)
    finally:
        mp.undo()
    return out


@pytest.mark.parametrize("path", ["multi", "chunked"])
def test_results_are_bitwise_those_of_the_fixed_windows(runs, path):
    _assert_same_results(runs[path, "on"], runs[path, "off"], path)
    assert all(r["is_good"] and r["iters_done"] == ITERS for r in runs[path, "on"][0])


@pytest.mark.parametrize("path", ["multi", "chunked"])
def test_fewer_samples_are_decoded(runs, path):
    on = np.array([t["n_decoded"] for t in runs[path, "on"][1]], np.int64)      # [object][iteration]
    off = np.array([t["n_decoded"] for t in runs[path, "off"][1]], np.int64)
    print(path, "decoded on", on.tolist(), "off", off.tolist())
    assert off.min() > 0
    assert (on <= off).all(), (on - off).tolist()
    assert on[:, 2:].sum() < off[:, 2:].sum()
    # iteration 0 has no history: the fixed windows themselves
    assert np.array_equal(on[:, 0], off[:, 0])


@pytest.mark.parametrize("path", ["multi", "chunked"])
def test_decoded_counts_repeat_run_to_run(runs, path):
    for a, b in zip(runs[path, "on"][1], runs[path, "on2"][1]):
        assert np.array_equal(a["n_decoded"], b["n_decoded"])
    _assert_same_results(runs[path, "on"], runs[path, "on2"], path)


def test_ragged_ray_counts_and_a_rayless_object(gpu_decoder, monkeypatch):
    """Ray counts across the 128-ray chunks (130, 456, 712) and an object without rays, in one
    group (chunked passes) and in two: the windows change no bit."""
    opt = _opt(gpu_decoder, iters=4)
    objs = []
    for i, nr in enumerate((130, 456, 712, 0)):
        o = S.kitti_object(60 + i, n_pts=512)
        rays = np.ascontiguousarray(o.rays[:nr])
        objs.append((o.t_cam_obj, o.pts, rays, np.ascontiguousarray(o.depth[:min(nr, o.depth.shape[0])]), None))
    for streams in ("1", "2"):
        res = {}
        for on in (False, True):
            _windows(monkeypatch, on, streams)
            res[on] = opt.reconstruct_objects(objs, trace=True)
        _assert_same_results(res[True], res[False], streams)
        assert not res[True][0][3]["is_good"] and res[True][0][3]["fail_reason"].startswith("fewer than 10")
        assert res[True][0][1]["is_good"]
        for a, b in zip(res[True][1][:3], res[False][1][:3]):
            assert (a["n_decoded"] <= b["n_decoded"]).all(), (streams, a["n_decoded"], b["n_decoded"])


def test_window_tables_and_the_switch_are_reported(gpu_decoder, monkeypatch):
    """dsr_batch_windows: the switch as the batch runs it and every object's table after the run
    (0 < first boundary >= the fixed first window, strictly increasing, last = M); an explicit
    DSR_RENDER_PASSES alone keeps its fixed windows, and so does a one-pass batch."""
    import bench
    from reconstruct import _libdsr as L

    params = L.optim_params(dict(S.KITTI_OPTIM, joint_optim=dict(S.KITTI_OPTIM["joint_optim"], num_iterations=3)))
    lib, ctx = gpu_decoder.ctx.lib, gpu_decoder.ctx

    def run(n_obj=3):
        h, keep = bench.make_batch(gpu_decoder, params, n_obj, 70, n_pts=256)
        try:
            ctx.check(lib.dsr_batch_run(h), "run")
            ad, nb = C.c_int(-1), C.c_int(-1)
            tab = (C.c_int * (n_obj * 64))()
            ctx.check(lib.dsr_batch_windows(h, C.byref(ad), C.byref(nb), tab), "windows")
            return ad.value, np.array(tab[:n_obj * nb.value]).reshape(n_obj, nb.value)
        finally:
            lib.dsr_batch_destroy(h)

    _windows(monkeypatch, True)
    ad, tab = run()
    assert ad == 1 and tab.shape == (3, len(BOUNDS))
    assert (tab[:, 0] == 0).all() and (tab[:, -1] == 50).all() and (tab[:, 1] >= BOUNDS[1]).all()
    assert (np.diff(tab, axis=1) > 0).all(), tab
    assert (tab != np.array(BOUNDS)).any(), tab            # (the objects did move their windows)
    _windows(monkeypatch, False)
    ad, tab = run()
    assert ad == 0 and (tab == np.array(BOUNDS)).all()
    monkeypatch.delenv("DSR_ADAPTIVE_WINDOWS")             # an explicit schedule alone: fixed
    ad, tab = run()
    assert ad == 0 and (tab == np.array(BOUNDS)).all()
    monkeypatch.delenv("DSR_RENDER_PASSES")                # this small batch's default: one pass
    ad, tab = run()
    assert ad == 0 and tab.tolist() == [[0, 50]] * 3


def _keyframes(n_kf, dets=4, seed0=800):
    kfs = []
    for k in range(n_kf):
        d = []
        for i in range(dets - (k % 2)):
            o = S.redwood_object(seed0 + 10 * k + i, n_pts=384 + 32 * ((k + i) % 5))
            d.append((o.t_cam_obj, o.pts, o.rays, o.depth, None, False))
        kfs.append(d)
    return kfs


def test_keyframe_graph_replays_with_adaptive_windows(gpu_decoder, monkeypatch):
    """A capacity batch replayed as a graph: the windows live in device state the graph's own
    kernels reset and update, so six ragged keyframes need one capture and give the records of
    the one-shot path — with the windows on and with them off."""
    from reconstruct import _libdsr as L

    kfs = _keyframes(6)
    res = {}
    for mode, on in (("oneshot", False), ("oneshot", True), ("graph", True)):
        _windows(monkeypatch, on)
        opt = _opt(gpu_decoder, S.REDWOOD_OPTIM, "Redwood", iters=None)
        opt.keyframe_mode = mode
        res[mode, on] = [opt.reconstruct_keyframe(d) for d in kfs]
        if mode == "graph":
            assert len(opt._slots) == 1
            st = L.Stats()
            opt._ctx.check(opt._ctx.lib.dsr_batch_stats(opt._slots[0].handle, C.byref(st)), "stats")
            assert st.graph_captures == 1 and st.graph_replays == 6, (st.graph_captures, st.graph_replays)
            ad, nb = C.c_int(-1), C.c_int(-1)
            opt._ctx.check(opt._ctx.lib.dsr_batch_windows(opt._slots[0].handle, C.byref(ad), C.byref(nb), None), "win")
            assert ad.value == 1 and nb.value > 2
            opt.close_slots()
    for k in range(len(kfs)):
        for other in (("oneshot", True), ("oneshot", False)):
            a, b = res["graph", True][k], res[other][k]
            assert len(a) == len(b)
            for x, y in zip(a, b):
                assert x["is_good"] == y["is_good"] and np.float32(x["loss"]) == np.float32(y["loss"])
                if x["is_good"]:
                    assert np.array_equal(x["t_cam_obj"], y["t_cam_obj"]) and np.array_equal(x["code"], y["code"])
