"""Host-side logic of the drop-in package on CPU (no GPU, no compute calls).

* the entry path the C++ side takes first (System.cc:95-98): ``get_configs`` on a
  config JSON with the reference's keys, then ``config_decoder``'s file handling
  (specs.json + ModelParameters/latest.pth, weights_only) — the device upload itself
  is covered by tests/test_gpu_api.py::test_entry_path_as_the_cpp_side_calls_it;
* argument validation before anything reaches C (a short code would be an
  out-of-bounds read there: the ABI copies code_len floats);
* the ingest hook runs the reference's own data-ingest modules (and resolves nothing else);
* golden F9 (tests/golden/make_mesher.py): the reference's voxel grid and its vertex
  transform around marching cubes.
"""
from __future__ import annotations

import json
import os
import sys

import numpy as np
import pytest

import synthetic as S
from conftest import golden


def _reference_style_config(tmp_path, deepsdf_dir, data_type="Redwood"):
    """A config with the keys configs/config_redwood_01053.json carries (written here)."""
    cfg = {"data_type": data_type, "detect_online": False, "DeepSDF_DIR": str(deepsdf_dir),
           "voxels_dim": 32, "min_bb_area": 1600, "min_mask_area": 1000, "downsample_ratio": 4.0,
           "optimizer": S.REDWOOD_OPTIM, "viewer": {"distance": 10, "tilt": 30, "frame_size": 0.5}}
    p = tmp_path / "config.json"
    p.write_text(json.dumps(cfg))
    return str(p)


def test_get_configs_and_checkpoint_files(tmp_path, full_state, full_layers):
    from deep_sdf.workspace import fold_state, load_specs, model_params_subdir
    from reconstruct.utils import get_configs

    exp = S.write_experiment_dir(str(tmp_path / "deepsdf"), full_state)
    cfg = get_configs(_reference_style_config(tmp_path, exp))
    assert cfg.optimizer.code_len == 64 and cfg.voxels_dim == 32
    assert cfg.optimizer.joint_optim.k3 == S.REDWOOD_OPTIM["joint_optim"]["k3"]
    with pytest.raises(KeyError):
        cfg.no_such_key                      # ForceKeyErrorDict (utils.py:82-84)
    specs = load_specs(cfg.DeepSDF_DIR)
    assert specs["CodeLength"] == 64
    import torch

    saved = torch.load(os.path.join(exp, model_params_subdir, "latest.pth"), map_location="cpu",
                       weights_only=True)
    layers = fold_state(saved["model_state_dict"], specs)
    for (W, b), (W0, b0) in zip(layers, full_layers):
        assert np.array_equal(W, W0) and np.array_equal(b, b0)


class _FakeDecoder:
    code_len = 64
    ctx = None
    handle = None


def test_short_code_is_rejected_before_c():
    from reconstruct.optimizer import MeshExtractor, Optimizer, sdf_eval
    from reconstruct.utils import ForceKeyErrorDict

    opt = Optimizer(_FakeDecoder(), ForceKeyErrorDict(data_type="KITTI", optimizer=S.KITTI_OPTIM))
    ob = S.redwood_object(0, n_pts=16)
    short = np.zeros(10, np.float32)
    with pytest.raises(ValueError):
        opt.reconstruct_objects([(ob.t_cam_obj, ob.pts, ob.rays, ob.depth, short)])
    with pytest.raises(ValueError):
        opt.estimate_pose_cam_obj(ob.t_cam_obj, 1.0, ob.pts, short)
    with pytest.raises(ValueError):
        opt.estimate_pose_cam_obj_batch([(ob.t_cam_obj, 1.0, ob.pts, short)])
    with pytest.raises(ValueError):
        opt.compute_sdf_loss_objectpoint_zhjd(ob.pts, short)
    with pytest.raises(ValueError):
        sdf_eval(_FakeDecoder(), short, ob.pts)
    mex = MeshExtractor.__new__(MeshExtractor)          # no device grid upload
    mex.decoder, mex.code_len = _FakeDecoder(), 64
    with pytest.raises(ValueError):
        mex.extract_mesh_from_code(short)


# Stand-ins for the ingest modules a DSP-SLAM checkout provides (written for this test, held in no
# other tree): they take from this package exactly the names the originals take (see the test's
# docstring) and construct the two sequence classes get_sequence dispatches to.
_STANDIN_HEAD = """\
import os
import numpy as np
import cv2
from reconstruct.loss_utils import get_rays, get_time
from reconstruct.utils import ForceKeyErrorDict, read_calib_file, load_velo_scan
from reconstruct import get_detectors
"""
_STANDIN_INGEST = {
    "kitti_sequence": _STANDIN_HEAD + """

class KITIISequence:
    def __init__(self, data_dir, configs):
        self.configs = configs
        self.num_frames = len(os.listdir(os.path.join(data_dir, "image_2")))
        calib = read_calib_file(os.path.join(data_dir, "calib.txt"))
        proj = calib["P2"].reshape(3, 4)
        self.K_cam = proj[:, :3].astype(np.float32)
        self.invK_cam = np.linalg.inv(self.K_cam).astype(np.float32)
        cam2_from_cam0 = np.eye(4)
        cam2_from_cam0[0, 3] = proj[0, 3] / proj[0, 0]
        cam0_from_velo = np.vstack([calib["Tr"].reshape(3, 4), [0.0, 0.0, 0.0, 1.0]])
        self.T_cam_velo = (cam2_from_cam0 @ cam0_from_velo).astype(np.float32)
        self.detector_2d, self.detector_3d = get_detectors(configs)
""",
    "mono_sequence": _STANDIN_HEAD + """

class MonoSequence:
    def __init__(self, data_dir, configs):
        self.configs = configs
        fs = cv2.FileStorage(configs.slam_config_path, cv2.FILE_STORAGE_READ)
        fx, fy, cx, cy, self.k1, self.k2 = (fs.getNode("Camera." + k).real()
                                            for k in ("fx", "fy", "cx", "cy", "k1", "k2"))
        self.K_cam = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
        self.invK_cam = np.linalg.inv(self.K_cam)
        self.detector_2d = get_detectors(configs)
""",
    # present in the directory, never loaded: only the four named ingest modules resolve there
    "loss": "raise RuntimeError('reconstruct.loss must never resolve outside the package')\n",
}


@pytest.fixture
def ingest_dir(tmp_path):
    """The directory ``DSR_REFERENCE_RECONSTRUCT`` names: the caller's own (a DSP-SLAM checkout's
    ``reconstruct/``) when the variable is set and provides the modules, else the stand-ins."""
    own = os.environ.get("DSR_REFERENCE_RECONSTRUCT", "")
    if own and all(os.path.isfile(os.path.join(own, n + ".py")) for n in ("kitti_sequence", "mono_sequence")):
        return own
    d = tmp_path / "ingest"
    d.mkdir()
    for name, text in _STANDIN_INGEST.items():
        (d / (name + ".py")).write_text(text)
    return str(d)


class _CV2Stub:
    """cv2 is absent here; the reference's ingest modules need it only inside frames
    (imread, undistortPoints) and for MonoSequence's intrinsics (FileStorage)."""

    FILE_STORAGE_READ = 0

    class FileStorage:
        VALUES = {"Camera.fx": 525.0, "Camera.fy": 520.0, "Camera.cx": 319.5, "Camera.cy": 239.5,
                  "Camera.k1": 0.01, "Camera.k2": -0.02}

        def __init__(self, path, mode):
            self.path = path

        def getNode(self, key):
            v = self.VALUES[key]
            return type("Node", (), {"real": lambda self: v})()


def test_ingest_hook_runs_the_reference_modules(tmp_path, monkeypatch, ingest_dir):
    """System.cc:99 calls reconstruct.get_sequence at every start-up.  Through the ingest hook
    the build loads kitti_sequence.py / mono_sequence.py from the directory
    DSR_REFERENCE_RECONSTRUCT names (the reference's own when the caller's environment points
    there, else stand-ins with the same imports), which import
    get_rays / get_time from reconstruct.loss_utils and read_calib_file / load_velo_scan /
    ForceKeyErrorDict from reconstruct.utils (kitti_sequence.py:22-24, mono_sequence.py:22-24):
    both sequences construct, calibration parsed by this package's reader.  Nothing else
    resolves to the reference: reconstruct.loss stays an ImportError although the directory
    holds loss.py."""
    import types

    import reconstruct
    from reconstruct.loss_utils import get_rays
    from reconstruct.utils import ForceKeyErrorDict, load_velo_scan, read_calib_file

    cv2 = types.ModuleType("cv2")
    for k, v in vars(_CV2Stub).items():
        if not k.startswith("__"):
            setattr(cv2, k, v)
    monkeypatch.setitem(sys.modules, "cv2", cv2)
    monkeypatch.setenv("DSR_REFERENCE_RECONSTRUCT", ingest_dir)
    assert os.path.isfile(os.path.join(ingest_dir, "loss.py"))
    for name in ("kitti_sequence", "mono_sequence"):
        monkeypatch.delitem(sys.modules, "reconstruct." + name, raising=False)
    # a KITTI sequence directory: calib.txt (P2 with a baseline term, Tr), two images, a scan
    d = tmp_path / "seq"
    (d / "image_2").mkdir(parents=True)
    for k in range(2):
        (d / "image_2" / f"{k:06d}.png").write_bytes(b"")
    P2 = [721.5, 0, 609.6, 44.9, 0, 721.5, 172.9, 0.2, 0, 0, 1, 0.003]
    Tr = [0.0, -1, 0, 0.01, 0, 0, -1, -0.07, 1, 0, 0, -0.27]
    (d / "calib.txt").write_text("P0: " + " ".join(map(str, P2)) + "\nP2: " + " ".join(map(str, P2))
                                 + "\nTr: " + " ".join(map(str, Tr)) + "\ndate: 2011-09-26\n\nP3: 1 2\n")
    cal = read_calib_file(str(d / "calib.txt"))
    assert set(cal) == {"P0", "P2", "Tr"} and cal["P2"].dtype == np.float64
    cfg = ForceKeyErrorDict(data_type="KITTI", detect_online=False, path_label_2d=str(tmp_path / "l2"),
                            path_label_3d=str(tmp_path / "l3"))
    seq = reconstruct.get_sequence(str(d), cfg)
    assert type(seq).__name__ == "KITIISequence" and seq.num_frames == 2
    K = np.array(P2, np.float64).reshape(3, 4)[:, :3]
    assert np.allclose(seq.K_cam, K) and np.allclose(seq.invK_cam, np.linalg.inv(K), rtol=1e-6)
    assert np.isclose(seq.T_cam_velo[0, 3], Tr[3] + P2[3] / P2[0], rtol=1e-6)
    assert seq.detector_2d is None and seq.detector_3d is None
    # the rays the reference's frames build with this package's get_rays (kitti_sequence.py:209)
    px = np.array([[100.0, 50.0], [600.5, 180.25]])
    rays = get_rays(px, seq.invK_cam)
    assert rays.dtype == np.float32
    assert np.allclose(rays, (np.c_[px, np.ones(2)] @ seq.invK_cam.T), rtol=1e-6)
    scan = np.arange(12, dtype=np.float32)
    scan.tofile(str(d / "scan.bin"))
    assert np.array_equal(load_velo_scan(str(d / "scan.bin")), scan.reshape(3, 4))
    # a Redwood (mono) sequence: intrinsics through cv2.FileStorage
    mcfg = ForceKeyErrorDict(data_type="Redwood", detect_online=False, slam_config_path="x.yaml",
                             path_label_2d=str(tmp_path / "l2"))
    mono = reconstruct.get_sequence(str(tmp_path), mcfg)
    assert type(mono).__name__ == "MonoSequence" and mono.K_cam[0, 0] == 525.0 and mono.k2 == -0.02
    with pytest.raises(ImportError):
        import reconstruct.loss  # noqa: F401
    assert reconstruct.get_detectors(ForceKeyErrorDict(detect_online=False, data_type="KITTI")) == (None, None)
    for name in ("kitti_sequence", "mono_sequence"):
        monkeypatch.delitem(sys.modules, "reconstruct." + name, raising=False)


# the package-level imports of the reference's own scripts (the names they take from
# ``reconstruct``): reconstruct_frame.py:20-23, visualize_map.py:22, extract_map_objects.py:21-22,
# and the C++ side's embedded imports (System.cc:93-99, LocalMapping.cc:38-40)
SCRIPT_IMPORTS = {
    "reconstruct.utils": ("color_table", "set_view", "get_configs", "get_decoder", "write_mesh_to_ply",
                          "ForceKeyErrorDict", "create_voxel_grid", "convert_sdf_voxels_to_mesh",
                          "read_calib_file", "load_velo_scan"),
    "reconstruct.loss_utils": ("get_time", "get_rays"),
    "reconstruct.optimizer": ("Optimizer", "MeshExtractor"),
    "reconstruct": ("get_sequence", "get_detectors"),
}


@pytest.mark.parametrize("module", sorted(SCRIPT_IMPORTS))
def test_reference_script_imports_resolve(module):
    """Every name the reference's scripts and its C++ side import from ``reconstruct`` exists
    in the build's package (so reconstruct_frame.py / visualize_map.py / extract_map_objects.py
    get past their imports with dsp-slam-rgbd_amd/ first on sys.path)."""
    import importlib

    mod = importlib.import_module(module)
    missing = [n for n in SCRIPT_IMPORTS[module] if not hasattr(mod, n)]
    assert not missing, (module, missing)


def test_voxel_grid_matches_reference_f9():
    from reconstruct.utils import create_voxel_grid

    f = golden("f9_mesher.npz")
    g = create_voxel_grid(vol_dim=int(f["dim"]))
    assert g.dtype == np.float32 and np.array_equal(g, f["grid"])


def test_vertex_transform_matches_reference_f9():
    from oracle.dsr_mc import vertex_transform

    f = golden("f9_mesher.npz")
    assert str(f["verts_dtype"]) == "float32"
    assert np.array_equal(vertex_transform(f["verts_index"], int(f["dim"])), f["verts_out"])
    assert np.allclose(f["spacing"], 2.0 / (int(f["dim"]) - 1)) and float(f["level"]) == 0.0


def test_viewer_helpers_match_reference_f11():
    """color_table / set_view (utils.py:26-55), imported by the reference's scripts
    (reconstruct_frame.py:20, visualize_map.py:22): the palette and the extrinsic set_view
    installs, against golden F11 (tests/golden/make_utils.py, recorded from the reference)."""
    import types

    from reconstruct.utils import color_table, set_view

    f = golden("f11_utils.npz")
    assert np.array_equal(np.asarray(color_table, np.float64), f["color_table"])

    class Vis:
        installed = None

        def get_view_control(self):
            vis = self

            class Ctl:
                def convert_to_pinhole_camera_parameters(self):
                    return types.SimpleNamespace(extrinsic=np.zeros((4, 4)))

                def convert_from_pinhole_camera_parameters(self, cam):
                    vis.installed = np.array(cam.extrinsic, np.float64)
            return Ctl()

    for (dist, theta), ext in zip(f["views"], f["extrinsics"][:-1]):
        v = Vis()
        set_view(v, dist=float(dist), theta=float(theta))
        assert np.array_equal(v.installed, ext)
    v = Vis()
    set_view(v)
    assert np.array_equal(v.installed, f["extrinsics"][-1])


def test_grid_decode_order_matches_reference_f9(oracle_dec):
    """The reference decodes create_voxel_grid's points and views them as (d, d, d)
    (optimizer.py:225-227): the oracle's decode in the same order reproduces the volume."""
    from oracle import dsr_oracle as O
    from reconstruct.utils import create_voxel_grid

    f = golden("f9_mesher.npz")
    d = int(f["dim"])
    vol = O.decode_sdf(oracle_dec, f["code"], create_voxel_grid(vol_dim=d)).reshape(d, d, d)
    assert np.abs(vol - f["volume"]).max() <= 2e-5


@pytest.mark.parametrize("change,what", [
    ({"xyz_in_all": True}, "shapes"),          # implemented, but these are 8x512 lin shapes
    ({"dims": [512] * 6}, "dims"),
    ({"latent_in": [3]}, "latent_in"),
])
def test_unsupported_decoder_variants_rejected_loudly(change, what):
    """decoder shapes libdsr does not implement (other dims / latent_in /
    CodeLength) are refused before anything reaches the device, never approximated; the
    implemented variants (deep_sdf_decoder.py:41-67, 89-102) pass."""
    import copy

    import synthetic as S
    from deep_sdf.workspace import check_topology, fold_state

    layers = fold_state(S.make_decoder(1234), S.DEFAULT_SPECS)
    check_topology(S.DEFAULT_SPECS, layers)                  # the supported topology passes
    specs = copy.deepcopy(S.DEFAULT_SPECS)
    specs["NetworkSpecs"].update(change)
    with pytest.raises(NotImplementedError, match=what):
        check_topology(specs, layers)
    specs = copy.deepcopy(S.DEFAULT_SPECS)
    specs["CodeLength"] = 48
    with pytest.raises(NotImplementedError, match="CodeLength"):
        check_topology(specs, layers)
    # implemented variants: use_tanh, dropout / latent_dropout (inert in eval), plain Linear layers
    for change in ({"use_tanh": True}, {"latent_dropout": True}, {"weight_norm": False, "norm_layers": []},
                   {"weight_norm": False}):     # the last: LayerNorm after lin0..lin7
        ok = copy.deepcopy(S.DEFAULT_SPECS)
        ok["NetworkSpecs"].update(change)
        check_topology(ok, layers)
    # xyz_in_all, with its own layer shapes (509 outputs on every hidden layer but lin3)
    xa = copy.deepcopy(S.DEFAULT_SPECS)
    xa["NetworkSpecs"]["xyz_in_all"] = True
    check_topology(xa, fold_state(S.make_decoder(1234, xa), xa))
    # CodeLength 32 is supported (LocalMapping_util.cc:416-422), with its own layer shapes
    specs["CodeLength"] = 32
    with pytest.raises(NotImplementedError, match="shapes"):
        check_topology(specs, layers)
    check_topology(specs, fold_state(S.make_decoder(1234, specs), specs))


def test_keyframe_slot_capacity_is_bounded(monkeypatch):
    """a keyframe slot batch is laid out for max_obj x max_rays x M ray samples
    whatever the fill.  A slot serves a keyframe only within SLOT_WASTE x the keyframe's own ray
    count, grows only inside that bound, and never beyond SLOT_MAX_SAMPLES — otherwise the
    keyframe runs one-shot (``_slot_for`` returns None).  SlotBatch is stubbed: no device here."""
    from reconstruct import optimizer as O
    from conftest import make_cfg

    made = []

    class Stub:
        def __init__(self, opt, max_obj, max_pts, max_rays, graph):
            self.max_obj, self.max_pts, self.max_rays, self.graph = max_obj, max_pts, max_rays, graph
            self.busy = False
            self.closed = False
            made.append(self)

        def fits(self, n, p, r):
            return n <= self.max_obj and p <= self.max_pts and r <= self.max_rays

        def close(self):
            self.closed = True

    monkeypatch.setattr(O, "SlotBatch", Stub)
    monkeypatch.setattr(O.Optimizer, "SLOT_MIN_RAYS", 256)
    opt = O.Optimizer(None, make_cfg(S.REDWOOD_OPTIM, "Redwood"))
    assert opt.keyframe_mode == "graph"

    def kf(n, n_pts, n_rays):
        return [(np.eye(4), np.zeros((n_pts, 3)), np.zeros((n_rays, 3)), np.zeros(0)) for _ in range(n)]

    many_small = opt._slot_for(kf(8, 256, 300))        # 8 x 384 rays padded
    assert (many_small.max_obj, many_small.max_rays) == (8, 384)
    # one large object: growing the 8-object slot to 8 x 4096 rays would be 8x its need -> a new
    # slot sized for it, BESIDE the free one (a keyframe that cannot grow a free slot
    # within the bounds no longer destroys it and its captured graph)
    big = opt._slot_for(kf(1, 2048, 4000))
    assert (big.max_obj, big.max_rays) == (1, 4096) and not many_small.closed
    # a small keyframe inside the large slot's bound is served by it
    assert opt._slot_for(kf(1, 100, 1500)) is big
    # a keyframe far smaller than every free slot does not use them: a slot of its own
    tiny = opt._slot_for(kf(1, 64, 100))
    assert tiny is not big and (tiny.max_obj, tiny.max_rays) == (1, 128)
    assert not big.closed and not many_small.closed and len(opt._slots) == 3
    # the 8-object keyframe shape comes back: its slot (and graph) is still there
    assert opt._slot_for(kf(8, 200, 300)) is many_small
    # a fourth slot (the others in flight, so none can grow)
    for sl in opt._slots:
        sl.busy = True
    fourth = opt._slot_for(kf(2, 1024, 1024))
    for sl in opt._slots:
        sl.busy = False
    assert len(opt._slots) == 4 and not any(sl.closed for sl in (many_small, big, tiny, fourth))
    assert opt._slot_for(kf(1, 100, 1500)) is big
    # MAX_SLOTS reached and no free slot can serve or grow: the least recently used free slot
    # (many_small; tiny is in flight) makes room, the others stay
    tiny.busy = True
    fifth = opt._slot_for(kf(1, 64, 60))
    assert many_small.closed and not any(sl.closed for sl in (big, tiny, fourth))
    assert len(opt._slots) == 4 and fifth in opt._slots and (fifth.max_obj, fifth.max_rays) == (1, 128)
    tiny.busy = False
    # beyond SLOT_MAX_SAMPLES ray samples: one-shot
    monkeypatch.setattr(O.Optimizer, "SLOT_MAX_SAMPLES", 1 << 16)
    for sl in opt._slots:
        sl.busy = True
    assert opt._slot_for(kf(4, 1024, 2048)) is None
    # every slot busy and MAX_SLOTS reached: one-shot
    monkeypatch.setattr(O.Optimizer, "SLOT_MAX_SAMPLES", 1 << 24)
    while len(opt._slots) < opt.MAX_SLOTS:
        opt._slots.append(Stub(opt, 1, 128, 128, True))
        opt._slots[-1].busy = True
    assert opt._slot_for(kf(1, 64, 100)) is None
