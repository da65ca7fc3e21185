"""Batched mesh extraction (dsr_mesher_run_batch) without a GPU: the ABI-12 entry
points, the stats struct's layout, the argument checks, and the sign-pass rule itself — restated
here in numpy (``mark_tiles``; tests/test_gpu_mesh_batch.py holds the device's flags to it) — on
an analytic volume: a lite volume within margin / 4 of the exact one, merged with the exact
values of the marked 64-point tiles, gives marching cubes the same mesh bit for bit."""
from __future__ import annotations

import ctypes
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from conftest import REPO

HDR = os.path.join(REPO, "include", "dsr.h")
NEW = ("dsr_mesher_run_batch", "dsr_mesher_stats_get", "dsr_mesher_peek")
MARGIN = 0.01
TILE = 64


def in_band(y, refine, level, m=MARGIN):
    """B: not finite, |y - level| < m (in fp32, as the device computes it), or flagged."""
    y = np.asarray(y, np.float32)
    with np.errstate(invalid="ignore"):
        far = np.abs(y - np.float32(level)) >= np.float32(m)
    return ~np.isfinite(y) | ~far | (np.asarray(refine) != 0)


def mark_tiles(lite, level, m=MARGIN, refine=None):
    """Rule (b) of the sign pass on a (d, d, d) lite volume.  Returns (needed voxels (d, d, d)
    bool, needed 64-point tiles bool, shell-audit tiles bool): a voxel needs an exact value if it
    or one of its 6 neighbours is in B, or a neighbour outside B lies on the other side of the
    level; a tile is needed if it holds such a voxel, and audited if it is not needed and holds a
    voxel with m <= |y - level| < 2m."""
    lite = np.asarray(lite, np.float32)
    d = lite.shape[0]
    refine = np.zeros(lite.shape, np.uint8) if refine is None else np.asarray(refine).reshape(lite.shape)
    b = in_band(lite, refine, level, m)
    inside = lite < np.float32(level)
    need = b.copy()
    for ax in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, d - 1), slice(1, d)
        lo, hi = tuple(lo), tuple(hi)
        pair = b[lo] | b[hi] | (inside[lo] != inside[hi])
        need[lo] |= pair
        need[hi] |= pair
    with np.errstate(invalid="ignore"):
        shell = ~b & (np.abs(lite - np.float32(level)) < np.float32(2.0) * np.float32(m))
    n = d ** 3
    nt = (n + TILE - 1) // TILE
    pad = nt * TILE - n
    tiles = lambda v: np.concatenate([v.reshape(-1), np.zeros(pad, bool)]).reshape(nt, TILE).any(axis=1)  # noqa: E731
    t_need = tiles(need)
    return need, t_need, tiles(shell) & ~t_need


def merge(lite, exact, decoded_tiles):
    """Final volume: exact where the voxel's tile was decoded, lite elsewhere."""
    n = lite.size
    dec = np.repeat(decoded_tiles, TILE)[:n].reshape(lite.shape)
    return np.where(dec, exact, lite).astype(np.float32)


def _declared():
    txt = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    return set(re.findall(r"^\s*(?:const\s+)?\w+\*?\s+\**(dsr_\w+)\s*\(", txt, flags=re.M))


def test_header_declares_and_library_exports_the_batch_entry_points():
    from reconstruct import _libdsr as L

    assert set(NEW) <= _declared()
    assert set(NEW) <= set(L.SIGNATURES)
    lib = L.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", L.lib_path()], capture_output=True, text=True,
                         check=True).stdout
    for f in NEW:
        assert hasattr(lib, f) and re.search(rf"\bT {f}$", out, flags=re.M), f
    assert L.ABI_VERSION == 12 and lib.dsr_abi_version() == 12
    assert re.search(r"^#define DSR_ABI_VERSION 12$", open(HDR).read(), flags=re.M)


def test_mesher_stats_layout_matches_ctypes():
    from reconstruct import _libdsr as L

    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HDR}"', "int main(void){",
             'printf("size %zu\\n", sizeof(dsr_mesher_stats));']
    for fld, _ in L.MesherStats._fields_:
        lines.append(f'printf("{fld} %zu\\n", offsetof(dsr_mesher_stats, {fld}));')
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c99", "-o", exe, src], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    seen = set()
    for line in out.strip().splitlines():
        what, val = line.split()
        if what == "size":
            assert ctypes.sizeof(L.MesherStats) == int(val), line
        else:
            assert getattr(L.MesherStats, what).offset == int(val), line
            seen.add(what)
    for f in ("n_codes", "n_passes", "sign_pass", "margin", "lite_tiles", "exact_tiles", "audit_tiles",
              "violations", "redone_codes", "max_lite_err", "lite_broken_blocks", "lite_ms", "exact_ms", "mc_ms"):
        assert f in seen, f


def test_argument_checks_need_no_device():
    from reconstruct import _libdsr as L

    lib = L.load_library()
    vo = np.zeros(2, np.int32)
    fo = np.zeros(2, np.int32)
    code = np.zeros(64, np.float32)
    assert lib.dsr_mesher_run_batch(None, 1, L.fptr(code), 0.0, None, 0, None, 0, L.iptr(vo), L.iptr(fo)) < 0
    assert lib.dsr_mesher_run_batch(None, -1, L.fptr(code), 0.0, None, 0, None, 0, L.iptr(vo), L.iptr(fo)) < 0
    assert lib.dsr_mesher_run_batch(None, 0, None, 0.0, None, 0, None, 0, None, None) < 0
    st = L.MesherStats()
    assert lib.dsr_mesher_stats_get(None, ctypes.byref(st)) < 0
    assert lib.dsr_mesher_peek(None, 0, None, None, None) < 0


def analytic_volume(d=12):
    """Two overlapping spheres and a box (union of signed distances), on the mesher's grid."""
    g = np.linspace(-1.0, 1.0, d)
    x, y, z = np.meshgrid(g, g, g, indexing="ij")
    s1 = np.sqrt((x + 0.25) ** 2 + y ** 2 + z ** 2) - 0.45
    s2 = np.sqrt((x - 0.2) ** 2 + (y - 0.1) ** 2 + z ** 2) - 0.4
    q = np.stack([np.abs(x - 0.1) - 0.3, np.abs(y + 0.45) - 0.25, np.abs(z - 0.3) - 0.35])
    box = np.linalg.norm(np.maximum(q, 0.0), axis=0) + np.minimum(q.max(axis=0), 0.0)
    return np.minimum(np.minimum(s1, s2), box).astype(np.float32)


@pytest.mark.parametrize("level", [0.0, 0.02])
@pytest.mark.parametrize("seed", [0, 1])
def test_merged_volume_meshes_bitwise_like_the_exact_one(level, seed):
    from oracle.dsr_mc import marching_cubes

    exact = analytic_volume(12)
    rng = np.random.default_rng(seed)
    noise = rng.uniform(-1.0, 1.0, exact.shape) * (0.999 * MARGIN / 4)
    lite = (exact.astype(np.float64) + noise).astype(np.float32)
    assert np.abs(lite.astype(np.float64) - exact).max() < MARGIN / 4
    need, t_need, t_shell = mark_tiles(lite, level)
    assert t_need.any() and not t_need.all()           # something to decode, something saved
    assert not (t_need & t_shell).any()
    n = exact.size
    tile_of = (np.arange(n) // TILE).reshape(exact.shape)
    # both endpoints of every crossing edge of the exact volume lie in a needed tile
    inside = exact < np.float32(level)
    d = exact.shape[0]
    crossings = 0
    for ax in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, d - 1), slice(1, d)
        lo, hi = tuple(lo), tuple(hi)
        cross = inside[lo] != inside[hi]
        crossings += int(cross.sum())
        assert need[lo][cross].all() and need[hi][cross].all()
        assert t_need[tile_of[lo][cross]].all() and t_need[tile_of[hi][cross]].all()
    assert crossings > 0
    # every voxel of the merged volume lies on the exact side of the level
    for decoded in (t_need, t_need | t_shell):
        merged = merge(lite, exact, decoded)
        assert np.array_equal(merged < np.float32(level), inside)
        v0, f0 = marching_cubes(exact, level)
        v1, f1 = marching_cubes(merged, level)
        assert v0.shape[0] > 0 and f0.shape[0] > 0
        assert v0.tobytes() == v1.tobytes() and f0.tobytes() == f1.tobytes()


def test_rule_marks_bad_values_and_flagged_voxels():
    """NaN / infinite lite values and voxels the lite kernel flagged are band voxels: they and
    their neighbours are decoded exactly."""
    exact = analytic_volume(12)
    lite = exact.copy()
    far = np.argwhere(np.abs(exact) > 0.3)
    a, b, c = (tuple(int(v) for v in far[i]) for i in (0, len(far) // 2, len(far) - 1))
    lite[a] = np.nan
    lite[b] = np.inf
    refine = np.zeros(exact.shape, np.uint8)
    refine[c] = 1
    need, t_need, _ = mark_tiles(lite, 0.0, refine=refine)
    clean, _, _ = mark_tiles(exact, 0.0)
    d = exact.shape[0]
    for p in (a, b, c):
        assert need[p] and not clean[p]
        for ax in range(3):
            for sg in (-1, 1):
                q = list(p)
                q[ax] += sg
                if 0 <= q[ax] < d:
                    assert need[tuple(q)]
        assert t_need[(p[0] * d + p[1]) * d + p[2] >> 6]
