"""Host side of the frame pipeline at any crop size (no GPU): the side library's kernel list and independence, the declared / bound /
exported surface, the cut of the fused front end (anysize_front_plan) for every height and width, the Python rules up to the first device
call, and the float64 restatement of tests/anysize_front_ref.py against torch with the mutations it is there to catch."""
import ctypes
import inspect
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from reid_amd import _ffi, synth
from reid_amd.engine import Engine
from reid_amd.tracking import CameraStream, LookaheadCameraStream, MultiCameraStream, ShardedCameraStream

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import anysize_front_ref as ref  # noqa: E402
import test_gpu_frontend as fe  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "real-time-reid-tracking_amd", "libreid_hip_anysize_front.so")
CPU_SIZES = ((32, 32), (33, 47), (96, 72), (57, 131), (33, 49))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()


@pytest.fixture(scope="module")
def stem():
    return ref.stem_of(synth.seres18_state_dict(0))


@pytest.fixture(scope="module")
def crops():
    return ref.crops()


def _kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import so_kernels
    rows = so_kernels.kernels(LIB)
    names = sorted(rows)
    return {so_kernels.short(d): rows[n] for d, n in zip(so_kernels.demangle(names), names)}


# ---------------------------------------------------------------------------------------------- 1. the library and the surface
def test_side_library_kernels_match_their_list(built, golden_dir):
    """libreid_hip_anysize_front.so holds the kernels of tests/golden/kernels_anysize_front.json by name, without scratch or AGPRs, under the
    VGPR and LDS caps that two blocks per CU allow; the product library does not name the file among what it needs, the side library
    needs nothing of the project's, and it loads on its own, without a GPU."""
    got = _kernels()
    spec = json.load(open(os.path.join(golden_dir, "kernels_anysize_front.json")))
    want = spec["kernels"]
    assert sorted(got) == sorted(want), {"new": sorted(set(got) - set(want)), "gone": sorted(set(want) - set(got))}
    assert all(v["scratch"] == 0 for v in got.values()) and not any(want.values()), {k: v["scratch"] for k, v in got.items()}
    assert all(v["agprs"] == 0 and 0 < v["vgprs"] <= spec["max_vgprs"] for v in got.values()), {k: v["vgprs"] for k, v in got.items()}
    assert all(0 < v["lds"] <= spec["max_lds"] for v in got.values()), {k: v["lds"] for k, v in got.items()}
    needed = subprocess.run(["readelf", "-d", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "NEEDED" in needed and "libreid_hip_anysize" not in needed
    own = subprocess.run(["readelf", "-d", LIB], capture_output=True, text=True, check=True).stdout
    assert "libreid_hip.so" not in own and "libreid_hip_" not in own
    lib = ctypes.CDLL(LIB)
    assert all(hasattr(lib, s) for s in ("anysize_front", "anysize_front_plan", "anysize_front_plan_band", "anysize_front_plan_coltile"))


def test_the_entries_and_the_harness_are_declared_bound_and_exported(built):
    hdr = open(os.path.join(ROOT, "include", "reid_hip.h")).read()
    dbg_hdr = open(os.path.join(ROOT, "include", "reid_hip_debug.h")).read()
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    declared = set(re.findall(r"^int\s+(reid_[a-z0-9_]+)\s*\(", hdr, re.M))
    for sym in ("reid_frame_submit_hw", "reid_embed_frame_u8_hw"):
        assert sym in declared and sym in _ffi.EXPORTS and sym in _ffi._SIGS and hasattr(lib, sym), sym
    assert len(_ffi._SIGS["reid_frame_submit_hw"][1]) == 9 and len(_ffi._SIGS["reid_embed_frame_u8_hw"][1]) == 11
    assert "reid_debug_any_front(" in dbg_hdr and "reid_debug_any_front" in _ffi.DEBUG_EXPORTS and hasattr(_ffi.debug_lib(), "reid_debug_any_front")
    for name in ("frame_submit_hw", "debug_any_front", "embed_frame_u8"):
        assert hasattr(Engine, name), name
    p = inspect.signature(Engine.embed_frame_u8).parameters
    assert p["size"].default is None and p["mean_std"].default is None
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "any_front" in readme and "any_front" in open(os.path.join(ROOT, "real-time-reid-tracking_amd", "csrc", "debug.hip")).read()


# ---------------------------------------------------------------------------------------------- 2. the cut
class Geom(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("H1", "W1", "H2", "W2", "nbands", "bands_per_block", "nstrips", "ncoltiles", "lds_bytes",
                                              "in_rows", "in_pitch", "max_ncol")]


class Band(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("p0", "np", "y_lo", "iy_lo")]


class ColTile(ctypes.Structure):
    _fields_ = [(n, ctypes.c_int32) for n in ("q0", "nq", "x0", "ncol", "ix_lo", "npx")]


def _plan(lib, h, w):
    g = Geom()
    assert lib.anysize_front_plan(h, w, ctypes.byref(g)) == 0
    bands, tiles = [Band() for _ in range(g.nbands)], [ColTile() for _ in range(g.ncoltiles)]
    for i, b in enumerate(bands):
        assert lib.anysize_front_plan_band(h, w, i, ctypes.byref(b)) == 0
    for i, t in enumerate(tiles):
        assert lib.anysize_front_plan_coltile(h, w, i, ctypes.byref(t)) == 0
    return g, bands, tiles


def test_plan_covers_every_pooled_pixel_once_and_stays_inside(built):
    """Every H with W = 32 and every W with H = 32 (rows and columns are cut independently).  Bands and column tiles partition the pooled
    rows / columns; the stem rows / columns a pooled pixel's window needs inside the map are the band's five local rows / the tile's ncol
    columns, and the input rows / pixels those need are among the 15 staged rows / npx staged pixels; what the kernel reads from the LDS
    image (the padded taps of the last column included) stays inside a staged row, a band's image and the ring inside the LDS declared."""
    lib = ctypes.CDLL(LIB)
    lds = list(_kernels().values())[0]["lds"]
    g = Geom()
    for bad in ((31, 64), (64, 513), (0, 0)):
        assert lib.anysize_front_plan(bad[0], bad[1], ctypes.byref(g)) != 0
    assert lib.anysize_front_plan_band(64, 64, 99, ctypes.byref(Band())) != 0 and lib.anysize_front_plan_coltile(64, 64, 1, ctypes.byref(ColTile())) != 0
    seen_tiles, seen_bpb = set(), set()
    for h, w in [(h, 32) for h in range(32, 513)] + [(32, w) for w in range(32, 513)] + [(512, 512), (224, 268)]:
        g, bands, tiles = _plan(lib, h, w)
        assert (g.H1, g.W1, g.H2, g.W2) == ref.maps(h, w)
        assert g.lds_bytes == lds == (64 * 172 + g.in_rows * g.in_pitch + 3 * g.max_ncol * 64) * 4 and g.in_rows == 15 and g.max_ncol == 32
        assert 1 <= g.bands_per_block <= 8 and (g.nstrips - 1) * g.bands_per_block < g.nbands <= g.nstrips * g.bands_per_block
        seen_tiles.add(g.ncoltiles)
        seen_bpb.add(g.bands_per_block)
        rows = [p for b in bands for p in range(b.p0, b.p0 + b.np)]
        assert rows == list(range(g.H2)), (h, w)
        for b in bands:
            assert 1 <= b.np <= 2 and b.y_lo == 2 * b.p0 - 1 and b.iy_lo == 2 * b.y_lo - 3
            for p in range(b.p0, b.p0 + b.np):
                for y in range(max(0, 2 * p - 1), min(g.H1, 2 * p + 2)):
                    j = y - b.y_lo
                    assert 2 * (p - b.p0) <= j <= 2 * (p - b.p0) + 2 and 0 <= j < 5       # the phase's ring rows
                    for iy in range(2 * y - 3, 2 * y + 4):
                        assert 0 <= iy - b.iy_lo == 2 * j + (iy - (2 * y - 3)) < g.in_rows
        cols = [q for t in tiles for q in range(t.q0, t.q0 + t.nq)]
        assert cols == list(range(g.W2)), (h, w)
        for t in tiles:
            assert t.nq >= 1 and 0 <= t.x0 and 1 <= t.ncol <= g.max_ncol and t.x0 + t.ncol <= g.W1
            assert t.ix_lo == 2 * t.x0 - 3 and t.npx == 2 * t.ncol + 5 and 3 * t.npx <= g.in_pitch
            for q in range(t.q0, t.q0 + t.nq):
                for x in range(max(0, 2 * q - 1), min(g.W1, 2 * q + 2)):
                    cc = x - t.x0
                    assert 0 <= cc < t.ncol
                    assert 0 <= (2 * x - 3) - t.ix_lo == 2 * cc and (2 * x + 3) - t.ix_lo < t.npx
            # lane half 1, last 8-group, last float of the second ds_read_b64: 6 cc + 4 + 16 + 3
            assert 6 * (t.ncol - 1) + 23 < g.in_pitch
    assert seen_tiles == set(range(1, 10)) and {1, 8} <= seen_bpb


# ---------------------------------------------------------------------------------------------- 3. the Python rules
def test_stream_classes_take_seres18_hw():
    """arch="seres18_hw" and the trailing keyword hw_precision belong to the three stream classes; a side of 31 or 513, a bad mean_std and
    hw_precision="f16" raise ValueError before any device call - with no GPU in this test, anything that reached the engine would fail
    differently.  The defaults and ShardedCameraStream are as they were."""
    blob = np.zeros(4, np.float32)
    for cls, extra in ((CameraStream, ()), (MultiCameraStream, (2,)), (LookaheadCameraStream, ())):
        p = inspect.signature(cls.__init__).parameters
        assert list(p)[-1] == "hw_precision" and p["hw_precision"].default is None and p["arch"].default == "seres18", cls
        for size in ((31, 64), (128, 513), (128,), "big"):
            with pytest.raises(ValueError):
                cls(blob, "", *extra, arch="seres18_hw", size=size)
        for ms in ([0.5, 0.5, 0.5, 0.2, 0.0, 0.2], [0.5] * 5, [[0.5] * 3, [float("nan")] * 3]):
            with pytest.raises(ValueError):
                cls(blob, "", *extra, arch="seres18_hw", size=(128, 64), mean_std=ms)
        for hp in ("f16", 1, True):
            with pytest.raises(ValueError, match="hw_precision"):
                cls(blob, "", *extra, arch="seres18_hw", size=(128, 64), hw_precision=hp)
        with pytest.raises(ValueError, match="hw_precision"):
            cls(blob, "", *extra, hw_precision="f16x3")
        with pytest.raises(ValueError, match="arch"):
            cls(blob, "", *extra, arch="seres18_any")
    assert "arch" not in inspect.signature(ShardedCameraStream.__init__).parameters
    assert Engine._hw_crop_args((128, 64), None) == (128, 64, None)
    with pytest.raises(ValueError):
        Engine._hw_crop_args((128, 600), None)


# ---------------------------------------------------------------------------------------------- 4. the restatement
def test_resized_is_resize64_at_256x128():
    """The generalised resize of the restatement is test_gpu_frontend.resize64 where that one applies: the same values, and a bound
    that is the same plus the one rounding a general std adds."""
    for crop in ref.crops()[1:] + [np.random.default_rng(1).integers(0, 256, (40, 7, 3), dtype=np.uint8)]:
        v, b = ref.resized(crop, 256, 128)
        v0, b0 = fe.resize64(crop)
        np.testing.assert_array_equal(v, v0)
        assert (b >= b0).all() and (b <= b0 + ref.SAFETY * ref.U * np.abs(v0) * (1 + 1e-12)).all()


@pytest.mark.parametrize("size", CPU_SIZES, ids=["%dx%d" % s for s in CPU_SIZES])
def test_restatement_against_torch(stem, crops, size):
    """F.conv2d + F.max_pool2d in float64 on oracle.matching.preprocess (fp32: the resize the device equals bit for bit) lies within the
    restatement's bound, for the default and another Normalize on the host side of it."""
    import torch
    import torch.nn.functional as F
    from oracle import matching
    w, _, scale, shift = stem
    h, wd = size
    x = torch.from_numpy(matching.preprocess(crops, size=(wd, h)).astype(np.float64))
    assert x.shape[2:] == (h, wd)
    y = F.conv2d(x, torch.from_numpy(w.astype(np.float64)).permute(0, 3, 1, 2), None, 2, 3)
    y = y * torch.from_numpy(scale.astype(np.float64))[None, :, None, None] + torch.from_numpy(shift.astype(np.float64))[None, :, None, None]
    got = F.max_pool2d(y, 3, 2, 1).permute(0, 2, 3, 1).numpy()
    assert got.shape[1:] == ref.maps(h, wd)[2:] + (64,)
    worst = 0.0
    for i, crop in enumerate(crops):
        want, b = ref.front64(crop, h, wd, w, scale, shift)
        err = np.abs(got[i] - want)
        assert (err <= b).all(), (size, crop.shape, float((err / b).max()))
        worst = max(worst, float((err / b).max()))
    assert 0.0 < worst < 1.0


def test_mutations_leave_the_bound(stem, crops):
    """What the bound must be able to see, on the GPU test's own inputs: a pool that pads with 0 (the stem has no ReLU: negative maxima
    exist), the last stem row / column left out when their count is odd, the taps of 256 x 128 at another size."""
    w, _, scale, shift = stem
    for size in CPU_SIZES:
        h1, w1 = ref.maps(*size)[:2]
        for i, crop in enumerate(crops):
            good, b = ref.front64(crop, size[0], size[1], w, scale, shift)
            zero = np.abs(ref.front64(crop, size[0], size[1], w, scale, shift, pad=0.0)[0] - good) > b
            assert zero[0].any() and zero[:, 0].any() and not zero[1:-1, 1:-1].any(), (size, i)
            if h1 % 2 or w1 % 2:
                drop = np.abs(ref.front64(crop, size[0], size[1], w, scale, shift, drop_last=True)[0] - good) > b
                assert drop.any() and (not h1 % 2 or drop[-1].any()) and (not w1 % 2 or drop[:, -1].any()), (size, i)
            if i > 0:      # source (1, 1) is one colour at every size
                taps = np.abs(ref.front64(crop, size[0], size[1], w, scale, shift, taps_size=(256, 128))[0] - good) > b
                assert taps.mean() > 0.5, (size, i, float(taps.mean()))
    assert any(ref.maps(*s)[0] % 2 for s in CPU_SIZES) and any(ref.maps(*s)[1] % 2 for s in CPU_SIZES)
