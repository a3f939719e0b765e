"""Host side of the fp16-storage mode of CARes18-IBN / EMARes18-IBN (no GPU): the library that holds their attention tails,
libreid_hip_siblings_f16.so (csrc/siblings_f16.hip), is a file of its own that libreid_hip.so opens from its own directory the first
time a sibling checkpoint runs in mode 1.  The product library, what it needs to load and its kernel list (tests/golden/kernels.json)
are untouched; the new library is held to its own list the same way."""
import ctypes
import json
import os
import subprocess
import sys

from reid_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "real-time-reid-tracking_amd", "libreid_hip_siblings_f16.so")


def test_siblings_f16_library_kernels_match_their_list(golden_dir):
    """Kernels read from the library's code objects (tools/so_kernels.py) equal tests/golden/kernels_siblings_f16.json by name, and none
    of them has scratch."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import so_kernels
    rows = so_kernels.kernels(LIB)
    names = sorted(rows)
    got = {so_kernels.short(d): rows[n] for d, n in zip(so_kernels.demangle(names), names)}
    want = json.load(open(os.path.join(golden_dir, "kernels_siblings_f16.json")))["kernels"]
    assert sorted(got) == sorted(want), {"new": sorted(set(got) - set(want)), "gone": sorted(set(want) - set(got))}
    assert len(got) == 7 and sum("ema_tail_f16_kernel" in k for k in got) == 4 and sum("ta_" in k for k in got) == 3
    assert all(v["scratch"] == 0 for v in got.values()) and not any(want.values()), {k: v["scratch"] for k, v in got.items()}


def test_product_library_does_not_link_the_siblings_library():
    needed = subprocess.run(["readelf", "-d", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "NEEDED" in needed                                          # readelf did read the dynamic section
    assert "libreid_hip_siblings_f16" not in needed                    # no new dependency: it is opened on first use


def test_siblings_library_loads_on_its_own_and_exports_the_launchers():
    lib = ctypes.CDLL(LIB)                                             # it needs nothing of the product library
    for name in ("siblings_f16_ta_tail", "siblings_f16_ema_tail", "siblings_f16_ta_workspace_bytes", "siblings_f16_ema_workspace_bytes"):
        assert hasattr(lib, name), name
    needed = subprocess.run(["readelf", "-d", LIB], capture_output=True, text=True, check=True).stdout
    assert "libreid_hip.so" not in needed
    # the workspace query is plain host arithmetic: per image 3 HW + 3 HC + (2 S + 1) WC floats, S row slices of 32768 elements
    lib.siblings_f16_ta_workspace_bytes.restype = ctypes.c_size_t
    for h, w, c, s in ((64, 32, 64, 4), (32, 16, 128, 2), (16, 8, 256, 1), (16, 8, 512, 2)):
        per = 3 * h * w + 3 * h * c + (2 * s + 1) * w * c
        assert lib.siblings_f16_ta_workspace_bytes(3, h, w, c) == 3 * per * 4, (h, w, c)
    assert lib.siblings_f16_ta_workspace_bytes(1, 64, 32, 48) == 0     # a shape the launcher refuses
    lib.siblings_f16_ema_workspace_bytes.restype = ctypes.c_size_t
    assert lib.siblings_f16_ema_workspace_bytes(3, 64, 32, 64) == 0

