"""The evaluation chain's shifted mirrored view and attribute distance on the MI355X (pytest -m gpu tests/test_gpu_eval_links.py).

Kernels (libreid_hip_eval_links.so) through the launchers the entries call: shift_mirror_nchw_kernel bit for bit against the view oracle
of tests/eval_links_ref.py (itself checked against Pillow in tests/test_eval_links_host.py), dist_add_l2_kernel inside that module's
squared-domain bound; every output has a guard row behind it that must still read as NaN.

Entries: reid_descriptor_f32_nchw_shift with every shift at (pad, pad) returns the bits of flip_tta = 1; with other shifts the bits of
the descriptor kernel on the embeddings of x and of the oracle's view of x; reid_descriptor_images_u8_shift the bits of the float entry
on PIL-preprocessed images with the normalised-zero fill - at 256 x 128 and on the any-size route.  The chain: evaluate_reid with
strong_offsets and attribute_dist."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import seres18
from reid_amd import _ffi, data_transforms, inference_utils, reid_inference, synth, tricks, weights
from reid_amd.engine import Engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_links_ref as ref  # noqa: E402
import pil_resize_ref  # noqa: E402

pytestmark = [pytest.mark.gpu]

FILL = np.asarray([-1.5, 0.25, 2.75], np.float32)          # distinct, signed, per channel
TILE = 64
SHIFTS5 = np.asarray([[0, 0], [0, 20], [20, 0], [20, 20], [3, 17]], np.int32)
SOURCES5 = ((90, 200), (64, 32), (257, 129), (300, 117), (128, 64))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def eng():
    from reid_amd.engine import get_engine
    e = get_engine(0)
    yield e
    e.set_side_index(None)
    e.set_precision(0)
    e.set_hw_precision(None)
    e.set_chunk(1024)


@pytest.fixture(scope="module")
def sd0():
    return synth.seres18_state_dict(0)


@pytest.fixture()
def eng_w0(eng, sd0):
    eng.set_precision(0)
    eng.load_seres18(*weights.pack_seres18(sd0)[:2])
    return eng


# ---------------------------------------------------------------------------------------------- 1. shift_mirror_nchw_kernel
@pytest.mark.parametrize("m,h,w", [(3, 256, 128), (3, 33, 47), (1, 224, 268)])
def test_shift_mirror_is_the_oracle_bit_for_bit(eng, m, h, w):
    """16-byte stores (w % 4 == 0) and scalar ones (47); per pad the four corner shifts, the centre and (3, 17), a different one per
    image; a distinct signed fill per channel; the guard row stays NaN."""
    x = np.random.default_rng(h + w).normal(size=(m, 3, h, w)).astype(np.float32)
    for pad in ref.PADS:
        sh = ref.shifts(pad)
        for k in range(0, len(sh), m):
            tl = np.asarray([sh[(k + i) % len(sh)] for i in range(m)], np.int32)
            y, guard = eng.debug_shift_mirror(x, tl, pad, FILL)
            assert np.array_equal(_bits(y), _bits(ref.shift_views(x, tl, pad, FILL))), (pad, tl.tolist())
            assert np.isnan(guard).all()
    y, _ = eng.debug_shift_mirror(x, np.full((m, 2), 10, np.int32), 10, FILL)
    assert np.array_equal(_bits(y), _bits(x[:, :, :, ::-1]))              # (pad, pad): the plain mirror
    assert eng.fault_bits() == 0


@pytest.mark.parametrize("m,h,w", [(48, 256, 128), (240, 33, 47)])
def test_shift_mirror_above_the_grid_cap(eng, m, h, w):
    """More work than 4096 blocks of 256 threads take in one step (a thread per four pixels at 128 wide, per pixel at 47): the loop."""
    cap = C.CDLL(os.path.join(os.path.dirname(_ffi.LIB_PATH), "libreid_hip_eval_links.so")).eval_links_grid_cap()
    assert m * 3 * h * (w // 4 if w % 4 == 0 else w) > cap * 256
    rng = np.random.default_rng(m)
    x = rng.normal(size=(m, 3, h, w)).astype(np.float32)
    tl = rng.integers(0, 21, (m, 2)).astype(np.int32)
    y, guard = eng.debug_shift_mirror(x, tl, 10, FILL)
    assert np.array_equal(_bits(y), _bits(ref.shift_views(x, tl, 10, FILL))) and np.isnan(guard).all()


# ---------------------------------------------------------------------------------------------- 2. descriptors at 256 x 128
def _x5(h=256, w=128, seed=4):
    return seres18.preprocess_u8(synth.smooth_crops_u8(5, seed, h, w)).numpy()


def _from_views(eng, x, tl, pad, fill):
    """The descriptor kernel (reid_debug_descriptor) on the embeddings of x and of the oracle's view of x."""
    e1, l1 = eng.embed_f32_nchw(x, logits=True)
    e2, l2 = eng.embed_f32_nchw(ref.shift_views(x, tl, pad, fill), logits=True)
    out, guard = eng.debug_descriptor(e1, l1, e2, l2)
    assert np.isnan(guard).all()
    return out


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_centre_shift_gives_the_bits_of_flip_tta(eng_w0, mode):
    eng, x = eng_w0, _x5()
    eng.set_precision(mode)
    try:
        want = eng.descriptor_f32_nchw(x, flip_tta=True)
        got = eng.descriptor_f32_nchw_shift(x, np.full((5, 2), 10, np.int32), pad=10)
        assert np.array_equal(_bits(got), _bits(want))
        assert np.array_equal(_bits(eng.descriptor_f32_nchw_shift(x, np.zeros((5, 2), np.int32), pad=0)), _bits(want))
    finally:
        eng.set_precision(0)


def test_centre_shift_gives_the_bits_of_flip_tta_cares18(eng):
    x = _x5()
    eng.set_precision(0)
    eng.load_seres18(*weights.pack_seres18(synth.cares18_state_dict(0))[:2])
    want = eng.descriptor_f32_nchw(x, flip_tta=True)
    assert np.array_equal(_bits(eng.descriptor_f32_nchw_shift(x, np.full((5, 2), 10, np.int32), pad=10)), _bits(want))


def test_shifted_view_descriptors_at_256x128(eng_w0):
    eng, x = eng_w0, _x5()
    fill = Engine.normalised_zero_fill()
    got = eng.descriptor_f32_nchw_shift(x, SHIFTS5, pad=10, fill=fill)
    assert np.array_equal(_bits(got), _bits(_from_views(eng, x, SHIFTS5, 10, fill)))
    other = eng.descriptor_f32_nchw_shift(x, SHIFTS5, pad=10, fill=FILL)      # the fill reaches the view
    assert np.array_equal(_bits(other), _bits(_from_views(eng, x, SHIFTS5, 10, FILL))) and not np.array_equal(_bits(other), _bits(got))
    corner = eng.descriptor_f32_nchw_shift(x, np.zeros((5, 2), np.int32), pad=10)
    centre = eng.descriptor_f32_nchw_shift(x, np.full((5, 2), 10, np.int32), pad=10)
    assert all(not np.array_equal(_bits(corner[i]), _bits(centre[i])) for i in range(5))
    try:                                                                    # passes of 2 images: the shifts follow their images
        eng.set_chunk(2)
        assert np.array_equal(_bits(eng.descriptor_f32_nchw_shift(x, SHIFTS5, pad=10, fill=fill)), _bits(got))
    finally:
        eng.set_chunk(1024)
    assert eng.fault_bits() == 0


# ---------------------------------------------------------------------------------------------- 3. the any-size route
@pytest.mark.parametrize("hw_precision", ["f32", "f16x3"])
def test_any_size_route(eng_w0, hw_precision):
    eng, x = eng_w0, _x5(96, 72, 22)
    fill = Engine.normalised_zero_fill()
    with eng.hw_precision_scope(hw_precision):
        want = eng.descriptor_f32_nchw(x, flip_tta=True)
        assert np.array_equal(_bits(eng.descriptor_f32_nchw_shift(x, np.full((5, 2), 10, np.int32), pad=10)), _bits(want))
        got = eng.descriptor_f32_nchw_shift(x, SHIFTS5, pad=10, fill=fill)
        assert np.array_equal(_bits(got), _bits(_from_views(eng, x, SHIFTS5, 10, fill)))
        assert not np.array_equal(_bits(got), _bits(want))
        try:                                                                # chunk 1: passes of 4 images, two passes for 5
            eng.set_chunk(1)
            assert np.array_equal(_bits(eng.descriptor_f32_nchw_shift(x, SHIFTS5, pad=10, fill=fill)), _bits(got))
        finally:
            eng.set_chunk(1024)
    assert eng.fault_bits() == 0


# ---------------------------------------------------------------------------------------------- 4. uint8 images
@pytest.mark.parametrize("size", [(256, 128), (96, 72)])
def test_uint8_entry_equals_the_float_entry_on_pil_preprocessed_images(eng_w0, size):
    eng = eng_w0
    images = [pil_resize_ref.formula_image(h, w, i) for i, (h, w) in enumerate(SOURCES5)]
    x = pil_resize_ref.preprocess(images, *size)
    with eng.hw_precision_scope("f32" if size != (256, 128) else None):
        want = eng.descriptor_f32_nchw_shift(x, SHIFTS5, pad=10, fill=Engine.normalised_zero_fill())
        got = eng.descriptor_images_u8_shift(images, SHIFTS5, pad=10, size=size)
        assert np.array_equal(_bits(got), _bits(want))
        assert not np.array_equal(_bits(got), _bits(eng.descriptor_images_u8(images, size=size)))
        # pending side indices serve both views: n for the uint8 entry, what the float entry computes when it is given them twice
        cams = np.asarray([2, 0, 5, 1, 3], np.int32)
        eng.set_side_index(np.concatenate([cams, cams]))
        want_side = eng.descriptor_f32_nchw_shift(x, SHIFTS5, pad=10, fill=Engine.normalised_zero_fill())
        eng.set_side_index(cams)
        got_side = eng.descriptor_images_u8_shift(images, SHIFTS5, pad=10, size=size)
        assert np.array_equal(_bits(got_side), _bits(want_side)) and not np.array_equal(_bits(got_side), _bits(got))
    assert eng.fault_bits() == 0


# ---------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_name_their_argument(eng_w0):
    eng = eng_w0
    x = np.zeros((2, 3, 256, 128), np.float32)
    out = np.full((2, 512 + eng.num_class), 7, np.float32)
    fill = Engine.normalised_zero_fill()

    def status(tl, pad, f=fill):
        tl = np.asarray(tl, np.int32)
        return eng.lib.reid_descriptor_f32_nchw_shift(eng.h, _p(x), 2, 256, 128, _p(tl), pad, _p(f), _p(out))

    assert status([[0, 0], [0, 21]], 10) == -1
    msg = eng.lib.reid_last_error().decode()
    assert "image 1" in msg and "left 21" in msg
    assert status([[-1, 0], [0, 0]], 10) == -1 and "image 0" in eng.lib.reid_last_error().decode()
    assert status([[0, 0], [0, 0]], 33) == -1 and "pad 33" in eng.lib.reid_last_error().decode()
    assert status([[0, 0], [0, 0]], -1) == -1 and "pad" in eng.lib.reid_last_error().decode()
    assert status([[0, 0], [0, 0]], 10, None) == -1 and "fill3" in eng.lib.reid_last_error().decode()
    assert status([[0, 0], [0, 0]], 10) == 0 and status([[64, 64], [0, 0]], 32) == 0
    img = np.zeros((9, 7, 3), np.uint8)
    offs, hw = np.asarray([0, 0], np.int64), np.asarray([[9, 7], [9, 7]], np.int32)
    bad = np.asarray([[0, 0], [3, 0]], np.int32)
    assert eng.lib.reid_descriptor_images_u8_shift(eng.h, _p(img), _p(offs), _p(hw), 2, 256, 128, None, _p(bad), 1, _p(out)) == -1
    assert "image 1" in eng.lib.reid_last_error().decode() and "top 3" in eng.lib.reid_last_error().decode()
    a = np.ones((3, 33), np.float32)
    io = np.zeros((3, 3), np.float32)
    assert eng.lib.reid_distmat_add_l2(eng.h, _p(a), 3, 33, _p(io)) == -1 and "1 .. 32" in eng.lib.reid_last_error().decode()
    assert eng.lib.reid_distmat_add_l2(eng.h, _p(a), 3, 0, _p(io)) == -1
    assert eng.lib.reid_distmat_add_l2(eng.h, _p(a), 0, 30, _p(io)) == 0 and not io.any()
    assert eng.fault_bits() == 0


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from reid_amd import _ffi, synth, weights
from reid_amd.engine import get_engine
assert _ffi.LIB_PATH.startswith(sys.argv[1]), _ffi.LIB_PATH
eng = get_engine(0)
eng.load_seres18(*weights.pack_seres18(synth.seres18_state_dict(0))[:2])
x = np.zeros((1, 3, 256, 128), np.float32)
tl = np.full((1, 2), 10, np.int32)
before = eng.descriptor_f32_nchw(x)
bad = 0
calls = (lambda: eng.descriptor_f32_nchw_shift(x, tl), lambda: eng.descriptor_images_u8_shift([np.zeros((9, 7, 3), np.uint8)], tl),
         lambda: eng.distmat_add_l2(np.ones((3, 30), np.float32), np.zeros((3, 3), np.float32)))
for call in calls:
    try:
        call()
        bad += 1
    except _ffi.ReidHipError as e:
        print("RAISED", e.status, e)
        bad += not (e.status == -3 and "libreid_hip_eval_links.so" in str(e) and eng.fault_bits() == 0)
same = np.array_equal(before, eng.descriptor_f32_nchw(x))
sys.exit(0 if bad == 0 and same else 3)
"""


def test_missing_library_is_an_error_of_the_call(tmp_path):
    """A copy of the build without libreid_hip_eval_links.so, loaded through REID_HIP_LIB in a fresh child process: the new entries are
    REID_ERR_STATE naming the file, and reid_descriptor_f32_nchw works before and after."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = "libreid_hip_eval_links.so"
    shutil.copytree(os.path.join(root, "reid_amd"), tmp_path / "reid_amd", ignore=shutil.ignore_patterns("__pycache__"))
    shutil.copytree(os.path.join(root, "real-time-reid-tracking_amd"), tmp_path / "real-time-reid-tracking_amd",
                    ignore=shutil.ignore_patterns("__pycache__", "csrc", lib))
    assert not (tmp_path / "real-time-reid-tracking_amd" / lib).exists()
    env = dict(os.environ, REID_HIP_LIB=str(tmp_path / "real-time-reid-tracking_amd" / "libreid_hip.so"))
    r = subprocess.run([sys.executable, "-c", _CHILD, str(tmp_path)], capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.count("RAISED -3") == 3 and lib in r.stdout


# ---------------------------------------------------------------------------------------------- 6. dist_add_l2_kernel
@pytest.mark.parametrize("d", [1, 30, 32])
@pytest.mark.parametrize("n", [1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 2])
def test_dist_add_l2_stays_inside_the_bound(eng, n, d):
    """Unit attribute-like rows with many duplicates (distances at the clamp), inout in [0, 1] with exact zeros: every element inside
    the squared-domain bound moved by inout and widened by one ulp of the sum; the guard row intact; three calls, equal bits; a zero
    inout becomes symmetric bit for bit; a NaN in inout stays one, a NaN in a row fills its row and column."""
    rng = np.random.default_rng(1000 * n + d)
    a = ref.attribute_like_rows(n, d, n + d)
    base = rng.uniform(0, 1, (n, n)).astype(np.float32)
    base[rng.uniform(size=(n, n)) < 0.3] = 0.0
    lo, hi = ref.dist_bounds(a)
    out, guard = eng.debug_dist_add_l2(a, base)
    ok = ref.inside_sum(out, base, lo, hi)
    assert ok.all(), (int((~ok).sum()), np.argwhere(~ok)[:4].tolist())
    assert np.isnan(guard).all()
    for _ in range(2):
        again, _g = eng.debug_dist_add_l2(a, base)
        assert np.array_equal(_bits(again), _bits(out))
    zero, _g = eng.debug_dist_add_l2(a, np.zeros((n, n), np.float32))
    assert np.array_equal(_bits(zero), _bits(zero.T)) and ref.inside(zero, lo, hi).all()
    assert np.array_equal(_bits(eng.distmat_add_l2(a, np.zeros((n, n), np.float32))), _bits(zero))       # the host entry: the same launch
    withnan = base.copy()
    withnan[n // 2, n // 3] = np.nan
    got, _g = eng.debug_dist_add_l2(a, withnan)
    assert np.isnan(got[n // 2, n // 3]) and np.isnan(got).sum() == 1
    bad = a.copy()
    bad[n // 2, d // 2] = np.nan
    got, _g = eng.debug_dist_add_l2(bad, base)
    want_nan = np.zeros((n, n), bool)
    want_nan[n // 2, :] = want_nan[:, n // 2] = True
    assert np.array_equal(np.isnan(got), want_nan)
    assert eng.fault_bits() == 0


# ---------------------------------------------------------------------------------------------- 7. the chain
def test_evaluate_reid_with_both_links(eng_w0, golden_dir):
    eng = eng_w0
    p = synth.e2e_problem(seed=100, n_gallery=40, n_query=12)
    ng, nq = 40, 12
    torch.manual_seed(7)
    offsets = data_transforms.strong_inference_offsets(ng + nq)
    labels = np.concatenate([p["gl"], p["ql"]])
    mat = os.path.join(golden_dir, "market_attribute_small.mat")
    rows = tricks.attribute_rows(labels, mat)
    seen = []

    def cluster(d):
        seen.append(d)
        return np.arange(d.shape[0]) % 3

    def run(**kw):
        taps = {}
        del seen[:]
        cmc, m_ap = reid_inference.evaluate_reid(p["g_img"], p["gl"], p["gc"], p["gs"], p["q_img"], p["ql"], p["qc"], p["qs"], engine=eng, taps=taps,
                                                 verbose=False, k1=6, k2=3, cluster_fn=cluster, **kw)
        assert cmc.shape == (ng,) and 0.0 <= m_ap <= 1.0 and len(seen) == 1
        return taps, seen[0]

    taps, handed = run(strong_offsets=offsets, attribute_dist=rows)
    # gallery and query are one call each in the chain (the forward's launch forms, and so its bits, depend on the batch)
    want = np.concatenate([inference_utils.extract_descriptors(p["g_img"], strong_offsets=offsets[:ng]),
                           inference_utils.extract_descriptors(p["q_img"], strong_offsets=offsets[ng:])])
    assert np.array_equal(_bits(taps["desc"]), _bits(want))
    assert handed is taps["dists"]
    lo, hi = ref.dist_bounds(tricks.normalize_rows(rows))
    ok = ref.inside_sum(taps["dists"], taps["jaccard"], lo, hi)
    assert ok.all(), int((~ok).sum())
    assert (taps["dists"] >= taps["jaccard"]).all() and not np.array_equal(taps["dists"], taps["jaccard"])
    # the add is the host entry's launch on the same operands: its bits (the re-ranking sums with LDS atomics, so two runs' Jaccard
    # matrices are compared through what was added to each, not with each other)
    unit = tricks.normalize_rows(rows)
    assert np.array_equal(_bits(taps["dists"]), _bits(eng.distmat_add_l2(unit, taps["jaccard"].copy())))
    pair, _ = run(strong_offsets=offsets, attribute_dist=(labels, mat))          # the (labels, path) form: the same rows
    assert np.array_equal(_bits(pair["dists"]), _bits(eng.distmat_add_l2(unit, pair["jaccard"].copy())))
    assert np.array_equal(_bits(pair["desc"]), _bits(taps["desc"]))
    torch.manual_seed(7)                                                         # strong_inference=True draws the same offsets itself
    drawn, _ = run(strong_inference=True)
    assert np.array_equal(_bits(drawn["desc"]), _bits(taps["desc"]))
    plain, handed = run()                                                        # both keywords left out: today's chain
    want = np.concatenate([inference_utils.extract_descriptors(p["g_img"]), inference_utils.extract_descriptors(p["q_img"])])
    assert np.array_equal(_bits(plain["desc"]), _bits(want))
    assert handed is plain["dists"] and np.array_equal(_bits(plain["dists"]), _bits(plain["jaccard"]))
    assert not np.array_equal(_bits(plain["desc"]), _bits(taps["desc"]))
    assert np.array_equal(_bits(drawn["jaccard"]), _bits(drawn["dists"]))
    assert eng.fault_bits() == 0
