"""Host side of the evaluation chain's two links (no GPU): the view oracle against Pillow itself, the crop offsets against torch's
draws, the attribute table and distance against the reference's own numbers (tests/golden/eval_links.npz, tools/gen_golden_eval_links.py),
the side library's kernel list and independence, the declared / bound / exported surface, and the Python keyword rules up to the first
device call."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from reid_amd import _ffi, data_transforms, inference_utils, reid_inference, tricks
from reid_amd.engine import Engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_links_ref as ref  # noqa: E402
import pil_resize_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "real-time-reid-tracking_amd", "libreid_hip_eval_links.so")
ENTRIES = ("reid_descriptor_f32_nchw_shift", "reid_descriptor_f32_nchw_shift_dev", "reid_descriptor_images_u8_shift", "reid_distmat_add_l2",
           "reid_distmat_add_l2_dev")
HARNESSES = ("reid_debug_shift_mirror", "reid_debug_dist_add_l2")


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "eval_links.npz"))


@pytest.fixture(scope="module")
def mat_path(golden_dir):
    return os.path.join(golden_dir, "market_attribute_small.mat")


# ---------------------------------------------------------------------------------------------- 1. the view
@pytest.mark.parametrize("size", ref.SIZES)
@pytest.mark.parametrize("pad", ref.PADS)
def test_view_oracle_is_pillows_flip_pad_crop(size, pad):
    """The formula on uint8 images against what torchvision's PIL back end calls: transpose(FLIP_LEFT_RIGHT), ImageOps.expand(border=pad,
    fill=0), crop((left, top, left + W, top + H)).  One mutation each: the source unmirrored, top and left exchanged."""
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageOps
    h, w = size
    img = pil_resize_ref.formula_image(h, w, 3)
    chw = np.ascontiguousarray(img.transpose(2, 0, 1))
    caught = {"mirror": False, "swap": False}
    for top, left in ref.shifts(pad):
        pil = ImageOps.expand(Image.fromarray(img).transpose(Image.FLIP_LEFT_RIGHT), border=pad, fill=0).crop((left, top, left + w, top + h))
        want = np.asarray(pil).transpose(2, 0, 1)
        assert np.array_equal(ref.shift_view(chw, top, left, pad, (0, 0, 0)), want), (top, left)
        caught["mirror"] |= not np.array_equal(ref.shift_view(chw, top, left, pad, (0, 0, 0), mirror=False), want)
        caught["swap"] |= not np.array_equal(ref.shift_view(chw, top, left, pad, (0, 0, 0), swap=True), want)
    assert caught["mirror"]
    assert caught["swap"] or pad == 0                                # pad 0 has the one shift (0, 0): nothing to exchange


def test_the_centre_shift_is_the_plain_mirror_and_fill_is_per_channel():
    x = np.random.default_rng(0).normal(size=(3, 33, 47)).astype(np.float32)
    assert np.array_equal(ref.shift_view(x, 10, 10, 10, (1, 2, 3)), x[:, :, ::-1])
    v = ref.shift_view(x, 0, 0, 10, (-1.5, 2.5, -3.5))
    assert (v[0, :10] == -1.5).all() and (v[1, :, :10] == 2.5).all() and (v[2, :10] == -3.5).all()
    assert np.array_equal(v[:, 10:, 10:], x[:, :23, ::-1][:, :, :37])


def test_normalised_zero_fill_is_the_tables_entry_for_black():
    for ms in (None, (0.5, 0.4, 0.3, 0.2, 0.25, 0.3)):
        table = pil_resize_ref.norm_table(pil_resize_ref.IMAGENET_MEAN_STD if ms is None else ms)
        got = Engine.normalised_zero_fill(ms)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), table[:, 0].copy().view(np.uint32))
    with pytest.raises(ValueError):
        Engine.normalised_zero_fill((0.5,) * 5)


# ---------------------------------------------------------------------------------------------- 2. the offsets
def test_strong_inference_offsets_are_torchs_draws_top_before_left():
    import torch
    for pad in (10, 1):
        torch.manual_seed(11)
        got = data_transforms.strong_inference_offsets(9, pad)
        torch.manual_seed(11)
        want = [int(torch.randint(0, 2 * pad + 1, (1,)).item()) for _ in range(18)]
        assert got.dtype == np.int32 and got.shape == (9, 2) and got.reshape(-1).tolist() == want        # top, left, top, left ...
        assert got.min() >= 0 and got.max() <= 2 * pad
    gen = torch.Generator().manual_seed(5)
    a = data_transforms.strong_inference_offsets(4, 10, generator=gen)
    gen.manual_seed(5)
    assert np.array_equal(a, data_transforms.strong_inference_offsets(4, 10, generator=gen))
    big = data_transforms.strong_inference_offsets(400, 10, generator=gen)
    assert big.min() == 0 and big.max() == 20                            # both ends of [0, 2 pad] are drawn
    assert not data_transforms.strong_inference_offsets(5, 0).any() and data_transforms.strong_inference_offsets(0).shape == (0, 2)
    nump = data_transforms.strong_inference_offsets(50, 3, generator=np.random.default_rng(1))
    assert nump.dtype == np.int32 and nump.min() >= 0 and nump.max() <= 6
    with pytest.raises(ValueError):
        data_transforms.strong_inference_offsets(3, -1)


# ---------------------------------------------------------------------------------------------- 3. the attribute table and distance
def test_get_attributes_equals_the_references_table(fx, mat_path):
    table = tricks.get_attributes(mat_path)
    assert sorted(table) == fx["ids"].tolist()
    for k, identity in enumerate(fx["ids"]):
        assert table[int(identity)].shape == (30,) and np.array_equal(table[int(identity)], fx["table"][k])
    assert (fx["table"][:, :4].sum(1) == 1).all()                        # the age one-hot
    rows = tricks.attribute_rows(fx["labels"], mat_path)
    for lab, row in zip(fx["labels"], rows):
        if int(lab) in table:
            assert np.array_equal(row, table[int(lab)].astype(np.float32))
        else:
            assert int(lab) in (0, -1, 999, 3) and (row == 1).all()      # 0, -1, an unknown id, an id of the second field: ones
    assert {0, -1, 999, 3} <= set(fx["labels"].tolist())


def test_the_references_distance_passes_the_bound_and_mutations_fail_it(fx, mat_path):
    """The reference's own recorded matrix lies inside the squared-domain bound, no element left out - its identical rows give 1e-6 or a
    few 1e-4 -, and so does a plain fp32 evaluation; without the clamp, or with alpha = -1, it does not."""
    a = tricks.normalize_rows(tricks.attribute_rows(fx["labels"], mat_path))
    lo, hi = ref.dist_bounds(a)
    assert ref.inside(fx["dist"], lo, hi).all()
    same = (np.asarray(a)[:, None, :] == np.asarray(a)[None, :, :]).all(2)
    assert same.sum() > len(a) and fx["dist"][same].max() < 1e-3 and fx["dist"][same].min() >= 1e-6 * (1 - 1e-6)
    assert ref.inside(ref.euclid32(a), lo, hi).all()
    assert not ref.inside(ref.euclid32(a, clamp=False), lo, hi).all()
    assert not ref.inside(ref.euclid32(a, alpha=-1.0), lo, hi).all()
    for n, d in ((5, 1), (70, 30), (66, 32)):
        rows = ref.attribute_like_rows(n, d, n + d)
        lo, hi = ref.dist_bounds(rows)
        assert ref.inside(ref.euclid32(rows), lo, hi).all() and not ref.inside(ref.euclid32(rows, clamp=False), lo, hi).all()


# ---------------------------------------------------------------------------------------------- 4. library, symbols, keywords
def test_eval_links_library_kernels_match_their_list(built, golden_dir):
    """The two kernels live in a library of their own that libreid_hip.so opens from its own directory on the first call that needs it:
    the kernel list equals tests/golden/kernels_eval_links.json by name, no kernel has scratch, the product library does not name the
    file among what it needs, and it loads on its own."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import so_kernels
    rows = so_kernels.kernels(LIB)
    names = sorted(rows)
    got = {so_kernels.short(d): rows[n] for d, n in zip(so_kernels.demangle(names), names)}
    want = json.load(open(os.path.join(golden_dir, "kernels_eval_links.json")))["kernels"]
    assert sorted(got) == sorted(want), {"new": sorted(set(got) - set(want)), "gone": sorted(set(want) - set(got))}
    assert sorted(got) == ["dist_add_l2_kernel", "shift_mirror_nchw_kernel"]
    assert all(v["scratch"] == 0 for v in got.values()) and not any(want.values()), {k: v["scratch"] for k, v in got.items()}
    needed = subprocess.run(["readelf", "-d", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "NEEDED" in needed and "libreid_hip_eval_links" not in needed
    own = subprocess.run(["readelf", "-d", LIB], capture_output=True, text=True, check=True).stdout
    assert "libreid_hip.so" not in own
    lib = ctypes.CDLL(LIB)
    for sym in ("eval_links_shift_mirror", "eval_links_dist_add_l2", "eval_links_grid_cap", "eval_links_tile", "eval_links_max_d"):
        assert hasattr(lib, sym)
    assert (lib.eval_links_grid_cap(), lib.eval_links_tile(), lib.eval_links_max_d()) == (4096, 64, 32)


def test_the_entries_are_declared_bound_and_exported(built):
    hdr = open(os.path.join(ROOT, "include", "reid_hip.h")).read()
    dbg_hdr = open(os.path.join(ROOT, "include", "reid_hip_debug.h")).read()
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for sym in ENTRIES:
        assert sym + "(" in hdr and sym in _ffi.EXPORTS and sym in _ffi._SIGS and hasattr(lib, sym)
    for cite in ("reid/data_transforms.py:130-191", "reid/image_reid_inference.py:276-289", "reid/losses/utils.py:21-35"):
        assert cite in hdr
    for sym in HARNESSES:
        assert sym + "(" in dbg_hdr and sym in _ffi.DEBUG_EXPORTS and hasattr(_ffi.debug_lib(), sym)
    for name in ("descriptor_f32_nchw_shift", "descriptor_shift_dev", "descriptor_images_u8_shift", "distmat_add_l2", "distmat_add_l2_dev",
                 "normalised_zero_fill", "debug_shift_mirror", "debug_dist_add_l2"):
        assert callable(getattr(Engine, name))


class _NoDevice:
    """Stands where an Engine would: any attribute a device call needs raises, so a check that lets a bad argument through fails."""
    swin_dim, swin_num_class, embed_dim, num_class = 96, 751, 512, 751
    _swin_crop_args = staticmethod(Engine._swin_crop_args)
    _pack_ragged = staticmethod(Engine._pack_ragged)

    def __getattr__(self, name):
        raise AssertionError("reached the engine: " + name)


def test_keyword_rules_raise_before_any_device_call():
    eng = _NoDevice()
    x = np.zeros((2, 3, 256, 128), np.float32)
    xs = np.zeros((2, 3, 448, 224), np.float32)
    lab = np.zeros(2, np.int64)
    ok = np.full((4, 2), 10, np.int32)
    # the Swin takes the plain mirror
    with pytest.raises(ValueError, match="swin"):
        reid_inference.evaluate_reid(xs, lab, lab, lab, xs, lab, lab, lab, engine=eng, arch="swin", strong_inference=True)
    with pytest.raises(ValueError, match="swin"):
        reid_inference.evaluate_reid(xs, lab, lab, lab, xs, lab, lab, lab, engine=eng, arch="swin", strong_offsets=ok)
    with pytest.raises(ValueError, match="swin"):
        reid_inference.inference_efficient(eng, xs, 1, arch="swin", strong_offsets=ok[:2])
    # a bad shift names the image, a bad pad its range
    bad = ok.copy()
    bad[3, 1] = 21
    with pytest.raises(ValueError, match="image 3.*left 21"):
        reid_inference.evaluate_reid(x, lab, lab, lab, x, lab, lab, lab, engine=eng, strong_offsets=bad)
    with pytest.raises(ValueError, match="image 1.*top -1"):
        reid_inference.inference_efficient(eng, x, 1, strong_offsets=[[0, 0], [-1, 0]])
    with pytest.raises(ValueError, match="pad"):
        reid_inference.evaluate_reid(x, lab, lab, lab, x, lab, lab, lab, engine=eng, strong_inference=True, pad=33)
    with pytest.raises(ValueError, match="pad"):
        reid_inference.inference_efficient(eng, x, 1, strong_offsets=ok[:2], pad=-1)
    with pytest.raises(ValueError, match=r"\[n, 2\]"):
        reid_inference.inference_efficient(eng, x, 1, strong_offsets=ok)             # 4 shifts for 2 images
    with pytest.raises(ValueError, match="flip"):
        reid_inference.inference_efficient(eng, x, 1, flip=False, strong_offsets=ok[:2])
    with pytest.raises(ValueError, match="image 0"):
        inference_utils.extract_descriptors(x, strong_offsets=[[30, 0], [0, 0]])
    with pytest.raises(ValueError, match="pad"):
        Engine.descriptor_f32_nchw_shift(eng, x, ok[:2], pad=40)
    with pytest.raises(ValueError, match="image 1"):
        Engine.descriptor_images_u8_shift(eng, [np.zeros((4, 4, 3), np.uint8)] * 2, [[0, 0], [0, 3]], pad=1)
    # the attribute rows: one per image, 1 .. 32 wide
    with pytest.raises(ValueError, match="attribute_dist"):
        reid_inference.evaluate_reid(x, lab, lab, lab, x, lab, lab, lab, engine=eng, attribute_dist=np.ones((3, 30)))
    with pytest.raises(ValueError, match="attribute_dist"):
        reid_inference.evaluate_reid(x, lab, lab, lab, x, lab, lab, lab, engine=eng, attribute_dist=np.ones((4, 33)))
    with pytest.raises(ValueError):
        Engine.distmat_add_l2(eng, np.ones((3, 30), np.float32), np.zeros((3, 4), np.float32))
