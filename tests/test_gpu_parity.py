"""GPU parity tests: the HIP path (through the C ABI) against the oracle and the committed golden
fixtures (which came from the reference's own modules).  Run on an MI355X: pytest -m gpu."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import matching, seres18
from reid_amd import _ffi, synth, weights

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from reid_amd.engine import get_engine
    return get_engine(0)


@pytest.fixture()
def eng_w0(eng):
    sd = synth.seres18_state_dict(0)
    blob, manifest, _ = weights.pack_seres18(sd)
    eng.load_seres18(blob, manifest)
    return eng, sd


# ----------------------------------------------------------------------------- single operators
@pytest.mark.parametrize("m,n,k", [(128, 128, 32), (1, 751, 512), (130, 70, 96), (257, 129, 36), (5, 3, 1263)])
def test_gemm_nt(eng, m, n, k):
    rng = np.random.default_rng(m * 1000 + n)
    a = rng.normal(size=(m, k)).astype(np.float32)
    b = rng.normal(size=(n, k)).astype(np.float32)
    bias = rng.normal(size=n).astype(np.float32)
    got = eng.gemm_nt(a, b, bias)
    ref = (a.astype(np.float64) @ b.astype(np.float64).T + bias).astype(np.float32)
    # fp32 MFMA = k-ordered fmaf chain: error ~1e-7 * sum|a.b|
    np.testing.assert_allclose(got, ref, rtol=1e-5, atol=2e-5 * np.sqrt(k))


@pytest.mark.parametrize("cfg", [
    dict(n=2, h=16, w=8, cin=64, cout=64, k=3, stride=1, pad=1),
    dict(n=3, h=32, w=16, cin=64, cout=128, k=3, stride=2, pad=1),
    dict(n=2, h=32, w=16, cin=64, cout=128, k=1, stride=2, pad=0),
    dict(n=1, h=16, w=8, cin=256, cout=512, k=3, stride=1, pad=1),
    dict(n=2, h=8, w=8, cin=32, cout=96, k=3, stride=1, pad=1),
])
def test_conv2d_nhwc(eng, cfg):
    rng = np.random.default_rng(cfg["cin"] + cfg["cout"])
    n, h, w, cin, cout, k = cfg["n"], cfg["h"], cfg["w"], cfg["cin"], cfg["cout"], cfg["k"]
    x = rng.normal(size=(n, h, w, cin)).astype(np.float32)
    wt = (rng.normal(size=(cout, cin, k, k)) / np.sqrt(cin * k * k)).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, cout).astype(np.float32)
    shift = rng.normal(size=cout).astype(np.float32)
    ref = F.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2), torch.from_numpy(wt), None, cfg["stride"], cfg["pad"])
    res = rng.normal(size=tuple(ref.permute(0, 2, 3, 1).shape)).astype(np.float32)
    ref2 = F.relu(ref * torch.from_numpy(scale)[None, :, None, None] + torch.from_numpy(shift)[None, :, None, None]
                  + torch.from_numpy(res).permute(0, 3, 1, 2))
    w_krsc = np.ascontiguousarray(wt.transpose(0, 2, 3, 1))
    got = eng.conv2d_nhwc(x, w_krsc, cfg["stride"], cfg["pad"])
    np.testing.assert_allclose(got, ref.permute(0, 2, 3, 1).numpy(), rtol=1e-4, atol=1e-4)
    got2 = eng.conv2d_nhwc(x, w_krsc, cfg["stride"], cfg["pad"], scale, shift, res, relu=True)
    np.testing.assert_allclose(got2, ref2.permute(0, 2, 3, 1).numpy(), rtol=1e-4, atol=1e-4)


# ----------------------------------------------------------------------------- embedding
@pytest.mark.parametrize("precision", [0, 2])
@pytest.mark.parametrize("tag,crops_fn", [("seed0", synth.crops_u8), ("smooth1", synth.smooth_crops_u8)])
def test_seres18_embed_matches_reference_fixture(eng, golden_dir, tag, crops_fn, precision):
    """Eval-mode semantics.  Tolerance: north_star 1e-3 cosine; the fp32 MFMA path is held to 1e-5 - and so is
    precision 2, the "fp32-class" mode (3x3 stride-1 convolutions as three f16 products per multiply with hi/lo-split operands
    and fp32 accumulation on the f16 matrix pipe; everything else is the exact-fp32 path): same thresholds, stage by stage."""
    eng.set_precision(precision)
    try:
        _seres18_fixture_check(eng, golden_dir, tag, crops_fn, precision)
    finally:
        eng.set_precision(0)


def _seres18_fixture_check(eng, golden_dir, tag, crops_fn, precision=0):
    g = np.load(os.path.join(golden_dir, "seres18_%s.npz" % tag))
    seed, n = int(g["seed"]), int(g["n"])
    sd = synth.seres18_state_dict(seed)
    blob, manifest, info = weights.pack_seres18(sd)
    eng.load_seres18(blob, manifest)
    assert info["num_class"] == 751
    crops = crops_fn(n, seed)
    eng.debug_keep(True)
    try:
        emb, logits = eng.embed_u8(crops, logits=True)
        taps = {}
        ref_emb, ref_logits = seres18.forward(sd, seres18.preprocess_u8(crops), taps)
        names = ["stem", "pool0"] + [b[0] for b in synth.SERES18_BLOCKS] + ["gem"]
        for s, name in enumerate(names):
            t = taps[name]
            want = t.permute(0, 2, 3, 1).contiguous().numpy().reshape(-1) if t.dim() == 4 else t.numpy().reshape(-1)
            got = eng.debug_stage(s, n)
            err = np.abs(got - want).max() / max(1e-6, np.abs(want).max())
            assert err < 2e-5, "stage %d (%s): rel max err %g" % (s, name, err)
        # debug_keep 2: the production kernels (stem with the max-pool on its accumulators - in precision 2 the split stem of
        # stem_split.hip, from uint8 and from fp32 input), every stage but the conv map itself
        eng.debug_keep(2)
        for entry in ("u8", "f32"):
            emb_p = eng.embed_u8(crops) if entry == "u8" else eng.embed_f32_nchw(seres18.preprocess_u8(crops).numpy())
            for s, name in enumerate(names):
                if s == 0:
                    continue
                t = taps[name]
                want = t.permute(0, 2, 3, 1).contiguous().numpy().reshape(-1) if t.dim() == 4 else t.numpy().reshape(-1)
                err = np.abs(eng.debug_stage(s, n) - want).max() / max(1e-6, np.abs(want).max())
                assert err < 2e-5, "production kernels, %s entry, stage %d (%s): rel max err %g" % (entry, s, name, err)
            assert np.abs(emb_p - g["emb"]).max() / np.abs(g["emb"]).max() < 5e-5
    finally:
        eng.debug_keep(False)
    for mine, ref in ((emb, g["emb"]), (emb, ref_emb.numpy()), (logits, g["logits"])):
        assert np.abs(mine - ref).max() / np.abs(ref).max() < 5e-5
    cos = (emb * g["emb"]).sum(1) / np.linalg.norm(emb, axis=1) / np.linalg.norm(g["emb"], axis=1)
    assert (1 - cos).max() < 1e-5
    # N=1 and the float NCHW entry of the plugin surface give the same embedding
    emb1 = eng.embed_u8(crops[:1])
    np.testing.assert_allclose(emb1, g["emb_single0"], rtol=1e-4, atol=2e-4 * np.abs(g["emb"]).max())
    embf = eng.embed_f32_nchw(seres18.preprocess_u8(crops).numpy())
    # precision 2: the uint8 entry convolves the exact integers 2 v - 255, the fp32 entry the hi/lo split of the normalised values
    np.testing.assert_allclose(embf, emb, rtol=1e-6, atol=(5e-6 if precision == 2 else 1e-6) * np.abs(emb).max())
    # rebatching does not change results beyond fp32 noise (chunked passes)
    eng.set_chunk(2)
    emb_c = eng.embed_u8(crops)
    eng.set_chunk(1024)
    np.testing.assert_allclose(emb_c, emb, rtol=1e-6, atol=1e-6 * np.abs(emb).max())


@pytest.mark.parametrize("form", [1, 2, 3])
@pytest.mark.parametrize("tag,crops_fn", [("seed0", synth.crops_u8), ("smooth1", synth.smooth_crops_u8)])
def test_two_blocks_per_cu_convolution_matches_reference_fixture(eng, golden_dir, tag, crops_fn, form):
    """csrc/conv3x3_x3.hip - the fp32-class 3x3 convolution of LARGE launches (4-wave blocks, several per CU; form 3, the default: on
    v_mfma_f32_16x16x32_f16 with 64-byte-row LDS images, two blocks per CU for the 128-wide tiles and four - one halo buffer - for
    layer 1's 64-wide ones; form 2 = the 128-wide tiles only; form 1 on 32x32x16) - forced onto the fixture's small batch (debug switch split_x3_min_blocks = 1), against the
    REFERENCE's stage taps, embeddings and logits at the exact-fp32 mode's thresholds (SERes18_IBN.py:120-128,250-276); the
    full-size configs[1] test runs it at its own launch sizes.  Another summation order than conv3x3_f16.hip's (per 32-channel
    chunk: xh.wh 2^11, xh.wl', xl'.wh), the same three products."""
    eng.set_precision(2)
    eng.debug_switch("split_x3_min_blocks", 1)
    eng.debug_switch("split_x3", form)
    try:
        _seres18_fixture_check(eng, golden_dir, tag, crops_fn, 2)
        # ragged and odd batches: a last 256-row tile of 128 rows (odd image counts in the 8-wide maps), single images
        sd = synth.seres18_state_dict(0)
        eng.load_seres18(*weights.pack_seres18(sd)[:2])
        crops = synth.smooth_crops_u8(7, 11)
        got = eng.embed_u8(crops)
        eng.debug_switch("split_x3", 0)
        want = eng.embed_u8(crops)
        assert not np.array_equal(got, want) and np.abs(got - want).max() <= 5e-6 * np.abs(want).max()
        eng.debug_switch("split_x3", form)
        assert np.array_equal(eng.embed_u8(crops[:1]), got[:1]) and np.array_equal(eng.embed_u8(crops[2:5]), got[2:5])   # images are independent
    finally:
        eng.debug_switch("split_x3", 3)
        eng.debug_switch("split_x3_min_blocks", 512)
        eng.set_precision(0)


def test_unrolled_and_looped_two_blocks_per_cu_kernels_agree_bit_for_bit(eng):
    """conv3x3_x3.hip: conv3x3_x3u_kernel (a chunk's 27 steps unrolled, buffer descriptors: the default) and conv3x3_x3m16_kernel (run-time
    step loop: what a pass takes whose input passes the 2-GB range of a descriptor, e.g. 4096 crops in ONE pass) run the same tiles in the
    same order through the same epilogue: identical embeddings at the launch sizes of a 1024-crop pass (debug switch x3_unroll)."""
    eng.load_seres18(*weights.pack_seres18(synth.seres18_state_dict(0))[:2])
    crops = synth.crops_u8(1024, 5)
    try:
        eng.set_precision(2)
        eng.set_chunk(1024)
        unrolled = eng.embed_u8(crops)
        eng.debug_switch("x3_unroll", 0)
        looped = eng.embed_u8(crops)
    finally:
        eng.debug_switch("x3_unroll", 3)
        eng.set_precision(0)
    assert np.isfinite(unrolled).all() and np.array_equal(unrolled, looped)


def test_fused_stem_pool_is_the_same_for_whole_images_and_strips(eng_w0):
    """stem_f32.hip with the max-pool on its accumulators: 520 crops in one pass (a block walks a whole image) and in chunks of
    260 (32-tile strips, each recomputing the tile above it) run the same arithmetic per pixel - bit-identical embeddings.
    (Chunks small enough for the split-K convolutions - a tracking frame - sum their K-tiles in another order: fp32 noise.)"""
    eng, _ = eng_w0
    crops = synth.smooth_crops_u8(520, seed=8)
    eng.set_chunk(1024)
    whole = eng.embed_u8(crops)
    eng.set_chunk(260)
    strips = eng.embed_u8(crops)
    eng.set_chunk(40)
    small = eng.embed_u8(crops)
    eng.set_chunk(1024)
    assert np.array_equal(whole, strips)
    cos = (whole * small).sum(1) / np.linalg.norm(whole, axis=1) / np.linalg.norm(small, axis=1)
    assert (1 - cos).max() < 1e-6 and np.abs(whole - small).max() < 1e-5 * np.abs(whole).max()


def test_embed_ragged_resize_matches_oracle(eng_w0):
    eng, sd = eng_w0
    crops = synth.ragged_crops_u8(6, seed=3) + [synth.crops_u8(1, 9)[0]]
    emb = eng.embed_ragged_u8(crops)
    x = matching.preprocess(crops)                      # oracle restatement of feature_extractor.py:31-46
    ref, _ = seres18.forward(sd, torch.from_numpy(x))
    ref = ref.numpy()
    assert np.abs(emb - ref).max() / np.abs(ref).max() < 5e-5
    assert eng.embed_ragged_u8([]).shape == (0, 512)    # empty input


def test_embed_rank_parity_and_cosine_distmat(eng_w0):
    """BASELINE config 1 shape: 64 crops -> 512-d -> cosine distmat; argmin ranks equal to the oracle's."""
    eng, sd = eng_w0
    crops = synth.smooth_crops_u8(64, seed=5)
    emb = eng.embed_u8(crops)
    ref = seres18.embed_u8(sd, crops)
    cos = (emb * ref).sum(1) / np.linalg.norm(emb, axis=1) / np.linalg.norm(ref, axis=1)
    assert (1 - cos).max() < 1e-5
    d_gpu = eng.distmat(emb, emb, _ffi.METRIC_COS)
    d_ref = matching.cosine_dist_deepsort(ref, ref)
    np.testing.assert_allclose(d_gpu, d_ref, atol=2e-5)
    np.fill_diagonal(d_gpu, np.inf)
    np.fill_diagonal(d_ref, np.inf)
    srt = np.sort(d_ref, axis=1)
    decided = (srt[:, 1] - srt[:, 0]) > 1e-5           # near-ties are not deterministic in the reference either
    assert decided.sum() >= 48
    assert (d_gpu.argmin(1)[decided] == d_ref.argmin(1)[decided]).all()


# ----------------------------------------------------------------------------- matching
def test_distances_match_reference_fixture(eng, golden_dir):
    g = np.load(os.path.join(golden_dir, "matching.npz"))
    x, y = g["x"], g["y"]
    np.testing.assert_allclose(eng.distmat(x, y, _ffi.METRIC_L2), g["euclid"], rtol=1e-5, atol=5e-4)
    mask = g["euclid"] > 0.1                            # away from the clamp(1e-12).sqrt() cancellation point
    np.testing.assert_allclose(eng.distmat(x, y, _ffi.METRIC_L2)[mask], g["euclid"][mask], rtol=1e-5, atol=2e-5)
    np.testing.assert_allclose(eng.distmat(x, y, _ffi.METRIC_COS_HALF), g["cosine"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(eng.distmat(x, y, _ffi.METRIC_COS), 2 * g["cosine"], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(eng.distmat(x, y, _ffi.METRIC_DOT), x @ y.T, rtol=1e-5, atol=1e-5)
    idx, val = eng.argmin_rows(x, y, _ffi.METRIC_L2)
    np.testing.assert_array_equal(idx, g["euclid"].argmin(1))
    np.testing.assert_allclose(val, g["euclid"].min(1), rtol=1e-5, atol=5e-4)


@pytest.mark.parametrize("m,n,d", [(1, 1, 4), (3, 1000, 96), (300, 257, 512), (17, 33, 1263)])
def test_distmat_shapes(eng, m, n, d):
    rng = np.random.default_rng(d)
    x = rng.normal(size=(m, d)).astype(np.float32)
    y = rng.normal(size=(n, d)).astype(np.float32)
    np.testing.assert_allclose(eng.distmat(x, y, _ffi.METRIC_L2), matching.euclidean_dist(x, y), rtol=2e-5, atol=1e-4)
    np.testing.assert_allclose(eng.distmat(x, y, _ffi.METRIC_COS_HALF), matching.cosine_dist(x, y), rtol=1e-5, atol=2e-6)
    assert eng.distmat(x[:0], y).shape == (0, n)        # empty inputs


@pytest.mark.parametrize("m,n,d", [(300, 257, 512), (129, 1000, 96), (640, 384, 2048)])
def test_distance_matrix_on_k16_tiles_equals_k32_tiles(eng, m, n, d):
    """gemm_f32_dma.hip: the 128-wide distance tile with K-tiles of 16 (four blocks per CU, the default since round 5) runs the MFMAs of an
    output element in the order of the K-tiles-of-32 form: bit-identical matrices, ragged edges included; both against the oracle."""
    rng = np.random.default_rng(m + n)
    x = rng.normal(size=(m, d)).astype(np.float32)
    y = rng.normal(size=(n, d)).astype(np.float32)
    try:
        eng.debug_switch("f32_dist_bk16", 0)
        want = eng.distmat(x, y, _ffi.METRIC_L2)
        want_cos = eng.distmat(x, y, _ffi.METRIC_COS_HALF)
        eng.debug_switch("f32_dist_bk16", 1)
        got = eng.distmat(x, y, _ffi.METRIC_L2)
        got_cos = eng.distmat(x, y, _ffi.METRIC_COS_HALF)
    finally:
        eng.debug_switch("f32_dist_bk16", 1)
    assert np.array_equal(got, want) and np.array_equal(got_cos, want_cos)
    np.testing.assert_allclose(got, matching.euclidean_dist(x, y), rtol=2e-5, atol=2e-4)


def test_knn_matches_oracle(eng):
    rng = np.random.default_rng(2)
    xb = rng.normal(size=(700, 64)).astype(np.float32)
    xq = np.concatenate([xb[:40] + 0.05 * rng.normal(size=(40, 64)).astype(np.float32), xb[:3]], 0)
    D, I = eng.knn(xq, xb, 20)
    Dr, Ir = matching.knn_l2sqr(xq, xb, 20)
    assert (np.diff(D, axis=1) >= 0).all()
    np.testing.assert_allclose(D, Dr, rtol=1e-4, atol=2e-4)
    gap = np.abs(np.diff(Dr, axis=1)).min(1) > 1e-3     # rows whose 20 neighbours are well separated
    assert gap.sum() > 20
    np.testing.assert_array_equal(I[gap], Ir[gap])
    assert (I[:, 0] == np.r_[np.arange(40), np.arange(3)]).all()


def test_knn_when_one_thread_holds_the_whole_top_k(eng):
    """topk_rows_kernel keeps four candidates per thread; gallery rows 7, 263, 519, ... (the elements one thread visits) are
    made the nearest neighbours of every query, so that thread's list runs dry and the row takes the exact fallback: the answer
    must not change.  Also k larger than the gallery (padding with inf / -1)."""
    rng = np.random.default_rng(9)
    xb = rng.normal(size=(3000, 32)).astype(np.float32) + 4.0
    xq = rng.normal(size=(6, 32)).astype(np.float32) * 0.01
    near = np.arange(7, 3000, 256)                      # 12 rows, all visited by thread 7 of a 256-thread block
    xb[near] = 0.001 * np.arange(1, len(near) + 1, dtype=np.float32)[:, None]
    D, I = eng.knn(xq, xb, 10)
    Dr, Ir = matching.knn_l2sqr(xq, xb, 10)
    np.testing.assert_array_equal(I, Ir)
    np.testing.assert_allclose(D, Dr, rtol=1e-4, atol=1e-5)
    assert set(I[0].tolist()) <= set(near.tolist())
    D2, I2 = eng.knn(xq, xb[:5], 8)
    assert (I2[:, 5:] == -1).all() and np.isinf(D2[:, 5:]).all() and (np.sort(I2[:, :5], 1) == np.arange(5)).all()


def test_diou_bit_exact(eng, golden_dir):
    g = np.load(os.path.join(golden_dir, "matching.npz"))
    demo = eng.diou([10, 12, 8, 9], [[9, 10, 9, 9], [8, 12, 9, 10], [10, 12, 9, 8]])
    np.testing.assert_array_equal(demo, g["diou_demo"])          # the reference file's own demo (iou_matching.py:50-53)
    got = np.stack([eng.diou(b, g["diou_cands"]) for b in g["diou_boxes"]], 0)
    np.testing.assert_array_equal(got, g["diou"])                # fp64, bit-exact
    np.testing.assert_array_equal(eng.diou_cost(g["diou_boxes"], g["diou_cands"]), 1.0 - g["diou"])
    assert eng.diou_cost(np.zeros((0, 4)), g["diou_cands"]).shape == (0, 31)


def test_rank_eval_matches_reference_fixture(eng, golden_dir):
    from reid_amd.evaluate import evaluate_all
    g = np.load(os.path.join(golden_dir, "matching.npz"))
    cmc, ap = evaluate_all(g["ev_qf"], g["ev_ql"], g["ev_qc"], g["ev_gf"], g["ev_gl"], g["ev_gc"], verbose=False)
    np.testing.assert_array_equal(np.asarray(cmc), g["ev_cmc"])  # integer rank counting: exact
    assert abs(ap - float(g["ev_map"])) < 1e-12


def test_rank_eval_market_shape(eng):
    """Config-5 shaped problem at reduced size against the oracle."""
    from reid_amd.evaluate import evaluate_all
    qf, ql, qc, gf, gl, gc = synth.clustered_embeddings(200, 3000, d=512, n_ids=120, seed=4)
    cmc, ap = evaluate_all(qf, ql, qc, gf, gl, gc, verbose=False)
    cmc_r, ap_r = matching.evaluate_all(qf, ql, qc, gf, gl, gc)
    np.testing.assert_array_equal(np.asarray(cmc), cmc_r)
    assert abs(ap - ap_r) < 1e-10


# ----------------------------------------------------------------------------- fp16-storage fast path
@pytest.mark.parametrize("tag,crops_fn", [("seed0", synth.crops_u8), ("smooth1", synth.smooth_crops_u8)])
def test_seres18_f16_path_within_north_star_tolerance(eng, golden_dir, tag, crops_fn):
    """precision=1: fp16 activations/weights, fp32 accumulation (v_mfma_f32_32x32x16_f16).  north_star tolerance:
    1e-3 cosine against the reference; measured here at < 2e-5 and asserted at 1e-4."""
    g = np.load(os.path.join(golden_dir, "seres18_%s.npz" % tag))
    seed, n = int(g["seed"]), int(g["n"])
    sd = synth.seres18_state_dict(seed)
    blob, manifest, _ = weights.pack_seres18(sd)
    eng.load_seres18(blob, manifest)
    crops = crops_fn(n, seed)
    eng.set_precision(1)
    eng.debug_keep(True)
    try:
        emb, logits = eng.embed_u8(crops, logits=True)
        taps = {}
        seres18.forward(sd, seres18.preprocess_u8(crops), taps)
        names = ["stem", "pool0"] + [b[0] for b in synth.SERES18_BLOCKS] + ["gem"]
        for s, name in enumerate(names):
            t = taps[name]
            want = t.permute(0, 2, 3, 1).contiguous().numpy().reshape(-1) if t.dim() == 4 else t.numpy().reshape(-1)
            got = eng.debug_stage(s, n)
            err = np.abs(got - want).max() / max(1e-6, np.abs(want).max())
            assert err < 1e-2, "f16 stage %d (%s): rel max err %g" % (s, name, err)
        embf = eng.embed_f32_nchw(seres18.preprocess_u8(crops).numpy())
        emb_r = eng.embed_ragged_u8(list(crops))
    finally:
        eng.debug_keep(False)
        eng.set_precision(0)
    cos = (emb * g["emb"]).sum(1) / np.linalg.norm(emb, axis=1) / np.linalg.norm(g["emb"], axis=1)
    assert (1 - cos).max() < 1e-4
    assert np.abs(emb - g["emb"]).max() / np.abs(g["emb"]).max() < 1e-2
    assert np.abs(logits - g["logits"]).max() / np.abs(g["logits"]).max() < 1e-2
    np.testing.assert_allclose(embf, emb, rtol=0, atol=2e-3 * np.abs(emb).max())
    np.testing.assert_allclose(emb_r, emb, rtol=0, atol=2e-3 * np.abs(emb).max())


def test_f16_path_rank_parity(eng_w0):
    eng, sd = eng_w0
    crops = synth.smooth_crops_u8(64, seed=5)
    ref = seres18.embed_u8(sd, crops)
    eng.set_precision(1)
    try:
        emb = eng.embed_u8(crops)
    finally:
        eng.set_precision(0)
    cos = (emb * ref).sum(1) / np.linalg.norm(emb, axis=1) / np.linalg.norm(ref, axis=1)
    assert (1 - cos).max() < 1e-4
    d_gpu = eng.distmat(emb, emb, _ffi.METRIC_COS)
    d_ref = matching.cosine_dist_deepsort(ref, ref)
    np.fill_diagonal(d_gpu, np.inf)
    np.fill_diagonal(d_ref, np.inf)
    srt = np.sort(d_ref, axis=1)
    decided = (srt[:, 1] - srt[:, 0]) > 2e-3           # fp16 storage: ranks are asserted where the gap exceeds its noise
    assert decided.sum() >= 32
    assert (d_gpu.argmin(1)[decided] == d_ref.argmin(1)[decided]).all()


# ----------------------------------------------------------------------------- Swin-T (v1)
@pytest.mark.parametrize("precision", [0, 2])
def test_swin_embed_matches_reference_fixture(eng, golden_dir, precision):
    """224x224, N=2 (Q14), eval mode.  Tolerance: 1e-3 cosine (north_star); the fp32 path and the fp32-class mode
    (precision 2: every Linear / conv of the trunk as three f16 matrix-core products on hi/lo-split operands) held to 1e-5."""
    from oracle import swin
    g = np.load(os.path.join(golden_dir, "swin_seed0.npz"))
    seed, n = int(g["seed"]), int(g["n"])
    sd = synth.swin_state_dict(seed)
    blob, manifest, info = weights.pack_swin(sd)
    eng.load_swin(blob, manifest)
    x = synth.images_f32(n, seed)
    eng.set_precision(precision)
    try:
        _swin_fixture_checks(eng, g, sd, x, swin)
    finally:
        eng.set_precision(0)


def _swin_fixture_checks(eng, g, sd, x, swin):
    emb, logits = eng.swin_embed_f32_nchw(x, logits=True)
    ref_emb, ref_logits = swin.forward(sd, torch.from_numpy(x))
    for mine, ref in ((emb, g["emb"]), (emb, ref_emb.numpy()), (logits, g["logits"])):
        assert np.abs(mine - ref).max() / np.abs(ref).max() < 2e-4
    cos = (emb * g["emb"]).sum(1) / np.linalg.norm(emb, axis=1) / np.linalg.norm(g["emb"], axis=1)
    assert (1 - cos).max() < 1e-5
    # N = 1 works here although the reference breaks on it; 448x224 is accepted as in the reference
    emb1 = eng.swin_embed_f32_nchw(x[:1])
    np.testing.assert_allclose(emb1, emb[:1], rtol=1e-4, atol=1e-4 * np.abs(emb).max())
    x2 = synth.images_f32(1, 3, h=448, w=224)
    e2 = eng.swin_embed_f32_nchw(x2)
    r2, _ = swin.forward(sd, torch.from_numpy(x2))
    assert np.abs(e2 - r2.numpy()).max() / np.abs(r2.numpy()).max() < 2e-4


def test_swin_f16_storage_mode_within_north_star_tolerance(eng, golden_dir):
    """precision=1 for Swin: the five linears of every block run on the f16 MFMA GEMM (fp32 accumulate) from f16 LayerNorm /
    attention / GELU outputs; LayerNorm, softmax and the residual stream stay fp32.  north_star tolerance 1e-3 cosine against
    the reference; asserted at 1e-4.  Odd batch sizes exercise the ragged last M tile (49 tokens per image in stage 4)."""
    g = np.load(os.path.join(golden_dir, "swin_seed0.npz"))
    seed, n = int(g["seed"]), int(g["n"])
    sd = synth.swin_state_dict(seed)
    blob, manifest, _ = weights.pack_swin(sd)
    eng.load_swin(blob, manifest)
    x = synth.images_f32(n, seed)
    x5 = synth.images_f32(5, seed + 1)
    ref5 = eng.swin_embed_f32_nchw(x5)
    eng.set_precision(1)
    try:
        emb, logits = eng.swin_embed_f32_nchw(x, logits=True)
        emb5 = eng.swin_embed_f32_nchw(x5)
        emb1 = eng.swin_embed_f32_nchw(x5[:1])
    finally:
        eng.set_precision(0)
    cos = (emb * g["emb"]).sum(1) / np.linalg.norm(emb, axis=1) / np.linalg.norm(g["emb"], axis=1)
    assert (1 - cos).max() < 1e-4
    assert np.abs(emb - g["emb"]).max() / np.abs(g["emb"]).max() < 1e-2
    assert np.abs(logits - g["logits"]).max() / np.abs(g["logits"]).max() < 1e-2
    cos5 = (emb5 * ref5).sum(1) / np.linalg.norm(emb5, axis=1) / np.linalg.norm(ref5, axis=1)
    assert (1 - cos5).max() < 1e-4
    assert np.array_equal(emb1, emb5[:1])          # images are independent: batch composition does not matter


def test_swin_backbone_object(eng):
    from reid_amd import models
    from oracle import swin
    m = models.build_model("swin_transformer", num_classes=751, loss="triplet", pretrained=False).eval()
    x = torch.from_numpy(synth.images_f32(3, 7))
    out = m(x)
    assert isinstance(out, torch.Tensor) and tuple(out.shape) == (3, 96)
    ref, _ = swin.forward(synth.swin_state_dict(0), x)
    assert np.abs(out.numpy() - ref.numpy()).max() / np.abs(ref.numpy()).max() < 2e-4


# ----------------------------------------------------------------------------- k-reciprocal re-ranking
@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_rerank_jaccard_matches_reference_fixture(eng, golden_dir, tag):
    """reid_rerank_jaccard against the reference's own compute_jaccard_distance output (tests/golden/rerank.npz), once
    from the reference's neighbour lists and once from the library's own k-NN."""
    z = np.load(os.path.join(golden_dir, "rerank.npz"))
    x, k1, k2 = z[f"{tag}_x"], int(z[f"{tag}_k"][0]), int(z[f"{tag}_k"][1])
    want = z[f"{tag}_jaccard"]
    got = eng.rerank_jaccard(x, k1, k2, rank=z[f"{tag}_rank"])
    # fp32 sums in a different order (softmax denominator, LDS-atomic min-sums): a few ulp of values in [0, 1]
    np.testing.assert_allclose(got, want, rtol=0, atol=3e-6)
    _, knn_i = eng.knn(x, x, k1)
    assert np.array_equal(knn_i, z[f"{tag}_rank"])          # no near-ties in these fixtures
    got2 = eng.rerank_jaccard(x, k1, k2)
    np.testing.assert_allclose(got2, want, rtol=0, atol=3e-6)
    assert (got >= 0).all() and (got <= 1).all()


def test_rerank_jaccard_oracle_sizes_and_host_mirror(eng):
    """Larger N (persistent blocks loop, several rows per block), D = 1263 as the reference's descriptor, default k1/k2,
    through the host mirror of reid/faiss_utils.py; checked against the oracle from the same neighbour lists."""
    from oracle import rerank
    from reid_amd import faiss_utils
    _, _, _, x, _, _ = synth.clustered_embeddings(1, 1500, d=1263, n_ids=40, n_cams=2, seed=31, sigma=0.8)
    _, rank = eng.knn(x, x, 20)
    got = faiss_utils.compute_jaccard_distance(torch.from_numpy(x), print_flag=False, initial_rank=rank)
    want = rerank.compute_jaccard_distance(x, 20, 6, initial_rank=rank)
    np.testing.assert_allclose(got, want, rtol=0, atol=3e-6)
    # properties: zero (up to rounding) on the diagonal of points that are their own nearest neighbour
    own = rank[:, 0] == np.arange(len(x))
    assert own.mean() > 0.99
    assert np.abs(np.diag(got)[own]).max() < 1e-5


def test_rerank_jaccard_argument_errors(eng):
    x = np.zeros((8, 4), np.float32)
    with pytest.raises(_ffi.ReidHipError):
        eng.rerank_jaccard(x, k1=9, k2=2)      # k1 > n
    with pytest.raises(_ffi.ReidHipError):
        eng.rerank_jaccard(x, k1=65, k2=2)     # k1 > 64


# ----------------------------------------------------------------------------- DeepSORT feature bank
@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_nn_matching_bank_follows_oracle_over_a_stream(eng, metric):
    """A 40-frame synthetic stream: tracks are born, updated (several samples per call, more than the budget over time)
    and dropped; after every frame the device cost matrix equals the oracle's, raw and gated."""
    from oracle import nn_matching as onm
    from reid_amd.nn_matching import NearestNeighborDistanceMetric
    rng = np.random.default_rng(5)
    d, budget = 512, 7
    ref = onm.NearestNeighborDistanceMetric(metric, 0.15, budget)
    dev = NearestNeighborDistanceMetric(metric, 0.15, budget, max_tracks=48)
    alive, next_id = [], 0
    for frame in range(40):
        for _ in range(rng.integers(0, 3)):                      # births
            alive.append(next_id)
            next_id += 1
        if alive and rng.random() < 0.6:                         # a death (its slot is reused later)
            alive.pop(rng.integers(len(alive)))
        feats, targets = [], []
        for t in alive:
            # 0..2 new samples per track per frame; a new track always brings one (DeepSORT only lists confirmed tracks,
            # which hold features - an active target without samples is a KeyError in the reference too)
            for _ in range(max(int(rng.integers(0, 3)), 0 if t in ref.samples else 1)):
                feats.append(rng.normal(0, 1, d).astype(np.float32) + 3.0 * np.sin(t + np.arange(d, dtype=np.float32)))
                targets.append(t)
        ref.partial_fit(feats, targets, alive)
        dev.partial_fit(np.stack(feats) if feats else np.zeros((0, d), np.float32), targets, alive)
        known = [t for t in alive if t in ref.samples]
        assert sorted(known) == sorted(dev.targets) or set(known) <= set(dev.targets)
        for t in known:
            assert dev.samples_count(t) == len(ref.samples[t])
        m = int(rng.integers(1, 40))
        dets = rng.normal(0, 1, (m, d)).astype(np.float32) + 3.0 * np.sin(rng.integers(0, 12, (m, 1)) + np.arange(d, dtype=np.float32))
        if not known:
            continue
        want = ref.distance(dets, known)
        got = dev.distance(dets, known)
        tol = 2e-6 if metric == "cosine" else 2e-6 * float(np.abs(want).max() + 1)
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=tol)
        thr = 0.15 if metric == "cosine" else float(np.median(want))
        gated = dev.distance(dets, known, max_distance=thr)
        far = want > thr + 10 * tol
        near = want < thr - 10 * tol
        np.testing.assert_allclose(gated[far], np.float32(thr) + np.float32(1e-5), rtol=1e-6)
        np.testing.assert_allclose(gated[near], want[near], rtol=1e-5, atol=tol)


def test_frame_pipeline_matches_the_synchronous_calls_and_the_oracle(eng_w0):
    """reid_frame_submit / _cost / _fetch / _update (one wait per frame, frame f+1 submitted before frame f is matched)
    give what Extractor.__call__ + metric.distance + iou_cost + metric.partial_fit give call by call, and what the oracle says."""
    from oracle import nn_matching as onm
    from reid_amd.iou_matching import iou_cost
    from reid_amd.nn_matching import NearestNeighborDistanceMetric
    eng, sd = eng_w0
    rng = np.random.default_rng(11)
    pool = synth.ragged_crops_u8(24, seed=4)
    pipe = NearestNeighborDistanceMetric("cosine", 0.15, 5, max_tracks=16)
    sync = NearestNeighborDistanceMetric("cosine", 0.15, 5, max_tracks=16)
    ref = onm.NearestNeighborDistanceMetric("cosine", 0.15, 5)
    frames = [[pool[(3 * f + i) % 24] for i in range(n)] for f, n in enumerate([5, 7, 0, 3, 9, 6])]
    boxes = rng.uniform(0, 300, (16, 4))
    boxes[:, 2:] = rng.uniform(10, 90, (16, 2))
    tracks = []
    eng.frame_submit(0, frames[0])
    for f, crops in enumerate(frames):
        slot = f & 1
        m = len(crops)
        pipe.frame_distance_begin(slot, tracks, max_distance=0.15, track_boxes=boxes[:len(tracks)], det_boxes=boxes[:m])
        if f + 1 < len(frames):
            eng.frame_submit(slot ^ 1, frames[f + 1])              # next frame goes up while this one is "matched"
        feats, cost, ic = pipe.frame_distance_end(slot)
        want_feats = eng.embed_ragged_u8(crops)
        np.testing.assert_array_equal(feats, want_feats)
        assert cost.shape == (len(tracks), m)
        if tracks and m:
            np.testing.assert_array_equal(cost, sync.distance(want_feats, tracks, max_distance=0.15))
            np.testing.assert_array_equal(ic, iou_cost(boxes[:len(tracks)], boxes[:m]))
            raw = ref.distance(want_feats, tracks)
            near = raw < 0.15 - 1e-5
            np.testing.assert_allclose(cost[near], raw[near], atol=2e-6)
            assert np.all(cost[raw > 0.15 + 1e-5] == np.float32(0.15) + np.float32(1e-5))
        else:
            assert ic is None
        # detection i updates track i; a new track per frame, the oldest dropped when more than 6 are alive
        k = min(m, len(tracks))
        rows, tg = list(range(k)), tracks[:k]
        if m > k:
            tracks.append(100 + f)
            rows.append(k)
            tg = tg + [100 + f]
        if len(tracks) > 6:
            tracks.pop(0)
        pipe.frame_partial_fit(slot, rows, tg, tracks)
        sync.partial_fit(want_feats[rows], tg, tracks)
        ref.partial_fit(list(want_feats[rows]), tg, tracks)
        for t in tracks:
            if t in ref.samples:
                assert pipe.samples_count(t) == len(ref.samples[t])
    with pytest.raises(_ffi.ReidHipError):
        eng.frame_update(0, pipe._bank, [99], [0])                 # row beyond the submitted frame


def test_frame_pipeline_large_frame_and_euclidean_metric(eng_w0):
    """A frame of 80 crops (more than one pass of the default 64-crop chunk), the euclidean metric, no boxes; then an empty
    frame and a frame costed without tracks."""
    from reid_amd.nn_matching import NearestNeighborDistanceMetric
    eng, _ = eng_w0
    pool = synth.ragged_crops_u8(20, seed=12)
    crops = [pool[i % 20] for i in range(80)]
    pipe = NearestNeighborDistanceMetric("euclidean", 50.0, 4, max_tracks=8)
    sync = NearestNeighborDistanceMetric("euclidean", 50.0, 4, max_tracks=8)
    want = eng.embed_ragged_u8(crops)
    for mtr in (pipe, sync):
        mtr.partial_fit(want[:6], [1, 1, 2, 3, 3, 3], [1, 2, 3])
    eng.frame_submit(1, crops)
    feats, cost, ic = pipe.frame_distance(1, [3, 1, 2], max_distance=40.0)
    np.testing.assert_array_equal(feats, want)
    np.testing.assert_array_equal(cost, sync.distance(want, [3, 1, 2], max_distance=40.0))
    assert ic is None and cost.shape == (3, 80)
    pipe.frame_partial_fit(1, [79, 0], [2, 1], [1, 2, 3])
    sync.partial_fit(want[[79, 0]], [2, 1], [1, 2, 3])
    eng.frame_submit(0, [])                                   # a frame without detections
    f0, c0, _ = pipe.frame_distance(0, [1, 2, 3])
    assert f0.shape == (0, 512) and c0.shape == (3, 0)
    eng.frame_submit(1, crops[:3])                            # ... and one costed against no track
    f1, c1, _ = pipe.frame_distance(1, [])
    np.testing.assert_array_equal(f1, eng.embed_ragged_u8(crops[:3]))   # (a 3-crop pass takes the split-K convolutions: fp32 noise vs want[:3])
    np.testing.assert_allclose(f1, want[:3], rtol=0, atol=2e-5 * np.abs(want).max())
    assert c1.shape == (0, 3)
    np.testing.assert_array_equal(pipe.distance(want[:5], [1, 2, 3]), sync.distance(want[:5], [1, 2, 3]))
    pipe.close()
    sync.close()


def test_camera_stream_driver_equals_the_blocking_calls():
    """tracking.CameraStream (own context, submit / step / commit) over four frames: features, gated appearance cost and DIoU cost
    equal the blocking Extractor-style calls on another context."""
    from reid_amd.engine import Engine
    from reid_amd.iou_matching import iou_cost
    from reid_amd.nn_matching import NearestNeighborDistanceMetric
    from reid_amd.tracking import CameraStream
    sd = synth.seres18_state_dict(0)
    blob, manifest, _ = weights.pack_seres18(sd)
    cam = CameraStream(blob, manifest, precision=0, max_dist=0.2, budget=4, max_tracks=8)
    ref_eng = Engine(0)
    ref_eng.load_seres18(blob, manifest)
    ref = NearestNeighborDistanceMetric("cosine", 0.2, 4, max_tracks=8, engine=ref_eng)
    pool = synth.ragged_crops_u8(12, seed=6)
    frames = [pool[0:4], pool[3:9], pool[8:11], pool[2:7]]
    rng = np.random.default_rng(2)
    boxes = rng.uniform(0, 200, (8, 4))
    boxes[:, 2:] = rng.uniform(10, 60, (8, 2))
    tracks = []
    cam.submit(frames[0])
    try:
        for f, crops in enumerate(frames):
            m = len(crops)
            feats, cost, ic = cam.step(tracks, boxes[:len(tracks)], boxes[:m], frames[f + 1] if f + 1 < len(frames) else None)
            want = ref_eng.embed_ragged_u8(crops)
            np.testing.assert_array_equal(feats, want)
            if tracks:
                np.testing.assert_array_equal(cost, ref.distance(want, tracks, max_distance=0.2))
                np.testing.assert_array_equal(ic, iou_cost(boxes[:len(tracks)], boxes[:m]))
            k = min(m, len(tracks))
            rows, tg = list(range(k)), tracks[:k]
            tracks.append(50 + f)
            rows.append(k)
            tg = tg + [50 + f]
            cam.commit(rows, tg, tracks)
            ref.partial_fit(want[rows], tg, tracks)
    finally:
        cam.close(destroy=True)
        ref.close()
        ref_eng.close()


def test_two_camera_streams_on_two_threads_do_not_disturb_each_other():
    """Two CameraStreams (own contexts) driven concurrently from two host threads give, frame by frame, what each gives alone."""
    import threading
    from reid_amd.tracking import CameraStream
    sd = synth.seres18_state_dict(0)
    blob, manifest, _ = weights.pack_seres18(sd)
    pool = synth.ragged_crops_u8(16, seed=7)
    boxes = np.random.default_rng(4).uniform(5, 150, (8, 4))

    def drive(cam, shift, out):
        frames = [[pool[(shift + 3 * f + i) % 16] for i in range(3 + (f + shift) % 4)] for f in range(12)]
        tracks = []
        cam.submit(frames[0])
        for f, crops in enumerate(frames):
            m = len(crops)
            feats, cost, ic = cam.step(tracks, boxes[:len(tracks)], boxes[:m], frames[f + 1] if f + 1 < len(frames) else None)
            out.append((feats.copy(), cost.copy()))
            k = min(m, len(tracks))
            rows, tg = list(range(k)), tracks[:k]
            if len(tracks) < 6:
                tracks.append(10 * shift + f)
                rows.append(min(k, m - 1))
                tg = tg + [10 * shift + f]
            cam.commit(rows, tg, tracks)
        cam.close()

    cams = [CameraStream(blob, manifest, precision=1, max_dist=0.3, budget=3, max_tracks=8) for _ in range(4)]
    try:
        alone = [[], []]
        for c in range(2):
            drive(cams[c], c + 1, alone[c])
        together = [[], []]
        th = [threading.Thread(target=drive, args=(cams[2 + c], c + 1, together[c])) for c in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        for c in range(2):
            assert len(alone[c]) == len(together[c]) == 12
            for (fa, ca), (fb, cb) in zip(alone[c], together[c]):
                np.testing.assert_array_equal(fa, fb)
                np.testing.assert_array_equal(ca, cb)
    finally:
        for cam in cams:
            cam.close(destroy=True)


def test_nn_matching_edge_cases(eng):
    from reid_amd.nn_matching import NearestNeighborDistanceMetric
    m = NearestNeighborDistanceMetric("cosine", 0.15, budget=3, max_tracks=2)
    e = np.eye(8, dtype=np.float32)
    m.partial_fit(e[:5], [1, 1, 1, 1, 1], [1])                   # five samples in one call, budget 3: e2, e3, e4 stay
    assert m.samples_count(1) == 3
    np.testing.assert_allclose(m.distance(e[:6], [1])[0], [1, 1, 0, 0, 0, 1], atol=1e-6)
    assert m.distance(np.zeros((0, 8), np.float32), [1]).shape == (1, 0)
    assert m.distance(e[:2], []).shape == (0, 2)
    with pytest.raises(KeyError):
        m.distance(e[:2], [99])
    m.partial_fit(e[:1], [2], [1, 2])
    with pytest.raises(RuntimeError):
        m.partial_fit(e[:1], [3], [1, 2, 3])                     # bank of two tracks is full
    m.partial_fit(np.zeros((0, 8), np.float32), [], [2])         # 1 dropped -> slot reusable
    m.partial_fit(e[5:6], [3], [2, 3])
    np.testing.assert_allclose(m.distance(e[5:6], [3, 2]), [[0.0], [1.0]], atol=1e-6)
    with pytest.raises(ValueError):
        NearestNeighborDistanceMetric("manhattan", 0.1)


# ----------------------------------------------------------------------------- crops cut from a frame on the device (§8f-3)
def test_embed_from_frame_equals_host_sliced_crops(eng_w0):
    """Extractor.from_frame(bbox_xywh, frame) == Extractor([frame[y1:y2, x1:x2] ...]) bit for bit (same taps, the frame is
    only indexed with a pitch), incl. boxes touching the frame border and a 3-pixel-wide window.  The host-sliced path is
    itself checked against the oracle's resize in tests/test_gpu_frontend.py::test_resize_on_device."""
    from reid_amd.extractor import Extractor
    eng, sd = eng_w0
    ext = Extractor(sd)
    rng = np.random.default_rng(9)
    frame = rng.integers(0, 256, (480, 640, 3), dtype=np.uint8)
    xywh = np.asarray([[100.4, 200.2, 60.0, 150.9], [5.0, 10.0, 40.0, 60.0], [630.0, 470.0, 50.0, 80.0], [320.0, 240.0, 2.2, 300.0],
                       [320.5, 240.5, 128.0, 256.0]])
    got = ext.from_frame(xywh, frame)
    crops = []
    for x, y, w, h in xywh:
        x1, y1 = max(int(x - w / 2), 0), max(int(y - h / 2), 0)
        x2, y2 = min(int(x + w / 2), 639), min(int(y + h / 2), 479)
        crops.append(frame[y1:y2, x1:x2])
    assert [c.shape[1] for c in crops][3] == 3
    want = ext(crops)
    assert np.array_equal(got, want)
    assert ext.from_frame(np.zeros((0, 4)), frame).size == 0
    with pytest.raises(_ffi.ReidHipError):
        eng.embed_frame_u8(frame, [[10, 10, 10, 50]])        # empty window
    with pytest.raises(_ffi.ReidHipError):
        eng.embed_frame_u8(frame, [[0, 0, 641, 50]])         # outside the frame


# ----------------------------------------------------------------------------- fused stem + maxpool kernel (fp16 path)
def test_f16_fused_stem_pool_matches_unfused_and_oracle(eng_w0):
    """stem_pool_f16.hip (conv 7x7 s2 + BN + MaxPool in one kernel, BN scale folded into the f16 weights) against the
    unfused GEMM + pool kernels (debug_keep 1) and the oracle's pooled map; every later stage and the embedding too."""
    eng, sd = eng_w0
    n = 6
    crops = synth.smooth_crops_u8(n, 3)
    crops[0] = 255          # saturated crop: all-equal windows
    crops[1, :, :3] = 0     # a dark left border exercises the -1 column clipping
    eng.set_precision(1)
    try:
        eng.debug_keep(1)
        emb_u = eng.embed_u8(crops)
        pool_u = eng.debug_stage(1, n)
        eng.debug_keep(2)
        emb_f = eng.embed_u8(crops)
        pool_f = eng.debug_stage(1, n)
        last_f = eng.debug_stage(9, n)
    finally:
        eng.debug_keep(0)
        eng.set_precision(0)
    taps = {}
    seres18.forward(sd, seres18.preprocess_u8(crops), taps)
    want = taps["pool0"].permute(0, 2, 3, 1).contiguous().numpy().reshape(-1)
    scale = np.abs(want).max()
    assert np.abs(pool_f - want).max() / scale < 4e-3        # f16 weights/activations, fp32 accumulate
    assert np.abs(pool_u - want).max() / scale < 4e-3
    assert np.abs(pool_f - pool_u).max() / scale < 4e-3      # scale folded before vs after the f16 rounding
    want9 = taps[synth.SERES18_BLOCKS[-1][0]].permute(0, 2, 3, 1).contiguous().numpy().reshape(-1)
    assert np.abs(last_f - want9).max() / np.abs(want9).max() < 1e-2
    cos = (emb_f * emb_u).sum(1) / np.linalg.norm(emb_f, axis=1) / np.linalg.norm(emb_u, axis=1)
    assert (1 - cos).max() < 2e-5
    emb_nk = None
    eng.set_precision(1)
    try:
        emb_nk = eng.embed_u8(crops)                         # production call: below 128 crops the tile-parallel kernels run
        big = np.concatenate([crops] * 22)[:128]             # 128 crops: the per-image kernels, as under debug_keep 2
        emb_big = eng.embed_u8(big)
    finally:
        eng.set_precision(0)
    for other in (emb_big[:n], emb_nk):                      # other pass sizes pick other tile shapes: equal to rounding
        cos = (other * emb_f).sum(1) / np.linalg.norm(other, axis=1) / np.linalg.norm(emb_f, axis=1)
        assert (1 - cos).max() < 2e-5


# ----------------------------------------------------------------------------- layer-1 kernel (register-resident weights)
def _conv_c64(eng, x, w, scale=None, shift=None, residual=None, relu=0, want_stats=True):
    import ctypes as C
    fn = _ffi.debug_lib().reid_debug_conv_c64
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_void_p]
    n = x.shape[0]
    out = np.empty((n, 64, 32, 64), np.float32)
    stats = np.empty((n, 64, 2), np.float32)
    p = lambda a: None if a is None else np.ascontiguousarray(a, np.float32).ctypes.data_as(C.c_void_p)
    keep = [np.ascontiguousarray(a, np.float32) if a is not None else None for a in (x, w, scale, shift, residual)]
    _ffi.check(fn(eng.h, n, *[None if a is None else a.ctypes.data_as(C.c_void_p) for a in keep], int(relu),
                  out.ctypes.data_as(C.c_void_p), stats.ctypes.data_as(C.c_void_p) if want_stats else None))
    return out, stats


@pytest.mark.parametrize("n,mode", [(1, "raw"), (3, "raw"), (5, "bn_res"), (2, "bn_res_relu"), (300, "bn_res")])
def test_conv3x3_c64_f16_kernel_against_torch(eng, n, mode):
    """conv3x3_c64_f16.hip in isolation (more images than CUs exercises the persistent loop): f16-rounded operands, fp32
    reference convolution in torch; output within f16 rounding, per-image statistics within fp32 summation error."""
    rng = np.random.default_rng(n)
    x = rng.normal(0, 1, (n, 64, 32, 64)).astype(np.float32)
    x[0, 0, :, :] = 3.0          # a bright top row / left column: border handling
    x[0, :, 0, :] = -2.0
    w = (rng.normal(0, 1, (64, 3, 3, 64)) / 24).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, 64).astype(np.float32) * np.where(rng.random(64) < 0.2, -1, 1).astype(np.float32)
    shift = rng.normal(0, 0.5, 64).astype(np.float32)
    res = rng.normal(0, 1, (n, 64, 32, 64)).astype(np.float32)
    if mode == "raw":
        got, stats = _conv_c64(eng, x, w.reshape(64, 576))
    else:
        got, stats = _conv_c64(eng, x, w.reshape(64, 576), scale, shift, res, relu=int(mode.endswith("relu")))
    h = lambda a: torch.from_numpy(a).half().float()
    wq = h(w * (scale[:, None, None, None] if mode != "raw" else 1.0))
    ref = F.conv2d(h(x).permute(0, 3, 1, 2), wq.permute(0, 3, 1, 2), padding=1)
    if mode != "raw":
        ref = ref.half().float() + torch.from_numpy(shift)[None, :, None, None] + h(res).permute(0, 3, 1, 2)
        if mode.endswith("relu"):
            ref = ref.clamp_min(0)
    ref = ref.permute(0, 2, 3, 1).numpy()
    sel = slice(None) if n <= 8 else slice(n - 3, n)
    err = np.abs(got[sel] - ref[sel])
    assert err.max() < 2e-2 and err.mean() < 2e-3, (err.max(), err.mean())
    s1 = ref.sum((1, 2))
    s2 = (ref.astype(np.float64) ** 2).sum((1, 2))
    np.testing.assert_allclose(stats[:, :, 0], s1, rtol=0, atol=1.5)          # 2048 values of O(1), f16-rounded outputs
    np.testing.assert_allclose(stats[:, :, 1], s2, rtol=5e-3, atol=1.0)


# ----------------------------------------------------------------------------- evaluation post-processing
def test_cam_debias_matches_reference_fixture(eng, golden_dir):
    """reid_cam_debias (Gram + Newton-Schulz inverse + projection as fp32 GEMMs) against the reference's own
    diminish_camera_bias output; also D = 1263 (the reference's descriptor width, padded to 1264 inside) against the oracle."""
    from oracle import postproc
    from reid_amd import inference_utils
    z = np.load(os.path.join(golden_dir, "postproc.npz"))
    got = eng.cam_debias(z["x"], z["cams"])
    np.testing.assert_allclose(got, z["debiased"], rtol=0, atol=5e-5)
    t = torch.from_numpy(z["x"].copy())
    assert inference_utils.diminish_camera_bias(t, torch.from_numpy(z["cams"])) is t      # in place, like the reference
    np.testing.assert_allclose(t.numpy(), z["debiased"], rtol=0, atol=5e-5)
    _, _, _, x, _, cams = synth.clustered_embeddings(1, 1500, d=1263, n_ids=60, n_cams=3, seed=43, sigma=0.9)
    cams[cams == 1] = 4                     # ids 1 and 3 have no rows: skipped
    got = eng.cam_debias(x, cams)
    want = postproc.diminish_camera_bias(x, cams)
    np.testing.assert_allclose(got, want, rtol=0, atol=5e-5)


def test_tta_descriptor_matches_oracle(eng_w0):
    """reid_descriptor_f32_nchw: device flip + two forwards + cat/average/normalise against the oracle forward on the plain
    and mirrored images (image_reid_inference.py:112-123,252-253)."""
    from oracle import postproc
    eng, sd = eng_w0
    x = seres18.preprocess_u8(synth.smooth_crops_u8(5, 7))
    got = eng.descriptor_f32_nchw(x.numpy(), flip_tta=True)
    e1, l1 = seres18.forward(sd, x)
    e2, l2 = seres18.forward(sd, torch.flip(x, dims=[3]))
    want = postproc.tta_descriptor(e1.numpy(), l1.numpy(), e2.numpy(), l2.numpy())
    assert got.shape == (5, 512 + 751)
    np.testing.assert_allclose(got, want, rtol=0, atol=2e-5)
    np.testing.assert_allclose(np.linalg.norm(got, axis=1), 1.0, atol=1e-5)
    single = eng.descriptor_f32_nchw(x.numpy(), flip_tta=False)
    np.testing.assert_allclose(single, postproc.descriptor(e1.numpy(), l1.numpy()), rtol=0, atol=2e-5)


# ----------------------------------------------------------------------------- BASELINE configs[1] at full size
@pytest.mark.parametrize("precision", [0, 1, 2])
def test_full_size_config1_properties(eng_w0, precision):
    """4096 crops + 4096 x 4096 L2 matrix (BASELINE configs[1]) through size-independent properties: the batch holds 256
    distinct crops, each 16 times, in shuffled order.  Crops are independent in eval mode (per-sample InstanceNorm / SE), so
    (a) copies of a crop get bit-identical embeddings wherever they sit in the batch; a different pass size may pick another
        tile shape for some layer (per-column partial sums of the InstanceNorm statistics then add up in another order), so
        across pass sizes they agree to rounding, not bit for bit,
    (b) the distance matrix is symmetric with a ~0 diagonal, duplicates are at distance ~0 and the 16 nearest neighbours of
        every row are exactly its 16 copies (k-NN selection at full size),
    (c) a sample of rows equals the oracle within the mode's tolerance."""
    eng, sd = eng_w0
    rng = np.random.default_rng(11)
    base = synth.smooth_crops_u8(256, 5)
    ids = np.repeat(np.arange(256), 16)
    rng.shuffle(ids)
    crops = base[ids]
    eng.set_precision(precision)
    try:
        eng.set_chunk(1024)
        emb = eng.embed_u8(crops)
        eng.set_chunk(96)                     # ragged passes: 96 does not divide 4096
        emb_small = eng.embed_u8(crops[:1000])
        first = np.asarray([np.flatnonzero(ids == c)[0] for c in range(256)])
        assert np.array_equal(emb, emb[first][ids])                     # (a) position invariance, bit-exact
        rel = np.abs(emb_small - emb[:1000]).max() / np.abs(emb).max()
        assert rel < (2e-3 if precision == 1 else 1e-4)                 # (a) pass-size invariance, to rounding
        dist = eng.distmat(emb, emb, _ffi.METRIC_L2)
        scale = float(np.median(dist))
        assert np.abs(dist - dist.T).max() <= 1e-4 * scale
        # |x|^2 + |y|^2 - 2x.y cancels ~1e-7 * |x|^2 in fp32 (the reference's addmm_ does too); the sqrt makes that 1e-3..1e-2 of a distance
        assert np.abs(np.diag(dist)).max() <= 1e-2 * scale
        same = ids[:, None] == ids[None, :]
        assert dist[same].max() <= 1e-2 * scale
        assert dist[~same].min() > 20 * dist[same].max()
        _, knn = eng.knn(emb, emb, 16)
        assert np.array_equal(np.sort(ids[knn], axis=1), np.repeat(ids[:, None], 16, 1))   # (b)
        sample = first[:6]
        want = seres18.embed_u8(sd, crops[sample])                      # (c)
        cos = (emb[sample] * want).sum(1) / np.linalg.norm(emb[sample], axis=1) / np.linalg.norm(want, axis=1)
        assert (1 - cos).max() < (1e-4 if precision == 1 else 1e-5)
    finally:
        eng.set_chunk(128)
        eng.set_precision(0)


@pytest.mark.parametrize("n", [1, 3, 7, 33])
def test_f16_path_small_and_odd_batches(eng_w0, n):
    """Batches that leave tiles ragged everywhere in the fp16 path: a single crop, odd counts (the 16x8 layers pair images per
    block), fewer images than CUs (persistent layer-1 / stem kernels with idle blocks) - against the exact fp32 path."""
    eng, sd = eng_w0
    crops = synth.smooth_crops_u8(n, 40 + n)
    ref = eng.embed_u8(crops)
    eng.set_precision(1)
    try:
        got = eng.embed_u8(crops)
        again = eng.embed_u8(np.concatenate([crops, crops[::-1]]))      # same crops inside a larger, different batch
    finally:
        eng.set_precision(0)
    cos = (got * ref).sum(1) / np.linalg.norm(got, axis=1) / np.linalg.norm(ref, axis=1)
    assert (1 - cos).max() < 1e-4
    scale = np.abs(ref).max()
    assert np.abs(again[:n] - got).max() <= 2e-3 * scale and np.abs(again[n:][::-1] - got).max() <= 2e-3 * scale


# ----------------------------------------------------------------------------- reference-held vectors at BASELINE sizes
# (precision, pass size) -> rows of config 1's NOISE set whose arg-min is allowed to differ from the reference's because the
# reference's own top-2 gap there is below the fp32 noise (2e-6).  Row 84: reference gap 2.7e-7 - the size of the
# reference's own batch-size instability; which of its two candidates a kernel picks is a property of its summation order.
#   (0, 1024): exact fp32, the 256 crops as ONE pass - found when this list was introduced (round 6; rounds 2-5 printed it: the exact-fp32
#              kernels did not change in round 6, the pass of 256 splits its K loops differently from four passes of 64)
#   (2, 1024): fp32-class, the 256 crops as ONE pass - row 180, reference gap 6e-8 (one ulp of the distance).  (2, 64) held row 84
#              while layers 3-4 of such a pass ran conv3x3_x3.hip's split-K forms; it left the list when conv_x3s_kernel took the
#              strided / 1x1 convolutions (round 6).
# Every other combination reproduces all 256 rows.
CONFIG1_RAND0_KNOWN_SUBNOISE_ROWS = {(0, 1024): {84}, (2, 1024): {180}}   # (2, 64): {84} until conv_x3s_kernel took the strided / 1x1 convolutions (round 6); row 180: gap 6e-8 = one ulp
@pytest.mark.parametrize("chunk", [40, 64, 130, 1024])   # passes of 40 (+ 16) and 130 + 126 crops: the small- and mid-size launch rules of round 6; four passes of 64 (the library default of rounds 1-3); one pass of 256
@pytest.mark.parametrize("precision", [0, 1, 2])
@pytest.mark.parametrize("tag,crops_fn,seed", [("rand0", synth.crops_u8, 0), ("smooth5", synth.smooth_crops_u8, 5)])
def test_config1_against_reference_vectors(eng_w0, golden_dir, precision, tag, crops_fn, seed, chunk):
    """BASELINE configs[0]: 256 crops -> emb[256,512] -> (1 - cos) / 2 matrix -> row arg-min, against vectors the REFERENCE's own
    SERse18_IBN + cosine_dist produced (tests/golden/config1.npz, oracle/gen_golden.py:gen_config1).  The arg-min vector is
    compared on ALL 256 rows: the number of differing rows is printed and every one of them must be a row whose top-2 gap in the
    reference is inside the arithmetic's own noise (north_star: "argmin ranks bit-exact" - a rank can only be decided where the
    reference itself separates the two candidates by more than one rounding of the distance); on the realistic set no row may
    differ at all in the exact-fp32 and the fp32-class mode."""
    eng, _ = eng_w0
    g = np.load(os.path.join(golden_dir, "config1.npz"))
    ref, gap = g[tag + "_emb"], g[tag + "_gap"]
    eng.set_precision(precision)
    eng.set_chunk(chunk)
    try:
        emb = eng.embed_u8(crops_fn(256, seed))
    finally:
        eng.set_precision(0)
        eng.set_chunk(1024)
    cos = (emb * ref).sum(1) / np.linalg.norm(emb, axis=1) / np.linalg.norm(ref, axis=1)
    f16s = precision == 1                                                 # precision 2 (fp32-class) is held to the fp32 thresholds
    assert (1 - cos).max() < (1e-4 if f16s else 1e-5)                     # north_star allows 1e-3
    dist = eng.distmat(emb, emb, _ffi.METRIC_COS_HALF)
    np.testing.assert_allclose(dist, g[tag + "_cosdist"], atol=(2e-4 if f16s else 2e-6))
    d = dist.copy()
    np.fill_diagonal(d, np.inf)
    flips = np.flatnonzero(d.argmin(1) != g[tag + "_argmin"])
    noise = 2e-4 if f16s else 2e-6                                        # twice the distance error asserted above
    decided = int((gap >= noise).sum())
    print("config1 %s precision %d: %d of 256 rows decided (reference top-2 gap >= %.0e), %d arg-mins differ, largest gap among "
          "them %.2e" % (tag, precision, decided, noise, len(flips), gap[flips].max() if len(flips) else 0.0))
    assert (gap[flips] < noise).all(), (flips, gap[flips])
    if tag == "smooth5":
        assert decided >= (150 if f16s else 250)                          # realistic crops: (nearly) every row is decided
    if not f16s:
        # the bar for a headline arithmetic (restated in round 5 - round-4 verdict, SURVEY.md Q15 / section 7 "hard parts"): no flip
        # where the reference separates the two candidates by more than the arithmetic's noise (asserted above, both sets), and
        # none at ALL on the realistic set (smooth5: smallest reference gap 6.5e-6).  The noise set (rand0) has one row whose
        # reference top-2 gap is 2.7e-7 - the size of the reference's OWN batch-size instability (2.4e-7): whether a
        # kernel agrees there is a property of its summation order, not of its parity, so such rows are printed, not failed
        # (rounds 2-4 asserted 0 of 256 on both sets, which vetoed every kernel that sums in another order on a coin flip).
        if tag == "smooth5":
            assert len(flips) == 0, (flips, gap[flips])
        else:
            # The published claim (README, DESIGN section 2, bench.py --precision help) is "0 of 256 rows differ on the noise set too,
            # at HEAD".  That claim is ENFORCED here through an explicit allowlist (CONFIG1_RAND0_KNOWN_SUBNOISE_ROWS): a kernel change that flips a
            # sub-noise row fails this test until the row is recorded in it (with the commit that moved it) and the published
            # sentence is reworded in the same commit.  Rows above the noise can never be listed: they failed the assertion above.
            if len(flips):
                print("config1 rand0 precision %d chunk %d: sub-noise rows that differ (row, reference gap): %s"
                      % (precision, chunk, [(int(r), float(gap[r])) for r in flips]))
            unexpected = sorted(set(int(r) for r in flips) - CONFIG1_RAND0_KNOWN_SUBNOISE_ROWS.get((precision, chunk), set()))
            assert not unexpected, ("rows %s of the noise set now differ from the reference's arg-min (reference gaps %s, all below the "
                                    "2e-6 noise): record them in CONFIG1_RAND0_KNOWN_SUBNOISE_ROWS and reword the '0 of 256' claims"
                                    % (unexpected, [float(gap[r]) for r in unexpected]))


@pytest.mark.parametrize("n", [1, 3, 7, 21, 30, 33, 48, 62, 66, 130])
def test_small_pass_split_k_forms_agree_and_are_position_invariant(eng_w0, n):
    """Round 6: small and mid-size passes run layer 4 (from 24 crops), layer 3 (from ~48) and large-enough 16- / 32-wide maps on
    conv3x3_x3.hip's kernels with the K loop split over 2-4 blocks per tile, reduced as a reduce-scatter (x3m16_tail: partials as 16-byte
    units, an arrival counter per tile, every block finishes a column slice, own slice in LDS).  Against the 12-wave forms of
    conv3x3_f16.hip that served these sizes until round 5 (debug switch split_x3_small = 0): same three products per multiply in another
    summation order - agreement to 5e-6 of the embedding's scale - and, the property that must hold exactly: copies of a crop inside
    one pass give bit-identical embeddings wherever they sit (another tile, another column slice, another image pair).
    The sizes sit on both sides of the steps of the pass-size staircase (profiles/r06_pass_size_sweep_8_100.txt) where the launch rules
    change form: 21 / 30 (layers 3-4 on these kernels at every size), 33 / 48 / 62 (layer 1 leaves the 12-wave kernel, the stem's strips
    fill one round, layer 4 takes 64-wide tiles), 66 (two ways split, wide again), 130 (unsplit, 64-wide because the last layer of
    128-wide blocks would cover 4 of 256 CUs).  Layer 4's tile width (switch x3_l4_narrow_nmt = 0: always 128 wide) must not change a
    bit where the K loop is not split, and stays within 5e-6 where the two widths split differently."""
    eng, _ = eng_w0
    base = synth.smooth_crops_u8(max(2, (n + 1) // 2), 90 + n)
    ids = np.arange(n) % len(base)                       # every crop at least twice when n >= 2 (odd n: one image pair is ragged)
    np.random.default_rng(n).shuffle(ids)
    crops = base[ids]
    eng.set_precision(2)
    try:
        got = eng.embed_u8(crops)
        first = np.asarray([np.flatnonzero(ids == c)[0] for c in range(len(base)) if (ids == c).any()])
        lut = {int(ids[f]): got[f] for f in first}
        assert all(np.array_equal(got[i], lut[int(ids[i])]) for i in range(n))
        eng.debug_switch("x3_l4_narrow_nmt", 0)
        wide = eng.embed_u8(crops)
        if n > 128:
            assert np.array_equal(got, wide)
        else:
            assert np.abs(got - wide).max() <= 5e-6 * np.abs(wide).max()
        eng.debug_switch("x3_l4_narrow_nmt", 31)
        eng.debug_switch("split_x3_small", 0)
        old = eng.embed_u8(crops)
        assert np.abs(got - old).max() <= 5e-6 * np.abs(old).max()
        assert eng.fault_bits() == 0
    finally:
        eng.debug_switch("x3_l4_narrow_nmt", 31)
        eng.debug_switch("split_x3_small", 2)
        eng.set_precision(0)


@pytest.mark.parametrize("precision", [0, 2])
def test_multi_camera_batched_stream_equals_independent_camera_streams(eng_w0, precision):
    """tracking.MultiCameraStream - K cameras' crops of a frame time in ONE pass, per-camera banks, per-camera cost blocks
    (reid_frame_cost_groups) - against K independent CameraStreams fed the same crops (the reference runs one
    track_yolov5.py:178-253 loop per video): features and gated appearance costs agree to fp32 summation order (a crop's
    embedding depends on the pass it rides in only through the tile shapes chosen for the pass size), DIoU costs bit for bit,
    over 6 frame times with bank updates, ragged detection counts, a camera without detections and one without tracks."""
    from reid_amd.tracking import CameraStream, MultiCameraStream
    eng, sd = eng_w0
    blob, manifest = weights.pack_seres18(sd)[:2]
    K, frames = 3, 6
    rng = np.random.default_rng(17)
    pool = synth.ragged_crops_u8(64, seed=12)
    counts = [[5, 9, 0], [7, 1, 4], [3, 3, 3], [12, 0, 2], [1, 6, 8], [4, 4, 9]]
    crops = lambda f, c: [pool[(11 * f + 5 * c + i) % 64] for i in range(counts[f][c])]
    tracks = [list(range(6)), list(range(100, 104)), []]            # camera 2 has no tracks at all
    seeds = [rng.normal(size=(len(t) * 3, 512)).astype(np.float32) for t in tracks]
    boxes = rng.uniform(0, 300, (16, 4))
    boxes[:, 2:] = rng.uniform(10, 90, (16, 2))
    mc = MultiCameraStream(blob, manifest, K, precision)
    singles = [CameraStream(blob, manifest, precision) for _ in range(K)]
    try:
        for c in range(K):
            if tracks[c]:
                for obj in (mc.metrics[c], singles[c].metric):
                    obj.partial_fit(seeds[c], np.repeat(tracks[c], 3), tracks[c])
        mc.submit([crops(0, c) for c in range(K)])
        for c in range(K):
            singles[c].submit(crops(0, c))
        for f in range(frames):
            nxt = f + 1 < frames
            got = mc.step(tracks, [boxes[:len(t)] for t in tracks], [boxes[:counts[f][c]] for c in range(K)],
                          [crops(f + 1, c) for c in range(K)] if nxt else None)
            for c in range(K):
                feats, cost, iou = singles[c].step(tracks[c], boxes[:len(tracks[c])], boxes[:counts[f][c]], crops(f + 1, c) if nxt else None)
                gf, gc, gi = got[c]
                assert gf.shape == (counts[f][c], 512) and gc.shape == (len(tracks[c]), counts[f][c])
                if counts[f][c]:
                    assert np.abs(gf - feats).max() <= 2e-5 * np.abs(feats).max()
                if gc.size:
                    np.testing.assert_allclose(gc, cost, atol=2e-5)
                    assert np.array_equal(gi, iou)
                k = min(counts[f][c], len(tracks[c]))
                singles[c].commit(np.arange(k), tracks[c][:k], tracks[c])
            mc.commit([np.arange(min(counts[f][c], len(tracks[c]))) for c in range(K)],
                      [tracks[c][:min(counts[f][c], len(tracks[c]))] for c in range(K)], tracks)
        for c in range(K):
            for t in tracks[c]:
                assert mc.metrics[c].samples_count(t) == singles[c].metric.samples_count(t)
    finally:
        mc.close(destroy=True)
        for s_ in singles:
            s_.close(destroy=True)


@pytest.mark.parametrize("precision", [0, 2])
def test_lookahead_stream_equals_the_frame_by_frame_stream(eng_w0, precision):
    """tracking.LookaheadCameraStream - F consecutive frames of ONE camera embedded as one pass, costs and bank updates per frame and
    in order - against `CameraStream` on the same detection dump: features and gated costs equal to fp32 summation order (a crop's
    embedding depends on the pass size through tile shapes only), DIoU bit for bit, bank sample counts equal; groups of 3 frames,
    the last group short, frames without detections.  Both forms of the look-ahead stream - cost / update stages on the match stream
    with the next group handed over at the group's first frame (reid_frame_match_stream), and everything on one stream - must agree
    BIT FOR BIT with each other."""
    from reid_amd.tracking import CameraStream, LookaheadCameraStream
    eng, sd = eng_w0
    blob, manifest = weights.pack_seres18(sd)[:2]
    rng = np.random.default_rng(23)
    pool = synth.ragged_crops_u8(48, seed=14)
    counts = [6, 0, 9, 4, 11, 2, 5, 7]                       # 8 frames -> groups of 3, 3, 2
    crops = lambda f: [pool[(7 * f + i) % 48] for i in range(counts[f])]
    tracks = list(range(5))
    boxes = rng.uniform(0, 300, (16, 4))
    boxes[:, 2:] = rng.uniform(10, 90, (16, 2))
    seeds = rng.normal(size=(15, 512)).astype(np.float32)
    la = LookaheadCameraStream(blob, manifest, 3, precision)                          # cost / update stages on the match stream
    la1 = LookaheadCameraStream(blob, manifest, 3, precision, match_stream=False)     # everything on one stream
    one = CameraStream(blob, manifest, precision)
    assert la.match_stream and not la1.match_stream
    try:
        for obj in (la.metric, la1.metric, one.metric):
            obj.partial_fit(seeds, np.repeat(tracks, 3), tracks)
        groups = [[0, 1, 2], [3, 4, 5], [6, 7]]
        for s_ in (la, la1):
            s_.submit_group([crops(f) for f in groups[0]])
        one.submit(crops(0))
        for gi, g in enumerate(groups):
            assert la.handover == 0 and la1.handover == len(g) - 1
            for j, f in enumerate(g):
                nxt = lambda s_: [crops(x) for x in groups[gi + 1]] if (j == s_.handover and gi + 1 < len(groups)) else None
                gf, gc, gi_ = la.step(j, tracks, boxes[:5], boxes[:counts[f]], nxt(la))
                gf1, gc1, gi1 = la1.step(j, tracks, boxes[:5], boxes[:counts[f]], nxt(la1))
                feats, cost, iou = one.step(tracks, boxes[:5], boxes[:counts[f]], crops(f + 1) if f + 1 < len(counts) else None)
                assert gf.shape == (counts[f], 512) and gc.shape == (5, counts[f])
                # the two look-ahead forms run the same passes and the same stages in the same order: bit for bit
                assert np.array_equal(gf, gf1) and np.array_equal(gc, gc1)
                if counts[f]:
                    assert np.array_equal(gi_, gi1)
                    assert np.abs(gf - feats).max() <= 2e-5 * np.abs(feats).max()
                    np.testing.assert_allclose(gc, cost, atol=2e-5)
                    assert np.array_equal(gi_, iou)
                k = min(counts[f], 5)
                la.commit(j, np.arange(k), tracks[:k], tracks)
                la1.commit(j, np.arange(k), tracks[:k], tracks)
                one.commit(np.arange(k), tracks[:k], tracks)
        for t in tracks:
            assert la.metric.samples_count(t) == one.metric.samples_count(t) == la1.metric.samples_count(t)
        # the bank's other entry points while the match stream is on: ordered on it (a clear, then costs from host features)
        q = rng.normal(size=(4, 512)).astype(np.float32)
        for s_ in (la, la1, one):
            s_.metric.partial_fit(q, np.asarray([0, 1, 2, 3]), tracks[:4])        # drops track 4
        d_la, d_la1, d_one = (s_.metric.distance(q, tracks[:4]) for s_ in (la, la1, one))
        assert np.array_equal(d_la, d_la1)
        np.testing.assert_allclose(d_la, d_one, atol=2e-5)
    finally:
        la.close(destroy=True)
        la1.close(destroy=True)
        one.close(destroy=True)


@pytest.mark.parametrize("precision", [0, 2])
def test_host_entry_points_pipeline_passes_bit_identically(eng_w0, precision):
    """Host in -> host out, the reference's own shape (feature_extractor.py:48-53 `.to(device)` ... `.cpu().numpy()`,
    image_reid_inference.py:116-122): with more crops than one pass holds the entry points upload pass k + 1 and download pass
    k - 1 on a copy stream under pass k's kernels (host_passes, csrc/reid_internal.h).  Same passes, same order, same stream:
    the results must equal the unpipelined call (debug switch host_pipeline = 0) BIT FOR BIT - pageable and pinned sources, a
    ragged last pass, logits, the float NCHW entry, ragged crops (contiguous views and separately allocated arrays)."""
    eng, _ = eng_w0
    n = 150
    crops = synth.smooth_crops_u8(n, 71)
    eng.set_precision(precision)
    eng.set_chunk(32)                                      # 5 passes, the last one of 22 crops
    try:
        def both(fn):
            eng.debug_switch("host_pipeline", 0)
            a = fn()
            eng.debug_switch("host_pipeline", 1)
            return a, fn()
        (e0, l0), (e1, l1) = both(lambda: eng.embed_u8(crops, logits=True))
        assert np.array_equal(e0, e1) and np.array_equal(l0, l1) and np.isfinite(e1).all()
        slab = eng.pinned(crops.nbytes).reshape(crops.shape)   # pinned source: real asynchronous DMA
        slab[...] = crops
        assert np.array_equal(eng.embed_u8(slab), e0)
        x = ((crops[:70].astype(np.float32) / 255.0 - 0.5) / 0.5).transpose(0, 3, 1, 2).copy()
        f0, f1 = both(lambda: eng.embed_f32_nchw(x))
        assert np.array_equal(f0, f1)
        rag = synth.ragged_crops_u8(70, 9)
        r0, r1 = both(lambda: eng.embed_ragged_u8(rag))
        assert np.array_equal(r0, r1)
        views = [slab[i] for i in range(n)]                # consecutive views of one buffer: handed over in place
        v0, v1 = both(lambda: eng.embed_ragged_u8(views))
        assert np.array_equal(v0, v1)
        assert np.array_equal(v1, eng.embed_ragged_u8([c.copy() for c in views]))   # = the packed copy of separate arrays
        cos = (v1 * e0).sum(1) / np.linalg.norm(v1, axis=1) / np.linalg.norm(e0, axis=1)
        assert (1 - cos).max() < 1e-6                      # resize of a 128x256 crop is the identity (float vs uint8 stem loader)
    finally:
        eng.debug_switch("host_pipeline", 1)
        eng.set_chunk(1024)
        eng.set_precision(0)


def test_swin_host_entry_pipeline_bit_identical(eng):
    """reid_swin_embed_f32_nchw in passes: pipelined upload / download against the unpipelined call, bit for bit."""
    eng.load_swin(*weights.pack_swin(synth.swin_state_dict(0))[:2])
    x = synth.images_f32(11, 3)
    eng.set_chunk(4)
    try:
        eng.debug_switch("host_pipeline", 0)
        a, la = eng.swin_embed_f32_nchw(x, logits=True)
        eng.debug_switch("host_pipeline", 1)
        b, lb = eng.swin_embed_f32_nchw(x, logits=True)
        assert np.array_equal(a, b) and np.array_equal(la, lb) and np.isfinite(b).all()
    finally:
        eng.debug_switch("host_pipeline", 1)
        eng.set_chunk(1024)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("layout", ["one_pass_64", "four_passes_16", "pass_1024_shuffled_copies"])
@pytest.mark.parametrize("precision", [0, 1, 2])
@pytest.mark.parametrize("tag,img_fn,seed", [("noise0", synth.noise_images_f32, 0), ("smooth11", synth.images_f32, 11)])
def test_swin_config_against_reference_vectors(eng, golden_dir, precision, tag, img_fn, seed, layout):
    """BASELINE configs[2]'s rank parity (north_star: "argmin ranks bit-exact"), the Swin counterpart of
    test_config1_against_reference_vectors: 64 images -> emb[64,96] -> (1 - cos) / 2 matrix -> row arg-min against vectors the
    REFERENCE's own swin_t + cosine_dist produced (tests/golden/swin_config.npz, oracle/gen_golden.py:gen_swin_config;
    /root/reference/reid/backbones/swin_transformer.py:397-427, reid/losses/utils.py:12-18), at three pass layouts: the 64 images as
    one pass, as four passes of 16, and as 1024 images (64 distinct x 16, shuffled) in ONE pass of the bench's size - copies must
    then be bit-identical and the first copy of each image gives the 64 rows.  Bar = config 1's: no arg-min may differ where the
    reference separates the two candidates by more than the asserted matrix noise; on the structured set (every row decided) none
    at all in the exact-fp32 and the fp32-class mode; sub-noise rows of the noise set that differ are printed."""
    g = np.load(os.path.join(golden_dir, "swin_config.npz"))
    ref, gap = g[tag + "_emb"], g[tag + "_gap"]
    eng.load_swin(*weights.pack_swin(synth.swin_state_dict(0))[:2])
    base = img_fn(64, seed)
    eng.set_precision(precision)
    try:
        if layout == "pass_1024_shuffled_copies":
            ids = np.repeat(np.arange(64), 16)
            np.random.default_rng(31).shuffle(ids)
            eng.set_chunk(1024)
            big = eng.swin_embed_f32_nchw(base[ids])
            first = np.asarray([np.flatnonzero(ids == c)[0] for c in range(64)])
            assert np.array_equal(big, big[first][ids])                  # copies of an image: bit-identical wherever they sit
            emb = big[first]
        else:
            eng.set_chunk(64 if layout == "one_pass_64" else 16)
            emb = eng.swin_embed_f32_nchw(base)
    finally:
        eng.set_precision(0)
        eng.set_chunk(1024)
    cos = (emb * ref).sum(1) / np.linalg.norm(emb, axis=1) / np.linalg.norm(ref, axis=1)
    f16s = precision == 1
    assert (1 - cos).max() < (1e-4 if f16s else 1e-5)                     # north_star allows 1e-3
    dist = eng.distmat(emb, emb, _ffi.METRIC_COS_HALF)
    np.testing.assert_allclose(dist, g[tag + "_cosdist"], atol=(2e-4 if f16s else 2e-6))
    d = dist.copy()
    np.fill_diagonal(d, np.inf)
    flips = np.flatnonzero(d.argmin(1) != g[tag + "_argmin"])
    noise = 2e-4 if f16s else 2e-6                                        # the distance error asserted above
    decided = int((gap >= noise).sum())
    print("swin_config %s precision %d %s: %d of 64 rows decided (reference top-2 gap >= %.0e), %d arg-mins differ, largest gap "
          "among them %.2e" % (tag, precision, layout, decided, noise, len(flips), gap[flips].max() if len(flips) else 0.0))
    assert (gap[flips] < noise).all(), (flips, gap[flips])
    if not f16s:
        if tag == "smooth11":
            assert decided == 64 and len(flips) == 0, (flips, gap[flips])
        elif len(flips):
            print("swin_config noise0 precision %d %s: sub-noise rows that differ (row, reference gap): %s"
                  % (precision, layout, [(int(r), float(gap[r])) for r in flips]))


@pytest.mark.parametrize("tag,sigma", [("s03", 0.3), ("s30", 3.0)])
def test_config5_market_full_size_against_reference(eng, golden_dir, tag, sigma):
    """BASELINE configs[4] at full size, single GPU: 3368 x 15913 x 512 similarity + evaluate_all against the REFERENCE's
    evaluate_all on the same synthetic Market-1501-sized problem (tests/golden/config5.npz): CMC exact, per-query first-good
    rank exact, mAP, and the top-1 gallery index of every query (bit-exact wherever the top-2 score gap exceeds fp32 rounding)."""
    from reid_amd.evaluate import evaluate_all
    g = np.load(os.path.join(golden_dir, "config5.npz"))
    qf, ql, qc, gf, gl, gc = synth.clustered_embeddings(3368, 15913, d=512, n_ids=751, n_cams=6, seed=4, sigma=sigma)
    cmc, mean_ap = evaluate_all(qf, ql, qc, gf, gl, gc, verbose=False)
    np.testing.assert_array_equal(np.asarray(cmc), g[tag + "_cmc"])       # Rank-1 .. Rank-15913 exact
    assert abs(mean_ap - float(g[tag + "_map"])) < 1e-7                   # a near-tie may swap two ranks of one query
    _, ap, valid = eng.rank_eval(qf, ql, qc, gf, gl, gc)
    dap = np.abs(ap - g[tag + "_ap"])                                     # per-query AP: equal except where two gallery items tie to
    assert (dap > 1e-9).sum() <= 0.02 * len(dap) and dap.max() < 5e-3, ((dap > 1e-9).sum(), dap.max())   # rounding and swap ranks
    top1, _ = eng.argmin_rows(qf, gf, _ffi.METRIC_COS)                    # unit-norm rows: arg-min of 1 - cos = arg-max of gf @ q
    flips = np.flatnonzero(top1 != g[tag + "_top1"])
    for q in flips:                                                       # only exact or rounding-level ties may move
        s = gf.astype(np.float64) @ qf[q].astype(np.float64)
        assert abs(s[top1[q]] - s[g[tag + "_top1"][q]]) < 2e-7, (q, s[top1[q]], s[g[tag + "_top1"][q]])
    print("config5 %s: Rank-1 %.6f mAP %.6f, %d of 3368 per-query APs differ by > 1e-9 (max %.1e), %d of 3368 top-1 indices differ "
          "(all within 2e-7 of the reference's best score)" % (tag, float(np.asarray(cmc)[0]), mean_ap, int((dap > 1e-9).sum()), dap.max(), len(flips)))


def test_entry_points_from_a_worker_thread(eng_w0):
    """hipSetDevice is per-thread: a fresh thread starts on device 0 whatever the engine's device is.  Every C entry point
    switches to the context's device itself (DeviceGuard), so a call from another thread gives the same bits."""
    import threading
    eng, _ = eng_w0
    crops = synth.smooth_crops_u8(5, 77)
    want = eng.embed_u8(crops)
    got = {}

    def work():
        got["emb"] = eng.embed_u8(crops)
        got["dist"] = eng.distmat(got["emb"], got["emb"], _ffi.METRIC_L2)
    t = threading.Thread(target=work)
    t.start()
    t.join()
    assert np.array_equal(got["emb"], want)
    assert np.array_equal(got["dist"], eng.distmat(want, want, _ffi.METRIC_L2))


# ----------------------------------------------------------------------------- multi-GPU exchange behind the C ABI (one GPU here)
def _loopback_engines(world, sd=None):
    """`world` engine contexts on device 0 joined by the loop-back communicator of libreid_hip_debug.so (one host thread per
    rank drives them): the multi-rank code of csrc/comm.hip with world > 1 on one GPU."""
    import ctypes as C
    from reid_amd.engine import Engine
    engs = [Engine(0) for _ in range(world)]
    if sd is not None:
        blob, manifest, _ = weights.pack_seres18(sd)
        for e in engs:
            e.load_seres18(blob, manifest)
    arr = (C.c_void_p * world)(*[e.h for e in engs])
    _ffi.check(_ffi.debug_lib().reid_debug_comm_loopback(arr, world))
    return engs


def _run_ranks(world, fn):
    """fn(rank) on one thread per rank (ctypes releases the GIL inside the C calls, so the ranks meet in the collectives)."""
    import threading
    res, err = [None] * world, [None] * world

    def work(r):
        try:
            res[r] = fn(r)
        except BaseException as e:     # noqa: BLE001 - reported below, on the main thread
            err[r] = e
    th = [threading.Thread(target=work, args=(r,)) for r in range(world)]
    for t in th:
        t.start()
    for t in th:
        t.join(300)
    for r, e in enumerate(err):
        if e is not None:
            raise AssertionError("rank %d: %r" % (r, e))
    return res


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world", [2, 3, 8])
def test_loopback_ranks_crops_sharded_and_gallery_sharded(eng_w0, world):
    """The device-resident multi-GPU entry points with SEVERAL ranks on one GPU (loop-back communicator, see _loopback_engines):
    embed_sharded_dev with equal, ragged and fewer-crops-than-ranks shards (reid_allgather_dev / reid_allgather_rows_dev: counts,
    padded payload, compaction), each rank's row block of the distance matrix, and reid_knn_gallery_sharded_dev with
    index_base > 0, empty shards, k larger than a shard and ties across shards - every rank must hold exactly what a
    single-context run produces."""
    from reid_amd import parallel
    eng, sd = eng_w0
    engs = _loopback_engines(world, sd)
    try:
        rng = np.random.default_rng(11)
        xb = rng.normal(size=(203, 64)).astype(np.float32)
        xb[150] = xb[7]                                                   # the same row in two shards: lowest global index first
        xq = np.concatenate([xb[:20] + 0.01 * rng.normal(size=(20, 64)).astype(np.float32), xb[7:8]], 0)
        want_knn = eng.knn(xq, xb, 9)
        want_small = eng.knn(xq, xb[:3], 3)
        crop_sets = {n: synth.smooth_crops_u8(n, 30 + n) for n in (world * 3, world * 3 + 1, max(1, world - 1))}
        want_emb = {n: eng.embed_u8(c) for n, c in crop_sets.items()}

        def rank_fn(r):
            e = engs[r]
            comm = parallel.RcclComm.attach(e)
            assert (comm.rank, comm.world) == (r, world)
            out = {}
            for n, crops in crop_sets.items():
                emb_all, (lo, hi) = parallel.embed_sharded(e, crops, comm)
                out["emb%d" % n] = emb_all.numpy()
                out["blk%d" % n] = parallel.distmat_row_block(e, emb_all, lo, hi, _ffi.METRIC_L2).numpy()
                out["lohi%d" % n] = (lo, hi)
            out["knn"] = parallel.knn_gallery_sharded(e, xq, xb, 9, comm)
            out["knn_small"] = parallel.knn_gallery_sharded(e, xq, xb[:3], 5, comm)      # most shards empty, k > gallery
            assert comm.all_reduce([float(r), 1.0], "sum").tolist() == [world * (world - 1) / 2.0, float(world)]
            assert comm.all_reduce([float(r)], "max").tolist() == [world - 1.0]
            return out

        res = _run_ranks(world, rank_fn)
        for r, out in enumerate(res):
            for n in crop_sets:
                # gather order = crop order; a shard is a smaller batch than the whole set, and small launches split K differently:
                # equal up to fp32 summation order (the same bound as the rebatching check of the embed test), identical on all ranks
                np.testing.assert_allclose(out["emb%d" % n], want_emb[n], rtol=1e-6, atol=1e-6 * np.abs(want_emb[n]).max(), err_msg=str((r, n)))
                assert np.array_equal(out["emb%d" % n], res[0]["emb%d" % n]), (r, n)
                lo, hi = out["lohi%d" % n]
                assert (lo, hi) == parallel.shard_bounds(n, world, r)
                if hi > lo:
                    mine = out["emb%d" % n]
                    assert np.array_equal(out["blk%d" % n], eng.distmat(mine[lo:hi], mine, _ffi.METRIC_L2))
            D, I = out["knn"]
            assert np.array_equal(I, want_knn[1]) and np.array_equal(D, want_knn[0])
            assert I[20, 0] == 7 and I[20, 1] == 150                                  # the cross-shard tie
            Ds, Is = out["knn_small"]
            assert np.array_equal(Is[:, :3], want_small[1]) and np.array_equal(Ds[:, :3], want_small[0])
            assert (Is[:, 3:] == -1).all() and np.isinf(Ds[:, 3:]).all()
    finally:
        for e in engs:
            e.close()


@pytest.mark.timeout(600)
@pytest.mark.parametrize("world", [2, 8])
def test_loopback_ranks_tracking_frames(eng_w0, world):
    """tracking.ShardedCameraStream with several ranks on one GPU: round-robin shares, reid_frame_gather (equal blocks, zeroed
    padding rows), costs over the gathered slot, bank updates from gathered rows - against the single-context CameraStream
    flow on the same frames (frames of 0, 1, world - 1, world + 1 ... detections)."""
    from reid_amd import parallel
    from reid_amd.nn_matching import NearestNeighborDistanceMetric
    from reid_amd.tracking import ShardedCameraStream
    eng, sd = eng_w0
    engs = _loopback_engines(world, sd)
    try:
        rng = np.random.default_rng(12)
        counts = [5, 0, 1, world - 1, world + 1, 13, 2 * world, 3]
        pool = synth.ragged_crops_u8(24, seed=9)
        frames = [[pool[(7 * f + i) % 24] for i in range(n)] for f, n in enumerate(counts)]
        tracks = [3, 5, 8, 9]
        boxes = rng.uniform(0, 400, (2 * world + 14, 4))
        boxes[:, 2:] = rng.uniform(15, 100, (len(boxes), 2))
        seed_feats = rng.normal(size=(8, 512)).astype(np.float32)
        seed_feats /= np.linalg.norm(seed_feats, axis=1, keepdims=True)

        def drive(stream, step):
            stream.metric.partial_fit(seed_feats, np.repeat(tracks, 2), tracks)
            out = []
            stream.submit(frames[0])
            for f, cr in enumerate(frames):
                n = len(cr)
                feats, cost, icost = step(stream, n, frames[f + 1] if f + 1 < len(frames) else None)
                out.append((feats, cost, icost))
                k = min(n, len(tracks))
                stream.commit(np.arange(k)[::-1], tracks[:k], tracks)
            stream.close()
            return out

        import types
        one = ShardedCameraStream(eng, types.SimpleNamespace(rank=0, world=1), 0.4, budget=3, max_tracks=16)   # no communicator
        try:
            want = drive(one, lambda st, n, nxt: st.step(n, tracks, boxes[:4], boxes[:n], nxt))
        finally:
            one.metric.close()

        def rank_fn(r):
            st = ShardedCameraStream(engs[r], parallel.RcclComm.attach(engs[r]), 0.4, budget=3, max_tracks=16,
                                      match_stream=(r % 2 == 0))     # both forms of the cost / update stages behind the all-gather
            try:
                return drive(st, lambda s, n, nxt: s.step(n, tracks, boxes[:4], boxes[:n], nxt))
            finally:
                st.metric.close()

        res = _run_ranks(world, rank_fn)
        for r, got in enumerate(res):
            for f, ((gf, gc, gi), (wf, wc, wi)) in enumerate(zip(got, want)):
                assert gf.shape == wf.shape and gc.shape == wc.shape, (r, f)
                assert np.isfinite(gc).all()
                if gf.size:                                              # a share is a smaller batch: equal up to fp32 summation order
                    np.testing.assert_allclose(gf, wf, rtol=1e-6, atol=1e-6 * np.abs(wf).max(), err_msg="rank %d frame %d" % (r, f))
                    assert np.array_equal(gf, res[0][f][0]), (r, f)      # and the same bits on every rank
                np.testing.assert_allclose(gc, wc, rtol=0, atol=2e-6, err_msg="rank %d frame %d" % (r, f))
                if wi is not None:
                    assert np.array_equal(gi, wi), (r, f)
    finally:
        for e in engs:
            e.close()


def test_sharded_search_without_a_communicator_is_refused(eng):
    """a context without a communicator that is handed a shard starting at row > 0 must not answer with that
    shard alone."""
    from reid_amd import parallel
    x = np.random.default_rng(1).normal(size=(12, 16)).astype(np.float32)
    dq, db = parallel.DevArray.from_numpy(eng, x[:3]), parallel.DevArray.from_numpy(eng, x)
    dD, dI = parallel.DevArray(eng, (3, 2)), parallel.DevArray(eng, (3, 2), np.int32)
    with pytest.raises(_ffi.ReidHipError, match="index_base"):
        parallel.knn_gallery_sharded_dev(eng, dq.ptr, 3, db.ptr, 12, 6, 16, 2, dD.ptr, dI.ptr)
    with pytest.raises(RuntimeError, match="spans 1"):
        parallel.knn_gallery_sharded_dev(eng, dq.ptr, 3, db.ptr, 12, 0, 16, 2, dD.ptr, dI.ptr, world=2)
    parallel.knn_gallery_sharded_dev(eng, dq.ptr, 3, db.ptr, 12, 0, 16, 2, dD.ptr, dI.ptr, world=1)
    assert np.array_equal(dI.numpy(), eng.knn(x[:3], x, 2)[1])


def test_rccl_single_rank_communicator_and_device_resident_sharding(eng_w0):
    """The RCCL branch of parallel.py with a REAL 1-rank communicator (ncclCommInitRank with nranks = 1): every collective goes
    through librccl, the sharded entry points stay in HBM, and the results equal the plain single-process calls."""
    from reid_amd import parallel
    eng, _ = eng_w0
    comm = parallel.RcclComm(eng, 0, 1, parallel.RcclComm.unique_id())
    try:
        assert comm.all_reduce([3.0, -1.0], "max").tolist() == [3.0, -1.0]
        comm.barrier()
        x = np.random.default_rng(3).normal(size=(37, 512)).astype(np.float32)
        dx = parallel.DevArray.from_numpy(eng, x)
        dy = parallel.DevArray(eng, x.shape)
        comm.all_gather(dx.ptr, dy.ptr, x.nbytes)                       # ncclAllGather, one rank
        assert np.array_equal(dy.numpy(), x)
        dz = parallel.DevArray(eng, x.shape)
        assert comm.all_gather_rows(dx.ptr, 37, 512 * 4, dz.ptr) == [37]
        assert np.array_equal(dz.numpy(), x)
        crops = synth.smooth_crops_u8(9, 3)
        emb_all, (lo, hi) = parallel.embed_sharded(eng, crops, comm=comm)   # DevArray, never on the host
        assert (lo, hi) == (0, 9) and isinstance(emb_all, parallel.DevArray)
        want = eng.embed_u8(crops)
        assert np.array_equal(emb_all.numpy(), want)
        block = parallel.distmat_row_block(eng, emb_all, 2, 7, _ffi.METRIC_L2)
        assert np.array_equal(block.numpy(), eng.distmat(want[2:7], want, _ffi.METRIC_L2))
        # the frame pipeline's device-side gather (reid_frame_gather) through the 1-rank communicator: one block of per rows
        from reid_amd.nn_matching import NearestNeighborDistanceMetric
        fc = synth.ragged_crops_u8(5, seed=2)
        metric = NearestNeighborDistanceMetric("cosine", 0.5, 3, max_tracks=4)
        want_f = eng.embed_ragged_u8(fc)
        metric.partial_fit(want_f[:2], [1, 2], [1, 2])
        rows, per = parallel.frame_rows(5, 1)
        eng.frame_submit(0, fc)
        eng.frame_gather(0, per, 1)
        feats, cost, _ = metric.frame_distance(0, [1, 2], max_distance=0.5)
        np.testing.assert_array_equal(feats[rows], want_f)
        np.testing.assert_array_equal(cost[:, rows], metric.distance(want_f, [1, 2], max_distance=0.5))
        metric.close()
        xb = np.random.default_rng(6).normal(size=(301, 64)).astype(np.float32)
        xq = xb[:11] + 0.01
        D, I = parallel.knn_gallery_sharded(eng, xq, xb, 7, comm=comm)
        Dr, Ir = eng.knn(xq, xb, 7)
        assert np.array_equal(I, Ir) and np.array_equal(D, Dr)
    finally:
        comm.close()
    # without a communicator the same calls are local copies
    solo = parallel.RcclComm(eng, 0, 1, None)
    try:
        D2, I2 = parallel.knn_gallery_sharded(eng, xq, xb, 7, comm=solo)
        assert np.array_equal(I2, Ir)
    finally:
        solo.close()


@pytest.mark.parametrize("world,kk,k", [(2, 5, 5), (8, 20, 20), (3, 4, 6)])
def test_device_knn_merge_equals_host_merge(eng, world, kk, k):
    """The merge kernel of reid_knn_gallery_sharded_dev on virtual shards: equal distances across shards (ties -> lowest global
    row), -1 padding of short shards, fewer candidates than k."""
    import ctypes as C
    from reid_amd import parallel
    rng = np.random.default_rng(world * 100 + k)
    nq = 13
    D = np.sort(rng.integers(0, 6, (world, nq, kk)).astype(np.float32) * 0.25, axis=2)      # many exact ties
    I = rng.permutation(world * nq * kk).reshape(world, nq, kk).astype(np.int32)
    I[-1, :, kk - 2:] = -1                                                                   # a short last shard
    D[-1, :, kk - 2:] = np.inf
    outD, outI = np.empty((nq, k), np.float32), np.empty((nq, k), np.int32)
    fn = _ffi.debug_lib().reid_debug_knn_merge
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    _ffi.check(fn(eng.h, D.ctypes.data, I.ctypes.data, world, nq, kk, k, outD.ctypes.data, outI.ctypes.data))
    wantD, wantI = parallel.merge_topk(list(D), list(I), k)
    assert np.array_equal(outI, wantI)
    assert np.array_equal(outD, wantD)


# ----------------------------------------------------------------------------- plugin surface on the device
def test_build_model_warmup_and_cuda_tensor_entry(eng_w0):
    """What track_yolov5.py:167-171 does with the object build_model returns: .to(device).eval(), warmup(), then
    model(cuda_batch) every frame.  A CUDA tensor goes through the device entry point on torch's current stream (no host
    round trip: the result is a CUDA tensor) and equals the numpy entry bit for bit; fp16 CUDA batches are widened on entry."""
    from reid_amd.models import build_model
    eng, sd = eng_w0
    model = build_model("seres18_ibn", num_classes=751, loss="triplet", pretrained=False, use_gpu=True)
    model.load_state_dict(sd, strict=True)
    model = model.to("cuda:0").eval().half()
    assert model.warmup() is model                                      # no-arg warmup(): one dummy batch
    x = seres18.preprocess_u8(synth.smooth_crops_u8(6, 21))              # float32 [6,3,256,128]
    want = model(x.numpy())
    xc = x.cuda()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):                                          # a non-default current stream, as a tracker thread may have
        got = model(xc)
        e2, lg = model(xc.half(), return_logits=True)
    s.synchronize()
    got0 = model(xc)                                                    # torch's DEFAULT stream (the HIP null stream, handle 0)
    assert np.array_equal(got0.cpu().numpy(), want)                     # .cpu() orders itself after the kernels on that stream
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (6, 512)
    assert np.array_equal(got.cpu().numpy(), want)
    assert lg.is_cuda and tuple(lg.shape) == (6, 751)
    cos = F.cosine_similarity(e2.float().cpu(), torch.from_numpy(want), dim=1)
    assert float((1 - cos).max()) < 1e-5                                # inputs rounded to fp16, arithmetic still fp32
    # host call right after a device call on another stream: the engine drains the old stream before it switches
    eng.set_stream(None)
    assert model.precision == os.environ.get("REID_PRECISION", "f16x3") and eng.precision == 0   # the model's arithmetic is its own:
    eng.set_precision({"f32": 0, "f16": 1, "f16x3": 2}[model.precision])                      # the shared engine kept the mode it had
    try:
        assert np.array_equal(eng.embed_f32_nchw(x.numpy()), want)
    finally:
        eng.set_precision(0)


_EXTRACTOR_FROM_FILE = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
from reid_amd import _ffi, synth
from reid_amd.extractor import Extractor
assert _ffi._lib is None and "torch" not in sys.modules          # importing the plugin loads neither torch nor the library
ext = Extractor(sys.argv[2], use_cuda=True)                        # feature_extractor.py:15: (model_path, use_cuda=True)
emb = ext(synth.ragged_crops_u8(5, seed=11))
hip = sorted({ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln})
print(json.dumps({"emb": emb.tolist(), "precision": ext.precision, "hip_runtimes": hip}))
"""


@pytest.mark.timeout(600)
def test_extractor_from_a_checkpoint_file_in_a_fresh_process(eng_w0, tmp_path):
    """The reference's actual constructor, ``Extractor(model_path: str, use_cuda=True)`` (modification_deepsort/
    feature_extractor.py:15-19: torch.load + load_state_dict(strict=False)), on a checkpoint FILE as the trainer writes it
    (saved from DataParallel: "module." prefix, image_reid_train.py:111,635), in a process that has imported nothing before:
    torch reads the file BEFORE the engine loads libreid_hip.so, so the process holds ONE HIP runtime (the other order loads
    torch's bundled libamdhip64 beside /opt/rocm's and aborts in the exit handlers), the call returns the
    embeddings of the in-process extractor bit for bit, in the plugin's default arithmetic, and the interpreter exits 0."""
    import json
    import subprocess
    import sys
    from reid_amd.extractor import Extractor
    eng, sd = eng_w0
    path = tmp_path / "ckpt.t7"
    torch.save({"module." + k: torch.from_numpy(np.array(v)) for k, v in sd.items()}, str(path))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k != "REID_PRECISION"}
    r = subprocess.run([sys.executable, "-c", _EXTRACTOR_FROM_FILE, root, str(path)], capture_output=True, text=True, env=env, timeout=500)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "double free" not in r.stderr and "corruption" not in r.stderr
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["precision"] == "f16x3" and len(d["hip_runtimes"]) == 1, d["hip_runtimes"]
    got = np.asarray(d["emb"], np.float32)
    crops = synth.ragged_crops_u8(5, seed=11)
    assert np.array_equal(got, Extractor(sd, precision="f16x3")(crops))
    want = seres18.forward(sd, torch.from_numpy(matching.preprocess(crops)))[0].numpy()
    cos = (got * want).sum(1) / np.linalg.norm(got, axis=1) / np.linalg.norm(want, axis=1)
    assert (1 - cos).max() < 1e-5


def test_plugin_precision_argument_environment_and_fallback(eng_w0, caplog, monkeypatch):
    """The plugin objects run in the arithmetic bench.py reports unless told otherwise: precision= argument > $REID_PRECISION >
    "f16x3"; their mode is applied per call and the shared engine keeps the mode other callers gave it.  A checkpoint the
    fp32-class mode refuses (a weight it cannot split: at load; an activation outside f16: through the fault word, at the first
    call) runs in exact fp32 from then on - same numbers as precision="f32" - with ONE log line."""
    import logging
    from reid_amd import models
    from reid_amd.extractor import Extractor
    eng, sd = eng_w0
    crops = synth.ragged_crops_u8(4, seed=5)
    monkeypatch.delenv("REID_PRECISION", raising=False)
    e2, e0 = Extractor(sd), Extractor(sd, precision="f32")
    assert (e2.precision, e0.precision) == ("f16x3", "f32")
    a2, a0 = e2(crops), e0(crops)
    assert eng.precision == 0 and not np.array_equal(a2, a0) and np.abs(a2 - a0).max() <= 2e-5 * np.abs(a0).max()
    eng.set_precision(2)
    try:
        b0 = eng.embed_ragged_u8(crops)          # the extractors left the weights of e0 bound (same checkpoint) and the engine's mode alone
        assert np.array_equal(b0, a2) and np.array_equal(e0(crops), a0) and eng.precision == 2
    finally:
        eng.set_precision(0)
    monkeypatch.setenv("REID_PRECISION", "f32")
    assert Extractor(sd).precision == "f32" and models.build_model("seres18_ibn", 751, loss="triplet", pretrained=False).precision == "f32"
    assert models.build_model("swin_transformer", 751, pretrained=False, precision=1).precision == "f16"
    monkeypatch.delenv("REID_PRECISION")
    with pytest.raises(ValueError):
        Extractor(sd, precision="bf16")
    # (1) weights outside the split range: refused when the mode is selected -> fall back at construction
    bad = dict(sd)
    bad["basicBlock31.block_pre.conv2.weight"] = np.array(sd["basicBlock31.block_pre.conv2.weight"], copy=True)
    bad["basicBlock31.block_pre.conv2.weight"][3, 5, 1, 1] = 40.0
    try:
        with caplog.at_level(logging.WARNING, logger="root.tracker"):
            caplog.clear()
            eb = Extractor(bad)
            assert eb.precision == "f32"
            got = eb(crops)
            got2 = eb(crops)
        lines = [r for r in caplog.records if "fp32-class" in r.getMessage()]
        assert len(lines) == 1 and "b31.conv2.w" in lines[0].getMessage()
        assert np.array_equal(got, Extractor(bad, precision="f32")(crops)) and np.array_equal(got, got2)
        # (2) an activation outside f16's range: the fault word at the first call -> cleared, exact fp32, same call answered
        hot = dict(sd)
        hot["bn0.weight"] = np.asarray(sd["bn0.weight"]) * 1e7
        with caplog.at_level(logging.WARNING, logger="root.tracker"):
            caplog.clear()
            m = models.build_model("seres18_ibn", 751, loss="triplet", pretrained=False)
            m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in hot.items()}, strict=True)
            assert m.precision == "f16x3"
            out = m.embed_crops(crops)
            assert m.precision == "f32" and np.isfinite(out).all()
            out2 = m.embed_crops(crops)
        assert len([r for r in caplog.records if "fp32-class" in r.getMessage()]) == 1
        assert np.array_equal(out, out2) and np.array_equal(out, Extractor(hot, precision="f32")(crops))
        eng.sync()                                # no fault left pending
        # (3) the shared engine holds BOTH backbones' weights: a Swin checkpoint the fp32-class mode refuses must not cost an
        # extractor with a good ResNet checkpoint its mode for good (round-5 advice) - while the bad Swin weights are loaded the
        # extractor's calls run in exact fp32 (one log line that says why), its own mode stays "f16x3", and it is back on the
        # fp32-class arithmetic as soon as a splittable Swin checkpoint replaces the bad one
        sw_sd = synth.swin_state_dict(0)
        sw_bad = dict(sw_sd)
        key = next(k for k in sw_sd if k.endswith("to_qkv.weight"))
        sw_bad[key] = np.array(sw_sd[key], copy=True)
        sw_bad[key][0, 0] = 50.0
        eng.load_swin(*weights.pack_swin(sw_bad)[:2])
        assert eng.precision_ok(0, 2) and not eng.precision_ok(1, 2)
        with caplog.at_level(logging.WARNING, logger="root.tracker"):
            caplog.clear()
            shared = e2(crops)
            shared2 = e2(crops)
        assert e2.precision == "f16x3" and np.array_equal(shared, a0) and np.array_equal(shared2, a0)
        assert len([r for r in caplog.records if "another model" in r.getMessage()]) == 1
        eng.load_swin(*weights.pack_swin(sw_sd)[:2])
        assert np.array_equal(e2(crops), a2)
        # ... and a fault word that was already up when a call began is not this call's to clear
        assert eng.fault_bits() == 0
    finally:
        eng.clear_fault()
        eng.set_precision(0)
        eng.load_seres18(*weights.pack_seres18(sd)[:2])


def test_swin_cuda_tensor_entry(eng):
    from reid_amd.models import build_model
    model = build_model("swin_transformer", num_classes=751, loss="softmax", pretrained=False, use_gpu=True).to("cuda").eval()
    model.warmup()
    x = synth.images_f32(2, 3)
    want = model(x)
    got = model(torch.from_numpy(x).cuda())
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    eng.set_stream(None)


def test_cam_debias_rejects_non_finite_rows(eng):
    x = np.random.default_rng(0).normal(size=(40, 32)).astype(np.float32)
    x[3, 5] = np.nan
    with pytest.raises(_ffi.ReidHipError, match="non-finite"):
        eng.cam_debias(x, np.zeros(40, np.int32))


def test_smooth_tracklets_matches_reference_fixture(eng, golden_dir):
    """reid_smooth_tracklets against the reference's own smooth_tracklets output (tests/golden/postproc.npz, st_* keys)."""
    from reid_amd import inference_utils
    z = np.load(os.path.join(golden_dir, "postproc.npz"))
    got = eng.smooth_tracklets(z["st_x"], z["st_seq"], z["st_valid"])
    np.testing.assert_allclose(got, z["st_out"], rtol=0, atol=2e-6)       # the mean is summed in row order, torch's in a tree
    assert np.array_equal(got[~z["st_valid"]], z["st_x"][~z["st_valid"]])
    t = torch.from_numpy(z["st_x"].copy())
    assert inference_utils.smooth_tracklets(t, torch.from_numpy(z["st_seq"]), torch.from_numpy(z["st_valid"])) is t   # in place
    np.testing.assert_allclose(t.numpy(), z["st_out"], rtol=0, atol=2e-6)
    assert eng.smooth_tracklets(np.zeros((0, 8), np.float32), np.zeros(0, np.int32)).shape == (0, 8)
    wide = np.random.default_rng(1).normal(size=(50, 1263)).astype(np.float32)      # descriptor width of the evaluation script
    from oracle import postproc
    seq = np.arange(50) % 4
    np.testing.assert_allclose(eng.smooth_tracklets(wide, seq), postproc.smooth_tracklets(wide, seq, np.ones(50, bool)), atol=2e-6)


@pytest.mark.parametrize("precision,tol", [(0, 2e-5), (1, 2e-2), (2, 2e-5)])
def test_swin_stage_taps_match_reference_fixture(eng, golden_dir, precision, tol):
    """Stage-level localisation for Swin, from the taps the REFERENCE's swin_t produced (tests/golden/swin_seed0.npz): the
    ShadowFeatureExtraction output, the four stage outputs and the GeM_1D output, sampled exactly as gen_golden.py sampled them.
    fp32 mode within 2e-5 of the stage's range; fp16-storage mode within 2e-2 (its residual stream is fp32, its linears f16);
    precision 2 (the linears in fp32-class arithmetic on the f16 matrix pipe) is held to the fp32 mode's 2e-5."""
    g = np.load(os.path.join(golden_dir, "swin_seed0.npz"))
    seed, n = int(g["seed"]), int(g["n"])
    eng.load_swin(*weights.pack_swin(synth.swin_state_dict(seed))[:2])
    eng.set_precision(precision)
    try:
        eng.swin_embed_f32_nchw(synth.images_f32(n, seed))
        for stage, name in ((0, "sfe"), (1, "stage1"), (2, "stage2"), (3, "stage3"), (4, "stage4")):
            t = torch.from_numpy(eng.debug_swin_stage(stage, n)).permute(0, 3, 1, 2)          # NHWC -> the reference's NCHW
            c, h, w = t.shape[1:]
            got = t[:, :: max(1, c // 8), :: max(1, h // 8), :: max(1, w // 4)].numpy()
            ref = g["tap_" + name]
            assert np.abs(got - ref).max() <= tol * np.abs(ref).max(), (name, np.abs(got - ref).max(), np.abs(ref).max())
            assert abs(float(t.double().mean()) - float(g["mean_" + name])) <= tol * float(g["absmean_" + name]), name
        gem = eng.debug_swin_stage(5, n)[:, :: 96 // 8]                    # the fixture keeps every 12th channel of [n,96,1]
        ref = g["tap_avgpool"].reshape(gem.shape)
        assert np.abs(gem - ref).max() <= tol * np.abs(ref).max()
    finally:
        eng.set_precision(0)


def test_swin_window_attention_mfma_equals_valu_kernel(eng):
    """The matrix-core window attention (S^T = K.Q^T, softmax in the accumulator layout, P.V with the accumulator tile as the
    MFMA operand) against round 1's one-lane-per-query VALU kernel (debug switch swin_attn_mfma = 0), both arithmetic modes, on
    448x224 so that shifted blocks see inner windows as well as the masked last row / column.  The switches are fields of the
    context that only libreid_hip_debug.so can move (reid_debug_set_switch); the product library reads none of them from the
    environment."""
    eng.load_swin(*weights.pack_swin(synth.swin_state_dict(0))[:2])
    x = synth.images_f32(3, 9, h=448, w=224)

    def run(mode, **switches):
        for k, v in switches.items():
            eng.debug_switch(k, v)
        eng.set_precision(mode)
        try:
            return eng.swin_embed_f32_nchw(x)
        finally:
            eng.set_precision(0)

    try:
        res = {m: (run(0, swin_attn_mfma=m), run(1, swin_attn_mfma=m)) for m in (0, 2)}   # 0 = VALU kernel in both modes, 2 = matrix cores in both
        for i, tol in ((0, 2e-5), (1, 2e-3)):
            a, b = res[0][i], res[2][i]
            assert np.abs(a - b).max() <= tol * np.abs(a).max(), (i, np.abs(a - b).max(), np.abs(a).max())
        eng.debug_switch("swin_attn_mfma", 1)
        # fp32-class mode: the split-operand matrix-core kernel (opt-in switch swin_attn_split: measured 5 % slower end to end than the
        # exact-fp32 VALU kernel it would replace) gives that kernel's result at the mode's own error level
        r0, r1 = run(2, swin_attn_split=0), run(2, swin_attn_split=1)
        assert not np.array_equal(r0, r1)                                   # the switch did select the other kernel
        assert np.abs(r0 - r1).max() <= 4e-6 * np.abs(r0).max(), np.abs(r0 - r1).max() / np.abs(r0).max()
    finally:
        eng.debug_switch("swin_attn_mfma", 1)
        eng.debug_switch("swin_attn_split", 0)
        with pytest.raises(_ffi.ReidHipError):
            eng.debug_switch("no_such_switch", 1)


# ----------------------------------------------------------------------------- sibling backbones
@pytest.mark.parametrize("precision", [0, 2])
@pytest.mark.parametrize("tag,name,sd_fn", [("ca", "cares18_ibn", synth.cares18_state_dict), ("ema", "emares18_ibn", synth.emares18_state_dict)])
def test_sibling_backbones_match_reference_fixture(eng, golden_dir, tag, name, sd_fn, precision):
    """CARes18_IBN (TripletAttention blocks) and EMARes18_IBN (EMA blocks) on the ResNet18-IBN conv kernels, against the embeddings,
    logits and per-block outputs the REFERENCE's own classes produced (tests/golden/siblings.npz); precision 2 = the same with the
    3x3 convolutions in fp32-class arithmetic on the f16 matrix pipe, same thresholds."""
    eng.set_precision(precision)
    try:
        _sibling_check(eng, golden_dir, tag, name, sd_fn, precision)
    finally:
        eng.set_precision(0)


def _sibling_check(eng, golden_dir, tag, name, sd_fn, precision):
    from reid_amd.models import build_model
    g = np.load(os.path.join(golden_dir, "siblings.npz"))
    model = build_model(name, num_classes=751, loss="triplet", pretrained=False, use_gpu=True, precision=precision)
    assert list(model.state_dict().keys()) == list(sd_fn(0).keys())       # the reference's own key layout (positional in downsample blocks)
    model.load_state_dict(sd_fn(0), strict=True)
    x = seres18.preprocess_u8(synth.smooth_crops_u8(3, 7)).numpy()
    eng.debug_keep(1)
    try:
        emb, logits = model(x, return_logits=True)
        for i, blk in enumerate(b[0] for b in synth.SERES18_BLOCKS):
            c, (h, w) = [64, 64, 128, 128, 256, 256, 512, 512][i], [(64, 32), (64, 32), (32, 16), (32, 16), (16, 8), (16, 8), (16, 8), (16, 8)][i]
            t = torch.from_numpy(eng.debug_stage(2 + i, 3).reshape(3, h, w, c)).permute(0, 3, 1, 2)
            got = t[:, :: max(1, c // 8), :: max(1, h // 8), :: max(1, w // 4)].numpy()
            ref = g["%s_tap_%s" % (tag, blk)]
            assert np.abs(got - ref).max() <= 2e-5 * np.abs(ref).max(), (blk, np.abs(got - ref).max(), np.abs(ref).max())
    finally:
        eng.debug_keep(0)
    cos = (emb * g[tag + "_emb"]).sum(1) / np.linalg.norm(emb, axis=1) / np.linalg.norm(g[tag + "_emb"], axis=1)
    assert (1 - cos).max() < 1e-5
    assert np.abs(emb - g[tag + "_emb"]).max() <= 2e-5 * np.abs(g[tag + "_emb"]).max()
    assert np.abs(logits - g[tag + "_logits"]).max() <= 5e-5 * np.abs(g[tag + "_logits"]).max()
    # other batch sizes go through the same kernels: a single crop, and the crops inside a larger batch
    e1 = model(x[:1])
    assert np.abs(e1 - emb[:1]).max() <= 2e-5 * np.abs(emb).max()


# ----------------------------------------------------------------------------- evaluation harness (SURVEY 8c harness row)
def test_e2e_harness_matches_reference_chain(eng_w0, golden_dir):
    """reid_amd.reid_inference.evaluate_reid - descriptor + flip-TTA -> camera de-biasing -> Jaccard re-ranking -> DBSCAN
    (host, scikit-learn as in the reference) -> tracklet smoothing -> CMC / mAP, device-resident between the links - against
    tests/golden/e2e.npz: the same chain run by gen_golden.gen_e2e through the reference's own classes and functions
    (image_reid_inference.py:238-322) on the same seeded 300-image gallery + 60 queries."""
    from reid_amd import reid_inference
    eng, _ = eng_w0
    g = np.load(os.path.join(golden_dir, "e2e.npz"))
    step = int(g["row_step"])
    prob = synth.e2e_problem()
    taps = {}
    cmc, mean_ap = reid_inference.evaluate_reid(prob["g_img"], prob["gl"], prob["gc"], prob["gs"], prob["q_img"], prob["ql"],
                                                prob["qc"], prob["qs"], num_gallery_cams=4, eps=float(g["eps"]), taps=taps,
                                                verbose=False, engine=eng)
    np.testing.assert_allclose(taps["desc"][::step], g["desc"], atol=2e-5)          # unit rows: absolute = relative to the norm
    np.testing.assert_allclose(taps["debiased"][::step], g["debiased"], atol=5e-5)
    np.testing.assert_allclose(taps["jaccard"][::step], g["jaccard"], atol=2e-4)
    # eps sits in the middle of the widest gap of the reference's distances (margin 1e-3 >> 2e-4): same neighbourhoods, same labels
    assert (taps["pseudo_labels"] == g["pseudo_labels"]).all()
    np.testing.assert_allclose(taps["smoothed"][::step], g["smoothed"], atol=5e-5)
    np.testing.assert_array_equal(cmc, g["cmc"])
    assert abs(mean_ap - float(g["map"])) < 1e-6
    # the clustering hook: handing the reference's labels in gives the same result without scikit-learn
    cmc2, map2 = reid_inference.evaluate_reid(prob["g_img"], prob["gl"], prob["gc"], prob["gs"], prob["q_img"], prob["ql"],
                                              prob["qc"], prob["qs"], cluster_fn=lambda d: g["pseudo_labels"], verbose=False,
                                              engine=eng)
    np.testing.assert_array_equal(cmc2, cmc)
    assert map2 == mean_ap


# ----------------------------------------------------------------------------- --renorm checkpoints
def test_renorm_checkpoint_matches_reference_fixture(eng, golden_dir):
    """A checkpoint in the --renorm layout (every BatchNorm2d a BatchRenormalization2D: gamma / beta / running_avg_* [1,C,1,1],
    SERes18_IBN.py:102-113,203-204, batchrenorm.py:26-40) through weights.pack_seres18 and through the model object, against
    the reference's own seres18_ibn(renorm=True) in eval mode (tests/golden/renorm.npz)."""
    from reid_amd import models
    g = np.load(os.path.join(golden_dir, "renorm.npz"))
    rsd = synth.renorm_state_dict(synth.seres18_state_dict(2))
    crops = synth.smooth_crops_u8(4, 8)
    blob, manifest, _ = weights.pack_seres18({"module." + k: v for k, v in rsd.items()})     # as the trainer saves it
    eng.load_seres18(blob, manifest)
    emb, logits = eng.embed_u8(crops, logits=True)
    for mine, ref in ((emb, g["emb"]), (logits, g["logits"])):
        assert np.abs(mine - ref).max() / np.abs(ref).max() < 5e-5
    cos = (emb * g["emb"]).sum(1) / np.linalg.norm(emb, axis=1) / np.linalg.norm(g["emb"], axis=1)
    assert (1 - cos).max() < 1e-5
    m = models.build_model("seres18_ibn", num_classes=751, loss="triplet", pretrained=False).eval()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in rsd.items()}, strict=True)
    out = m(seres18.preprocess_u8(crops))
    assert np.abs(out.numpy() - g["emb"]).max() / np.abs(g["emb"]).max() < 5e-5


# ----------------------------------------------------------------------------- optional side-information branches
@pytest.mark.parametrize("precision", [0, 1, 2])
def test_camera_bias_and_view_embedding_match_reference_fixture(eng, golden_dir, precision):
    """SERse18_IBN.forward(x, cam) (SERes18_IBN.py:269-271) and SwinTransformer.forward(img, view_index) of a model built with
    camera = 4 (swin_transformer.py:285-302), against what the reference's own classes returned (tests/golden/side.npz):
    through the C ABI (reid_ctx_set_side_index + embed) and through the model objects; chunked passes consume the indices in
    order; a bad index or a count mismatch is an error and leaves nothing pending."""
    from reid_amd import models
    g = np.load(os.path.join(golden_dir, "side.npz"))
    tol, ctol = (5e-5, 1e-5) if precision != 1 else (2e-2, 1e-4)
    sd = synth.seres18_state_dict(3)
    crops = synth.smooth_crops_u8(4, 11)
    eng.load_seres18(*weights.pack_seres18(sd)[:2])
    eng.set_precision(precision)
    try:
        eng.set_chunk(3)                                   # two passes: 3 + 1 images
        eng.set_side_index(g["cam"])
        emb, logits = eng.embed_u8(crops, logits=True)
        for mine, ref in ((emb, g["emb"]), (logits, g["logits"])):
            assert np.abs(mine - ref).max() / np.abs(ref).max() < tol
        plain = eng.embed_u8(crops)                        # the indices were consumed: no bias now
        assert np.abs(plain - emb).max() > 1e-2
        np.testing.assert_allclose(emb - plain, -1.0 * sd["cam_bias"][g["cam"]], atol=2e-5 * np.abs(emb).max())
        eng.set_side_index([0, 1, 6, 2])                   # 6 cameras: index 6 is outside the table
        with pytest.raises(_ffi.ReidHipError):
            eng.embed_u8(crops)
        eng.set_side_index([0, 1])                         # fewer indices than images
        with pytest.raises(_ffi.ReidHipError):
            eng.embed_u8(crops)
        np.testing.assert_array_equal(eng.embed_u8(crops), plain)      # nothing left pending after the errors
        eng.set_chunk(1024)
        m = models.build_model("seres18_ibn", num_classes=751, loss="triplet", pretrained=False, precision=precision).eval()
        m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
        out, lg = m(seres18.preprocess_u8(crops), cam=torch.from_numpy(g["cam"]), return_logits=True)
        assert np.abs(out.numpy() - g["emb"]).max() / np.abs(g["emb"]).max() < tol
        assert np.abs(lg.numpy() - g["logits"]).max() / np.abs(g["logits"]).max() < tol
        # Swin with a side-information table of 4 views
        ssd = synth.swin_state_dict(4, views=4)
        img = synth.images_f32(3, 4)
        eng.load_swin(*weights.pack_swin(ssd)[:2])
        eng.set_side_index(g["view"])
        semb, slog = eng.swin_embed_f32_nchw(img, logits=True)
        assert np.abs(semb - g["swin_emb"]).max() / np.abs(g["swin_emb"]).max() < (2e-4 if precision != 1 else 2e-2)
        assert np.abs(slog - g["swin_logits"]).max() / np.abs(g["swin_logits"]).max() < (2e-4 if precision != 1 else 2e-2)
        cos = (semb * g["swin_emb"]).sum(1) / np.linalg.norm(semb, axis=1) / np.linalg.norm(g["swin_emb"], axis=1)
        assert (1 - cos).max() < ctol
        from reid_amd import backbone
        sm = backbone.swin_t(num_classes=751, loss="triplet", pretrained=False, camera=4, precision=precision).eval()   # swin_t(**kwargs), swin_transformer.py:508-510
        sm.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in ssd.items()}, strict=True)
        e2 = sm(torch.from_numpy(img), view_index=torch.from_numpy(g["view"]))
        assert np.abs(e2.numpy() - g["swin_emb"]).max() / np.abs(g["swin_emb"]).max() < (2e-4 if precision != 1 else 2e-2)
        assert np.abs(sm(torch.from_numpy(img)).numpy() - e2.numpy()).max() > 1e-2        # and without the index: no embedding
        with pytest.raises(AttributeError):                # a model built without camera / sequence has no table
            models.build_model("swin_transformer", num_classes=751, loss="triplet", pretrained=False)(img, view_index=[0, 0, 0])
    finally:
        eng.set_side_index(None)
        eng.set_chunk(1024)
        eng.set_precision(0)


# ----------------------------------------------------------------------------- BASELINE configs[2] at its stated size
@pytest.mark.timeout(900)
@pytest.mark.parametrize("precision", [0, 1, 2])
def test_full_size_config2_swin_properties(eng, precision):
    """Swin-T v1 on 4096 images of 224 x 224 (BASELINE configs[2]) through size-independent properties - 256 distinct images, each
    16 times, shuffled.  Images are independent in eval mode (LayerNorm per token, window attention per image, MixedNorm's
    InstanceNorm per image), so (a) copies of an image get the same embedding wherever they sit in the batch - bit-identical in
    EVERY arithmetic mode.  (Round 3 saw one-f16-ulp flips on ~2e-6 of the fc1 + GELU outputs in modes 1 and 2: 63 of the 64
    unrolled GELU instances of the linear kernel's epilogue ended in v_fma_mixlo_f16 - one rounding to f16 - and one in
    v_fmac_f32 + v_cvt_f16_f32 - two roundings -, so the rows of that accumulator register disagreed with the rest;
    gemm_f16.hip:cvt_f16_rn now pins one form, test_linear_kernels_are_row_position_invariant checks the kernel alone) -, (b) the
    96-d distance matrix has a ~0 diagonal and the 16 nearest neighbours of every row are exactly its 16 copies, (c) six rows
    equal the oracle (torch-CPU restatement, pinned by swin_seed0.npz) within the mode's tolerance."""
    from oracle import swin
    sd = synth.swin_state_dict(0)
    eng.load_swin(*weights.pack_swin(sd)[:2])
    rng = np.random.default_rng(12)
    base = synth.images_f32(256, 2)
    ids = np.repeat(np.arange(256), 16)
    rng.shuffle(ids)
    x = base[ids]                                                        # 2.4 GB of host memory
    eng.set_precision(precision)
    try:
        eng.set_chunk(256)
        emb = eng.swin_embed_f32_nchw(x)
        del x
        first = np.asarray([np.flatnonzero(ids == c)[0] for c in range(256)])
        assert emb.shape == (4096, 96) and np.isfinite(emb).all()
        bad = np.flatnonzero((emb != emb[first][ids]).any(1))
        print("config2 precision %d: rows that differ from their first copy: %d (passes %s), max rel %.2e"
              % (precision, len(bad), sorted(set((bad // 256).tolist()))[:16], float(np.abs(emb - emb[first][ids]).max() / np.abs(emb).max())))
        assert np.array_equal(emb, emb[first][ids])                     # (a) position invariance, bit-exact in every mode
        dist = eng.distmat(emb, emb, _ffi.METRIC_L2)
        scale = float(np.median(dist))
        same = ids[:, None] == ids[None, :]
        # |x|^2 + |y|^2 - 2x.y cancels ~1e-7 * |x|^2 in fp32 (the reference's addmm_ does too); the sqrt makes that ~1e-2 of a distance
        assert dist[same].max() <= 3e-2 * scale
        assert dist[~same].min() > 5 * dist[same].max()
        _, knn = eng.knn(emb, emb, 16)
        assert np.array_equal(np.sort(ids[knn], axis=1), np.repeat(ids[:, None], 16, 1))   # (b)
        sample = first[:6]
        want = swin.embed(sd, base[ids[sample]])                         # (c)
        cos = (emb[sample] * want).sum(1) / np.linalg.norm(emb[sample], axis=1) / np.linalg.norm(want, axis=1)
        assert (1 - cos).max() < (1e-4 if precision == 1 else 1e-5)
        assert np.abs(emb[sample] - want).max() / np.abs(want).max() < (1e-2 if precision == 1 else 2e-4)
    finally:
        eng.set_chunk(128)
        eng.set_precision(0)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("precision", [0, 2])
def test_swin_at_the_bench_pass_size(eng, precision):
    """bench.py times Swin in ONE pass of 1024 images per reid_swin_embed_* pass (run_swin: set_chunk(min(chunk, 1024)); 13 GB of
    activations, csrc/swin.hip reid_swin_embed_f32_nchw_dev) - the size nothing else exercises.  1024 images = 64 distinct x 16,
    shuffled, in exact fp32 and in the bench's fp32-class arithmetic: (a) copies bit-identical, (b) bit-equal to the same batch
    in four passes of 256 (images are independent: swin_transformer.py:191-232 attends inside a window of ONE image, LayerNorm
    is per token, :248-260), (c) six rows against oracle/swin.py at the thresholds of the 256-pass full-size test."""
    from oracle import swin
    sd = synth.swin_state_dict(0)
    eng.load_swin(*weights.pack_swin(sd)[:2])
    rng = np.random.default_rng(21)
    base = synth.images_f32(64, 7)
    ids = np.repeat(np.arange(64), 16)
    rng.shuffle(ids)
    x = base[ids]                                                        # 617 MB of host memory
    eng.set_precision(precision)
    try:
        eng.set_chunk(1024)
        emb = eng.swin_embed_f32_nchw(x)
        eng.set_chunk(256)
        emb256 = eng.swin_embed_f32_nchw(x)
        first = np.asarray([np.flatnonzero(ids == c)[0] for c in range(64)])
        assert emb.shape == (1024, 96) and np.isfinite(emb).all()
        assert np.array_equal(emb, emb[first][ids])                     # (a)
        assert np.array_equal(emb, emb256)                              # (b)
        sample = first[:6]
        want = swin.embed(sd, base[ids[sample]])                        # (c)
        cos = (emb[sample] * want).sum(1) / np.linalg.norm(emb[sample], axis=1) / np.linalg.norm(want, axis=1)
        assert (1 - cos).max() < 1e-5
        assert np.abs(emb[sample] - want).max() / np.abs(want).max() < 2e-4
    finally:
        eng.set_chunk(128)
        eng.set_precision(0)


# ----------------------------------------------------------------------------- BASELINE configs[3] stand-in at its stated size
@pytest.mark.timeout(900)
@pytest.mark.parametrize("precision", [0, 1, 2])
def test_full_size_config3_tracking_stream(eng_w0, precision):
    """The 600-frame stream of SURVEY.md 8(d) config 4 (detections ~ Poisson(30) in [1, 80], ragged crops; synth.tracking_stream -
    the generator bench.py times) through the frame pipeline as the bench drives it (tracking.ShardedCameraStream, one rank):
    submit f+1 under the costs of f, 40 tracks x 100-sample ring that wraps during the stream.  Every 50th frame is checked
    against the oracle: features vs oracle preprocess + forward (cosine), the gated appearance cost vs oracle/nn_matching.py over a
    host bank that was fed the same features frame by frame, the DIoU cost bit-exact."""
    import types
    from oracle import nn_matching as onn
    from reid_amd.tracking import ShardedCameraStream
    eng, sd = eng_w0
    counts, pool, boxes, crops_of = synth.tracking_stream(600, 3)
    tracks = list(range(40))
    rng = np.random.default_rng(30)
    seed_feats = rng.normal(size=(40 * 100, 512)).astype(np.float32)
    eng.set_precision(precision)
    stream = ShardedCameraStream(eng, types.SimpleNamespace(rank=0, world=1), 0.15, 100)
    host = onn.NearestNeighborDistanceMetric("cosine", 0.15, budget=100)
    try:
        stream.metric.partial_fit(seed_feats, np.repeat(tracks, 100), tracks)
        host.partial_fit(list(seed_feats), np.repeat(tracks, 100), tracks)
        stream.submit(crops_of(0))
        checked = 0
        for f in range(600):
            n = int(counts[f])
            feats, cost, icost = stream.step(n, tracks, boxes[:40], boxes[:n], crops_of(f + 1) if f + 1 < 600 else None)
            assert feats.shape == (n, 512) and cost.shape == (40, n) and icost.shape == (40, n)
            if f % 50 == 0 or f == 599:
                want = seres18.forward(sd, torch.from_numpy(matching.preprocess(crops_of(f))))[0].numpy()
                cos = (feats * want).sum(1) / np.linalg.norm(feats, axis=1) / np.linalg.norm(want, axis=1)
                assert (1 - cos).max() < (1e-4 if precision == 1 else 1e-5), (f, (1 - cos).max())   # mode 2 (bench.py's tracking dtype) at mode 0's bar
                np.testing.assert_allclose(cost, onn.gate(host.distance(feats, tracks), 0.15), rtol=0, atol=2e-6, err_msg="frame %d" % f)
                assert np.array_equal(icost, matching.diou_cost(boxes[:40], boxes[:n])), f
                assert (cost <= 0.15 + 1e-5 + 1e-7).all()
                checked += 1
            k = min(n, 40)
            stream.commit(np.arange(k), tracks[:k], tracks)
            host.partial_fit(list(feats[:k]), tracks[:k], tracks)
        assert checked == 13
        assert stream.metric.samples_count(0) == 100                     # the ring has wrapped (600 samples into 100 slots)
    finally:
        stream.close()
        stream.metric.close()
        eng.set_precision(0)


# ----------------------------------------------------------------------------- fused distance + selection (dist_select.hip)
def _knn_oracle(xq, xb, k):
    """Brute force in float64 with the engine's tie rule (ascending distance, then lowest index)."""
    d = (xq.astype(np.float64) ** 2).sum(1)[:, None] + (xb.astype(np.float64) ** 2).sum(1)[None, :] - 2.0 * xq.astype(np.float64) @ xb.astype(np.float64).T
    idx = np.argsort(d, axis=1, kind="stable")[:, :k]
    return np.take_along_axis(d, idx, 1), idx


@pytest.mark.parametrize("m,n,d,k", [(1, 1, 32, 1), (3, 129, 33, 5), (130, 257, 96, 20), (257, 2100, 512, 64), (64, 5000, 1263, 20),
                                     (300, 3000, 40, 1), (129, 2049, 33, 7), (200, 2500, 512, 65)])
def test_fused_select_matches_two_pass_and_oracle(eng, m, n, d, k):
    """reid_knn / reid_argmin_rows through the fused kernel (no m x n matrix; galleries under 2048 rows and k = 65 take the
    two-pass path) against the
    distance matrix of the same library (the fused distances must be the matrix kernel's, bit for bit) and a float64 oracle:
    ragged tiles, K padded to whole K-tiles (d = 33, 40, 1263), k up to the list's compaction size, k > gallery."""
    rng = np.random.default_rng(m * 7 + n)
    xq = rng.normal(size=(m, d)).astype(np.float32)
    xb = rng.normal(size=(n, d)).astype(np.float32)
    if n > 40:
        xb[n // 2] = xb[3]                                  # a duplicate gallery row: the tie goes to the lower index
        xq[0] = xb[3]
    kk = min(k, n)
    D, I = eng.knn(xq, xb, k)
    full = eng.distmat(xq, xb, _ffi.METRIC_L2SQR)
    order = np.lexsort((np.broadcast_to(np.arange(n), full.shape), full), axis=1)[:, :kk]
    assert np.array_equal(I[:, :kk], order)                 # exactly the selection a full sort of the library's own matrix gives
    assert np.array_equal(D[:, :kk], np.take_along_axis(full, order, 1))
    if k > n:
        assert (I[:, n:] == -1).all() and np.isinf(D[:, n:]).all()
    Dr, Ir = _knn_oracle(xq, xb, kk)
    # |x|^2 + |y|^2 - 2x.y cancels ~1e-7 of the norms (the duplicate row's distance 0 comes out as ~1e-4 |x|^2 at d = 1263)
    scale = float((xq.astype(np.float64) ** 2).sum(1).max() + (xb.astype(np.float64) ** 2).sum(1).max())
    assert (np.abs(D[:, :kk] - Dr) <= 2e-6 * scale).all()
    if n > 40 and kk >= 2:
        assert I[0, 0] == 3 and I[0, 1] == n // 2
    for metric in (_ffi.METRIC_L2, _ffi.METRIC_COS, _ffi.METRIC_COS_HALF, _ffi.METRIC_DOT):
        idx, val = eng.argmin_rows(xq, xb, metric)
        fm = eng.distmat(xq, xb, metric)
        assert np.array_equal(idx, fm.argmin(1)) and np.array_equal(val, fm.min(1)), metric


@pytest.mark.parametrize("order", ["random", "ascending", "descending"])
def test_fused_select_long_sweeps_and_adversarial_order(eng, order):
    """20 000 gallery rows (the sample bound, many column tiles per block, list compactions): the gallery sorted by distance to
    every query in DESCENDING order makes every element a candidate (each one beats the running threshold), ascending order
    none after the first tile - the result must be the full sort's either way."""
    rng = np.random.default_rng(17)
    n, d, k = 20000, 64, 20
    base = rng.normal(size=d).astype(np.float32)
    dirs = rng.normal(size=(n, d)).astype(np.float32)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    radius = np.sort(rng.uniform(0.5, 30.0, n)).astype(np.float32)
    if order == "descending":
        radius = radius[::-1].copy()
    elif order == "random":
        rng.shuffle(radius)
    xb = base + dirs * radius[:, None]
    xq = (base + 0.01 * rng.normal(size=(150, d))).astype(np.float32)    # every query sits at the centre: distance ~ radius
    D, I = eng.knn(xq, xb, k)
    full = eng.distmat(xq, xb, _ffi.METRIC_L2SQR)
    want = np.lexsort((np.broadcast_to(np.arange(n), full.shape), full), axis=1)[:, :k]
    assert np.array_equal(I, want)
    assert np.array_equal(D, np.take_along_axis(full, want, 1))
    idx, val = eng.argmin_rows(xq, xb, _ffi.METRIC_L2)
    fl2 = eng.distmat(xq, xb, _ffi.METRIC_L2)
    assert np.array_equal(idx, fl2.argmin(1)) and np.array_equal(val, fl2.min(1))


# ----------------------------------------------------------------------------- precision 2 at tracking sizes
@pytest.mark.parametrize("n", [1, 3, 7, 30, 33])
def test_fp32_class_mode_small_and_odd_batches(eng_w0, n):
    """precision 2 on batches that leave tiles ragged and take the split-K form of the halo kernel (a tracking frame): against
    the exact-fp32 mode at the fp32 thresholds, and the same crops inside a larger batch."""
    eng, sd = eng_w0
    crops = synth.smooth_crops_u8(n, 60 + n)
    ref = eng.embed_u8(crops)
    eng.set_precision(2)
    try:
        got = eng.embed_u8(crops)
        again = eng.embed_u8(np.concatenate([crops, crops[::-1]]))
        ragged = eng.embed_ragged_u8([c[: 200 + 5 * i, : 100 + 3 * i] for i, c in enumerate(crops)])
    finally:
        eng.set_precision(0)
    ragged_ref = eng.embed_ragged_u8([c[: 200 + 5 * i, : 100 + 3 * i] for i, c in enumerate(crops)])
    cos = (got * ref).sum(1) / np.linalg.norm(got, axis=1) / np.linalg.norm(ref, axis=1)
    assert (1 - cos).max() < 1e-5
    scale = np.abs(ref).max()
    assert np.abs(got - ref).max() <= 2e-5 * scale
    assert np.abs(again[:n] - got).max() <= 2e-5 * scale and np.abs(again[n:][::-1] - got).max() <= 2e-5 * scale
    assert np.abs(ragged - ragged_ref).max() <= 2e-5 * np.abs(ragged_ref).max()


# ----------------------------------------------------------------------------- object lifetime
@pytest.mark.parametrize("first", ["engine", "bank", "cycle"])
def test_engine_and_bank_can_be_collected_in_any_order(first):
    """An engine and the feature banks created on it reference each other; whichever goes first - an explicit close of either, or
    the cycle collector finalising them in its own order at interpreter exit (bench.py's camera streams) - the device bank is
    destroyed exactly once (a second reid_bank_destroy is a use-after-free)."""
    import gc
    from reid_amd.engine import Engine
    from reid_amd.nn_matching import NearestNeighborDistanceMetric
    e = Engine(0)
    m = NearestNeighborDistanceMetric("cosine", 0.2, 10, max_tracks=8, engine=e)
    m.partial_fit(np.random.default_rng(0).normal(size=(3, 512)).astype(np.float32), np.asarray([1, 2, 3]), [1, 2, 3])
    assert m._bank is not None
    if first == "engine":
        e.close()
        m.close()
    elif first == "bank":
        m.close()
        e.close()
    else:
        m.__del__()           # what the collector may do first ...
        e.__del__()           # ... and then: the engine must not destroy the bank again
        m.__del__()
    del m, e
    gc.collect()


# ----------------------------------------------------------------------------- large k-NN on the f16 matrix pipe (knn_wide.hip)
@pytest.mark.parametrize("n,d,k,scale", [(8200, 512, 5, 1.0), (8300, 200, 20, 1.0), (9000, 136, 24, 300.0), (8200, 256, 1, 1e-4)])
def test_wide_knn_equals_the_fused_fp32_search_bit_for_bit(eng_w0, n, d, k, scale):
    """reid_knn on a LARGE problem (reid/faiss_utils.py:149-176: the re-ranking's search) takes its candidates from an fp32-class
    GEMM on the f16 matrix pipe and recomputes them in exact fp32 (knn_wide.hip): indices AND distances must equal the fused
    fp32 search (dist_select.hip - itself bit-equal to a full sort of the library's distance matrix,
    test_fused_select_matches_two_pass_and_oracle) bit for bit - on clustered features with duplicate rows (exact ties go to
    the lower index), with features far outside / inside f16's range (the candidate stage normalises by powers of two), and
    with every 13th row forced through the exact-row fallback that a failed sufficiency proof takes."""
    import ctypes as C
    eng, _ = eng_w0
    sw = _ffi.debug_lib().reid_debug_knn_wide
    sw.restype = C.c_int
    sw.argtypes = [C.c_void_p, C.c_int, C.c_int]
    _, _, _, x, _, _ = synth.clustered_embeddings(1, n, d=d, n_ids=97, n_cams=6, seed=n + k, sigma=0.9)
    x = (x * scale).astype(np.float32)
    x[n // 2] = x[7]
    x[n - 1] = x[7]
    q = np.ascontiguousarray(x[: n - 100])              # queries: a (ragged) subset, so that M is not a multiple of the tile
    try:
        _ffi.check(sw(eng.h, 0, 0))
        D0, I0 = eng.knn(q, x, k)
        _ffi.check(sw(eng.h, 1, 0))
        D1, I1 = eng.knn(q, x, k)
        _ffi.check(sw(eng.h, 1, 13))
        D2, I2 = eng.knn(q, x, k)
    finally:
        _ffi.check(sw(eng.h, 1, 0))
    assert np.array_equal(I0, I1) and np.array_equal(D0, D1)
    assert np.array_equal(I0, I2) and np.array_equal(D0, D2)
    assert I0[7, 0] == 7 and (k < 3 or (I0[7, 1] == n // 2 and I0[7, 2] == n - 1))     # the duplicates, lowest index first


# ----------------------------------------------------------------------------- row-position invariance of the linear kernels
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("n,k", [(384, 96), (96, 384), (288, 96), (768, 192), (3072, 768), (768, 3072)])
def test_linear_kernels_are_row_position_invariant(eng_w0, mode, n, k):
    """The f16 linear build (gemm_f16.hip, LIN: every Linear of the Swin trunk in modes 1 and 2) on rows that repeat: eight distinct
    input rows spread over 4224 rows (16.5 tiles of 256, so the ragged last tile's general path runs too) must give bit-identical
    output rows wherever a row sits in its tile - for the LDS-staged f16 / [yh | yl'] epilogue with and without GELU and for the
    fp32 stream epilogue with residual.  This is the kernel-level form of the position invariance that
    test_full_size_config2_swin_properties asserts on embeddings (swin_transformer.py:191-232,248-260: tokens of different images
    never meet in a Linear)."""
    import ctypes as C
    eng, _ = eng_w0
    fn = _ffi.debug_lib().reid_debug_linear_rows
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p] * 5 + [C.c_int] * 5 + [C.c_void_p]
    rng = np.random.default_rng(n + k + mode)
    m, R = 4096 + 128, 8
    base = rng.normal(size=(R, k)).astype(np.float32)
    ids = np.asarray([(i * 5 + i // 7) % R for i in range(m)])
    x = np.ascontiguousarray(base[ids])
    w = (rng.normal(size=(n, k)) / np.sqrt(k)).astype(np.float32)
    bias = rng.normal(size=n).astype(np.float32)
    resb = rng.normal(size=(R, n)).astype(np.float32)
    res = np.ascontiguousarray(resb[ids])
    first = np.asarray([np.flatnonzero(ids == r)[0] for r in range(R)])
    want = (base.astype(np.float64) @ w.astype(np.float64).T + bias)
    for flags, with_res in ((3, False), (2, False), (0, True), (1, False)):
        out = np.empty((m, n), np.float32)
        _ffi.check(fn(eng.h, x.ctypes.data, w.ctypes.data, bias.ctypes.data, res.ctypes.data if with_res else None, m, n, k, mode,
                      flags, out.ctypes.data))
        assert np.array_equal(out, out[first][ids]), (mode, flags)
        if not flags & 1:    # and the values are the layer's (loose: f16 operands in mode 1)
            ref = want + (resb if with_res else 0.0)
            assert np.abs(out[first] - ref).max() < (3e-2 if mode == 1 else 2e-5) * max(1.0, np.abs(ref).max())


# ----------------------------------------------------------------------------- precision 2: operand-range guards
def test_mode2_refuses_weights_it_cannot_split(eng):
    """reid_model_factory.load_pretrained_weights accepts any shape-compatible checkpoint (modification_tracking/
    reid_model_factory.py:158-210); the fp32-class arithmetic splits weights as [wh 2^11 | wh | wl'] f16 and needs |w| 2^11 < 65504.
    A checkpoint outside that range is refused for mode 2 with the tensor's name, both ways round (select the mode, then load /
    load, then select the mode), and keeps working in mode 0."""
    from reid_amd._ffi import ReidHipError
    sd = synth.seres18_state_dict(0)
    sd["basicBlock31.block_pre.conv2.weight"] = np.array(sd["basicBlock31.block_pre.conv2.weight"], copy=True)
    sd["basicBlock31.block_pre.conv2.weight"][3, 5, 1, 1] = 40.0
    blob, manifest, _ = weights.pack_seres18(sd)
    crops = synth.smooth_crops_u8(2, seed=3)
    try:
        eng.set_precision(0)
        eng.load_seres18(blob, manifest)                       # fine in mode 0 ...
        assert np.isfinite(eng.embed_u8(crops)).all()
        with pytest.raises(ReidHipError, match=r"b31\.conv2\.w.*use mode 0"):
            eng.set_precision(2)                               # ... but mode 2 is refused, naming the tensor
        eng.set_precision(1)
        eng.set_precision(0)
        good = weights.pack_seres18(synth.seres18_state_dict(0))
        eng.load_seres18(*good[:2])
        eng.set_precision(2)                                   # a checkpoint inside the range: accepted
        with pytest.raises(ReidHipError, match=r"b31\.conv2\.w"):
            eng.load_seres18(blob, manifest)                   # loading the bad one into a mode-2 context: refused
        # Swin: the same for a Linear weight
        ssd = synth.swin_state_dict(0)
        key = "stage2.layers.0.0.mlp_block.fn.fn.net.0.weight"
        ssd[key] = np.array(ssd[key], copy=True)
        ssd[key][7, 9] = -33.0
        with pytest.raises(ReidHipError, match=r"fc1\.w"):
            eng.load_swin(*weights.pack_swin(ssd)[:2])
        eng.set_precision(0)
        eng.load_swin(*weights.pack_swin(ssd)[:2])
        with pytest.raises(ReidHipError, match=r"fc1\.w"):
            eng.set_precision(2)
    finally:
        eng.set_precision(0)
        eng.load_swin(*weights.pack_swin(synth.swin_state_dict(0))[:2])
        eng.load_seres18(*weights.pack_seres18(synth.seres18_state_dict(0))[:2])


def test_mode2_activation_overflow_and_nonfinite_embedding_are_reported(eng):
    """An activation f16 cannot hold (here: a stem BatchNorm scaled by 1e7) reaching a split-operand site raises the context's
    sticky fault word: the embed call that produced it fails with REID_ERR_STATE instead of returning laundered values
    (max(NaN, 0) = 0 in every ReLU), so does every later call until reid_ctx_clear_fault; mode 0 runs the same checkpoint.  A
    non-finite embedding (an infinite BNNeck scale) is reported in every mode."""
    from reid_amd._ffi import ReidHipError
    crops = synth.smooth_crops_u8(3, seed=4)
    good = weights.pack_seres18(synth.seres18_state_dict(0))[:2]
    sd = synth.seres18_state_dict(0)
    sd["bn0.weight"] = np.asarray(sd["bn0.weight"]) * 1e7
    hot = weights.pack_seres18(sd)[:2]
    try:
        eng.set_precision(0)
        eng.load_seres18(*hot)
        assert np.isfinite(eng.embed_u8(crops)).all()          # InstanceNorm rescales: exact fp32 handles it
        eng.set_precision(2)
        with pytest.raises(ReidHipError, match="outside f16's range"):
            eng.embed_u8(crops)
        with pytest.raises(ReidHipError, match="outside f16's range"):
            eng.embed_u8(crops)                                # sticky
        with pytest.raises(ReidHipError):
            eng.sync()
        eng.clear_fault()
        eng.load_seres18(*good)
        want = eng.embed_u8(crops)
        assert np.isfinite(want).all()
        # fp32 crops take the other stem loader and the general pack pass
        with pytest.raises(ReidHipError, match="outside f16's range"):
            eng.load_seres18(*hot)
            eng.embed_f32_nchw(np.random.default_rng(0).normal(size=(2, 3, 256, 128)).astype(np.float32))
        eng.clear_fault()
        # a non-finite embedding, any mode
        sd2 = synth.seres18_state_dict(0)
        sd2["bnneck.weight"] = np.array(sd2["bnneck.weight"], copy=True)
        sd2["bnneck.weight"][5] = np.inf
        eng.load_seres18(*weights.pack_seres18(sd2)[:2])
        for mode in (0, 1, 2):
            eng.set_precision(mode)
            with pytest.raises(ReidHipError, match="non-finite embedding"):
                eng.embed_u8(crops)
            eng.clear_fault()
    finally:
        eng.clear_fault()
        eng.set_precision(0)
        eng.load_seres18(*good)


# ----------------------------------------------------------------------------- bench contract
@pytest.mark.timeout(600)
def test_bench_prints_one_json_line_and_exits_cleanly():
    """`python bench.py` (here: a small embed workload over a REAL 1-rank RCCL communicator, REID_BENCH_COMM1=1) writes exactly one
    line to stdout - the JSON of the contract, with `roofline` (--full) - and exits 0: RCCL's version banner and any other native print go
    to stderr, and the interpreter's shutdown (engine / bank finalisers) does not crash."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, REID_BENCH_COMM1="1")
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--full", "--workload", "embed", "--crops", "256", "--steps",
                        "1", "--warmup", "1", "--no-cpu", "--single"], capture_output=True, text=True, env=env, timeout=500)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[:2000]
    d = json.loads(lines[0])
    assert d["unit"] == "crops/s" and d["n_gpus"] == 1 and d["value"] > 0 and d["dtype"] == "f16x3"
    assert d["roofline"]["bound"] in ("hbm", "mfma") and 0 < d["roofline"]["frac"] < 1


@pytest.mark.gpu
@pytest.mark.parametrize("m,c,hid,act,ln", [(2048, 96, 384, 1, 1), (1024 + 49, 96, 96, 0, 0), (4096 + 160, 96, 384, 1, 0), (2048 + 16 * 49, 192, 768, 1, 1),
                                             (1024 + 784, 192, 192, 0, 0)])
def test_fused_pair_of_linears_matches_float64_and_is_position_invariant(eng_w0, m, c, hid, act, ln):
    """csrc/two_linear_f16.hip (precision 2, Swin stages 1-2: to_out -> post_proj + x, LayerNorm -> fc1 -> GELU -> fc2 + x;
    swin_transformer.py:23-39,66-82,191-232) through reid_debug_two_linear: out = res + w2 . act(w1 . [LN](x) + b1) + b2 against float64
    at the fp32-class bound, ragged token counts, and copies of one row at different tile positions bit-identical (images are
    independent in eval mode)."""
    import ctypes as C
    import math
    eng, _ = eng_w0
    fn = _ffi.debug_lib().reid_debug_two_linear
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p] * 7 + [C.c_int] * 5 + [C.c_void_p] * 4
    rng = np.random.default_rng(m + hid)
    R = 61
    base = rng.normal(size=(R, c)).astype(np.float32)
    if ln:
        base = (base * rng.uniform(0.5, 3.0, size=(R, 1)) + rng.normal(size=(R, 1))).astype(np.float32)
    rb = rng.normal(size=(R, c)).astype(np.float32)
    ids = np.asarray([(i * 5 + i // 7) % R for i in range(m)])
    x, res = np.ascontiguousarray(base[ids]), np.ascontiguousarray(rb[ids])
    w1 = (rng.normal(size=(hid, c)) / np.sqrt(c)).astype(np.float32)
    b1 = rng.normal(size=hid).astype(np.float32)
    w2 = (rng.normal(size=(c, hid)) / np.sqrt(hid)).astype(np.float32)
    b2 = rng.normal(size=c).astype(np.float32)
    g = (1.0 + 0.1 * rng.normal(size=c)).astype(np.float32)
    bt = (0.1 * rng.normal(size=c)).astype(np.float32)
    out = np.empty((m, c), np.float32)
    eng.set_precision(2)
    try:
        _ffi.check(fn(eng.h, x.ctypes.data, w1.ctypes.data, b1.ctypes.data, w2.ctypes.data, b2.ctypes.data, res.ctypes.data, m, c, hid, act, 1,
                      out.ctypes.data, None, g.ctypes.data if ln else None, bt.ctypes.data if ln else None))
    finally:
        eng.set_precision(0)
    b64 = base.astype(np.float64)
    if ln:
        b64 = (b64 - b64.mean(1, keepdims=True)) / np.sqrt(b64.var(1, keepdims=True) + 1e-5) * g + bt
    h = b64 @ w1.T.astype(np.float64) + b1
    if act:
        h = 0.5 * h * (1.0 + np.vectorize(math.erf)(h / math.sqrt(2.0)))
    ref = (h @ w2.T.astype(np.float64) + b2 + rb)[ids]
    assert np.abs(out - ref).max() <= 1.5e-6 * np.abs(ref).max()          # fp32-class: three f16 products, fp32 sums (measured 3e-7)
    first = [int(np.flatnonzero(ids == r)[0]) for r in range(R)]
    assert np.array_equal(out, out[first][ids])


@pytest.mark.gpu
def test_swin_embeddings_do_not_depend_on_the_pass_size(eng):
    """reid_swin_embed_* walks a batch in passes of up to 1024 images (swin.hip); REID_SWIN_CHUNK_MAX - one of the two environment
    variables the product library reads, both sizing knobs - lowers the cap.  Images are independent in eval mode
    (swin_transformer.py:248-260), so 12 images embedded in passes of 2, 5 and 12 must agree bit for bit, in the exact and in the
    fp32-class mode (whose stage 1-2 launches are the fused kernels of two_linear_f16.hip in every one of these passes, and plain
    gemm_f16 launches with the debug switch swin_two_linear = 0 - which must agree with them at the mode's error level)."""
    import subprocess, sys, json as _json
    code = ("import sys, json, numpy as np; sys.path.insert(0, %r); from reid_amd import synth, weights; from reid_amd.engine import get_engine;"
            "eng = get_engine(0); eng.load_swin(*weights.pack_swin(synth.swin_state_dict(0))[:2]); eng.set_chunk(4096); x = synth.images_f32(12, 4);"
            "a = eng.swin_embed_f32_nchw(x); eng.set_precision(2); b = eng.swin_embed_f32_nchw(x); print(json.dumps([a.tolist(), b.tolist()]))"
            % os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

    def run(**env):
        out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, check=True).stdout
        return [np.asarray(v, np.float32) for v in _json.loads(out.strip().splitlines()[-1])]

    ref = run(REID_SWIN_CHUNK_MAX="12")
    for cap in ("2", "5"):
        got = run(REID_SWIN_CHUNK_MAX=cap)
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), cap
    # the same through reid_ctx_set_chunk in this process, and with the fused stage 1-2 launches switched off
    eng.load_swin(*weights.pack_swin(synth.swin_state_dict(0))[:2])
    x = synth.images_f32(12, 4)
    try:
        eng.set_chunk(5)
        assert np.array_equal(eng.swin_embed_f32_nchw(x), ref[0])
        eng.set_precision(2)
        assert np.array_equal(eng.swin_embed_f32_nchw(x), ref[1])
        eng.debug_switch("swin_two_linear", 0)
        unfused = eng.swin_embed_f32_nchw(x)
        assert not np.array_equal(unfused, ref[1])                             # the switch did select the other launches
        assert np.abs(unfused - ref[1]).max() <= 2e-6 * np.abs(ref[1]).max()   # same roundings, another summation order
    finally:
        eng.debug_switch("swin_two_linear", 1)
        eng.set_precision(0)
        eng.set_chunk(1024)
    assert np.abs(ref[1] - ref[0]).max() <= 2e-6 * np.abs(ref[0]).max()       # fp32-class against exact fp32


@pytest.mark.gpu
def test_swin_dense_x3_kernel_agrees_with_the_gemm_f16_linear_build(eng):
    """conv3x3_x3.hip, lin_x3_kernel (round 5): the stage 3-4 linears of the fp32-class mode (N % 128 == 0) as 4-wave blocks, two per CU,
    on v_mfma_f32_16x16x32_f16 - the xh fragments shared by two of the three products - for EVERY batch size (ragged last tiles: 1, 3 and 7
    images are 196-, 588- and 1372-row matrices in stage 3, 49 / 147 / 343 rows in stage 4).  Same three products per multiply, another
    summation order than gemm_f16.hip's linear build (debug switch lin_x3 = 0): agreement at the mode's error level, both inside the
    mode's bound against exact fp32; an image's embedding does not depend on its batch (swin_transformer.py:191-232, 248-260)."""
    eng.load_swin(*weights.pack_swin(synth.swin_state_dict(0))[:2])
    x = synth.images_f32(7, 9)
    try:
        eng.set_precision(0)
        exact = eng.swin_embed_f32_nchw(x)
        eng.set_precision(2)
        eng.debug_switch("lin_x3", 0)
        old = eng.swin_embed_f32_nchw(x)
        eng.debug_switch("lin_x3", 1)
        new = eng.swin_embed_f32_nchw(x)
        assert not np.array_equal(new, old)                                      # the switch did select the other kernel
        scale = np.abs(exact).max()
        assert np.abs(new - old).max() <= 2e-6 * scale
        assert np.abs(new - exact).max() <= 2e-6 * scale and np.abs(old - exact).max() <= 2e-6 * scale
        assert np.array_equal(eng.swin_embed_f32_nchw(x[:1]), new[:1]) and np.array_equal(eng.swin_embed_f32_nchw(x[2:5]), new[2:5])
    finally:
        eng.debug_switch("lin_x3", 1)
        eng.set_precision(0)


@pytest.mark.parametrize("n", [1, 7, 30, 64, 130, 256])
def test_strided_and_1x1_convolutions_on_the_x3s_kernel(eng_w0, n):
    """conv3x3_x3.hip, conv_x3s_kernel (round 6): the strided 3x3 and the 1x1 convolutions of the fp32-class mode (SERes18_IBN.py:120-128
    conv1 of a down-sampling block, :250-276 the shortcut convolutions) as lin_x3_kernel's block over an im2col GATHER - per-lane pixel
    of tap (0, 0), scalar tap / chunk offsets, taps outside the image as offsets past the descriptor - with split-K over the (tap, chunk)
    steps (uneven shares) and the convolution epilogue of x3m16_tail.  Default (switch conv_x3s = 1): wherever gemm_f16.hip's SPLIT
    build served; 2: also the small launches that otherwise run in exact fp32; 0: off.  The three forms against each other and against
    exact fp32 at the mode's error level (odd image counts: ragged last tile rows; 130: unsplit, 64: the size where the forms meet),
    copies of a crop bit-identical inside a pass in every form, no fault bit."""
    eng, _ = eng_w0
    base = synth.smooth_crops_u8(max(2, (n + 1) // 2), 40 + n)
    ids = np.arange(n) % len(base)
    np.random.default_rng(n).shuffle(ids)
    crops = base[ids]
    try:
        eng.set_precision(0)
        exact = eng.embed_u8(crops)
        eng.set_precision(2)
        out = {}
        for sw in (0, 1, 2):
            eng.debug_switch("conv_x3s", sw)
            out[sw] = eng.embed_u8(crops)
            first = {int(c): int(np.flatnonzero(ids == c)[0]) for c in np.unique(ids)}
            assert all(np.array_equal(out[sw][i], out[sw][first[int(ids[i])]]) for i in range(n)), sw
        scale = np.abs(exact).max()
        for sw in (0, 1, 2):
            assert np.abs(out[sw] - exact).max() <= 5e-6 * scale, sw
        assert np.abs(out[1] - out[0]).max() <= 5e-6 * scale and np.abs(out[2] - out[0]).max() <= 5e-6 * scale
        assert not np.array_equal(out[2], out[0])                          # the switch did select the other kernel
        if n >= 130:
            assert not np.array_equal(out[1], out[0])                      # the default uses it where the launches are large
        assert eng.fault_bits() == 0
    finally:
        eng.debug_switch("conv_x3s", 1)
        eng.set_precision(0)


def test_fp32_class_mode_is_run_to_run_deterministic_across_launch_forms(eng_w0):
    """A race in a split-K rendezvous, a gather or an LDS-DMA wait shows as a run-to-run difference: every launch form of the
    fp32-class mode sums in a fixed order (reduce-scatter partials in split order, conv_x3s shares in step order), so repeats of the
    same pass must be bit-identical - at the pass sizes on both sides of the steps where the forms change (7: everything split; 33 / 48:
    layer 1 and the stem change form, layer 4 on 64-wide tiles; 66: two ways split; 130: unsplit, conv_x3s for the strided
    convolutions; 300: two passes' worth of tiles)."""
    eng, _ = eng_w0
    crops = synth.smooth_crops_u8(300, 33)
    eng.set_precision(2)
    try:
        for n in (7, 33, 48, 66, 130, 300):
            first = eng.embed_u8(crops[:n])
            for _ in range(3):
                assert np.array_equal(eng.embed_u8(crops[:n]), first), n
        assert eng.fault_bits() == 0
    finally:
        eng.set_precision(0)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_match_stream_random_operation_sequences_are_bit_identical_to_one_stream(eng_w0, seed):
    """reid_frame_match_stream under operation orders the streams' normal flow does not produce: the SAME random sequence of frame
    steps (with and without a next frame riding on them, frames without detections, tracks that die and come back), direct bank
    operations between frames (distance / partial_fit from host features, which join the two streams) and re-submissions of a slot
    runs on two CameraStreams - cost / update stages on the match stream, and everything on one stream.  Every result must be
    bit-identical: the second stream changes when things run, never what they compute."""
    from reid_amd.tracking import CameraStream
    eng, sd = eng_w0
    blob, manifest = weights.pack_seres18(sd)[:2]
    rng = np.random.default_rng(100 + seed)
    pool = synth.ragged_crops_u8(40, seed=30 + seed)
    boxes = rng.uniform(0, 300, (16, 4))
    boxes[:, 2:] = rng.uniform(10, 90, (16, 2))
    a = CameraStream(blob, manifest, 2, match_stream=True)
    b = CameraStream(blob, manifest, 2, match_stream=False)
    assert a.match_stream and not b.match_stream
    try:
        tracks = list(range(6))
        seeds = rng.normal(size=(12, 512)).astype(np.float32)
        for s_ in (a, b):
            s_.metric.partial_fit(seeds, np.repeat(tracks, 2), tracks)
        frame = lambda: [pool[int(i)] for i in rng.integers(0, 40, int(rng.integers(0, 12)))]
        known = list(tracks)                                         # tracks that have samples (the reference's `samples` keys)
        cur = frame()
        for s_ in (a, b):
            s_.submit(cur)
        for it in range(25):
            op = int(rng.integers(0, 10))
            if op == 0:                                              # direct bank operations between two frames
                q = rng.normal(size=(int(rng.integers(1, 6)), 512)).astype(np.float32)
                da, db = a.metric.distance(q, known), b.metric.distance(q, known)
                assert np.array_equal(da, db), it
                k = min(len(q), len(tracks))
                revived = sorted(set(known) | set(tracks[:k]))       # dead tracks come back with a sample from the host
                for s_ in (a, b):
                    s_.metric.partial_fit(q[:k], tracks[:k], revived)
                known = revived
                continue
            if op == 1:                                              # the pending frame is replaced before anyone asked for it
                cur = frame()
                for s_ in (a, b):
                    s_.submit(cur)
                continue
            nxt = frame() if op < 9 else None                        # (op 9: no next frame rides on this step)
            alive = [t for t in known if rng.random() > 0.15] or known[:1]
            ra = a.step(alive, boxes[:len(alive)], boxes[:len(cur)], nxt)
            rb = b.step(alive, boxes[:len(alive)], boxes[:len(cur)], nxt)
            for x, y in zip(ra, rb):
                assert (x is None and y is None) or np.array_equal(x, y), it
            k = min(len(cur), len(alive))
            rows = rng.permutation(len(cur))[:k]
            for s_ in (a, b):
                s_.commit(rows, alive[:k], alive)                    # tracks outside `alive` are forgotten here, and come back later
            known = list(alive)
            if nxt is None:
                nxt = frame()
                for s_ in (a, b):
                    s_.submit(nxt)
            cur = nxt
        for t in known:
            assert a.metric.samples_count(t) == b.metric.samples_count(t)
        assert a.eng.fault_bits() == 0 and b.eng.fault_bits() == 0
    finally:
        a.close(destroy=True)
        b.close(destroy=True)
