"""GPU parity of the Swin-T ``version="v2"`` blocks: the forward against the reference's own vectors (tests/golden/swin_v2.npz), against
the CPU restatement (tests/swin_v2_ref.py) for shapes the fixture does not hold, and the two v2 kernels alone (csrc/swin_v2.hip,
through the harnesses of libreid_hip_debug.so) against float64."""
import os
import sys

import numpy as np
import pytest
import torch

from reid_amd import _ffi, synth, weights

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import swin_v2_ref  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def eng():
    from reid_amd.engine import get_engine
    return get_engine(0)


@pytest.fixture(scope="module")
def g(golden_dir):
    return np.load(os.path.join(golden_dir, "swin_v2.npz"))


@pytest.fixture(scope="module")
def sd2():
    return synth.swin_state_dict(0, version="v2")


@pytest.fixture()
def eng_v2(eng, sd2):
    eng.set_precision(0)
    eng.load_swin(*weights.pack_swin(sd2)[:2])
    yield eng
    eng.set_precision(0)
    eng.set_chunk(1024)


def _cosdist(g):
    """The reference's symmetric 64 x 64 matrix from its stored upper triangle."""
    d = np.zeros((64, 64), np.float32)
    d[np.triu_indices(64)] = g["rank_cosdist_triu"]
    return d + np.triu(d, 1).T


def _cos_err(a, b):
    return float((1 - (a * b).sum(1) / np.linalg.norm(a, axis=1) / np.linalg.norm(b, axis=1)).max())


# ----------------------------------------------------------------------------- the forward against the reference's vectors
@pytest.mark.parametrize("precision", [0, 2, 1])
def test_v2_embed_matches_reference_fixture(eng_v2, g, sd2, precision):
    """v1's bars (test_swin_embed_matches_reference_fixture / test_swin_f16_storage_mode_within_north_star_tolerance): modes 0 and 2
    within 2e-4 of the fixture's range and 1 - cos < 1e-5; mode 1 within 1e-2 and 1 - cos < 1e-4.  Then N = 1 and a 448x224 image
    against the restatement, and N = 1 == row 0 of the batch bit for bit."""
    x = synth.images_f32(int(g["n"]), int(g["seed"]))
    x2 = synth.images_f32(1, 3, h=448, w=224)
    eng_v2.set_precision(precision)
    emb, logits = eng_v2.swin_embed_f32_nchw(x, logits=True)
    emb1 = eng_v2.swin_embed_f32_nchw(x[:1])
    e2 = eng_v2.swin_embed_f32_nchw(x2)
    eng_v2.set_precision(0)
    rel, cosbar = (1e-2, 1e-4) if precision == 1 else (2e-4, 1e-5)
    r1 = swin_v2_ref.forward(sd2, torch.from_numpy(x[:1]))[0].numpy()
    r2 = swin_v2_ref.forward(sd2, torch.from_numpy(x2))[0].numpy()
    figs = {"emb": np.abs(emb - g["emb"]).max() / np.abs(g["emb"]).max(), "logits": np.abs(logits - g["logits"]).max() / np.abs(g["logits"]).max(),
            "1-cos": _cos_err(emb, g["emb"]), "n1": np.abs(emb1 - r1).max() / np.abs(r1).max(), "448x224": np.abs(e2 - r2).max() / np.abs(r2).max()}
    print("swin v2 precision %d:" % precision, {k: "%.2e" % v for k, v in figs.items()})
    assert figs["emb"] < rel and figs["logits"] < rel and figs["1-cos"] < cosbar
    assert figs["n1"] < rel and figs["448x224"] < rel
    assert np.array_equal(emb1, emb[:1])


@pytest.mark.parametrize("precision,tol", [(0, 2e-5), (2, 2e-5), (1, 2e-2)])
def test_v2_stage_taps_match_reference_fixture(eng_v2, g, precision, tol):
    """The taps reid_debug_swin_stage hands out keep their meaning for v2: SFE output, the four stage outputs, GeM output, sampled as the
    fixture's generator sampled the reference's; v1's bars (test_swin_stage_taps_match_reference_fixture)."""
    n = int(g["n"])
    eng_v2.set_precision(precision)
    eng_v2.swin_embed_f32_nchw(synth.images_f32(n, int(g["seed"])))
    for stage, name in ((0, "sfe"), (1, "stage1"), (2, "stage2"), (3, "stage3"), (4, "stage4")):
        t = torch.from_numpy(eng_v2.debug_swin_stage(stage, n)).permute(0, 3, 1, 2)
        c, h, w = t.shape[1:]
        got = t[:, :: max(1, c // 8), :: max(1, h // 8), :: max(1, w // 4)].numpy()
        ref = g["tap_" + name]
        print("swin v2 precision %d tap %s: %.2e of range" % (precision, name, np.abs(got - ref).max() / np.abs(ref).max()))
        assert np.abs(got - ref).max() <= tol * np.abs(ref).max(), (name, np.abs(got - ref).max(), np.abs(ref).max())
        assert abs(float(t.double().mean()) - float(g["mean_" + name])) <= tol * float(g["absmean_" + name]), name
    gem = eng_v2.debug_swin_stage(5, n)[:, :: 96 // 8]
    ref = g["tap_avgpool"].reshape(gem.shape)
    assert np.abs(gem - ref).max() <= tol * np.abs(ref).max()


def test_v2_is_not_a_silent_v1_answer(eng, g, sd2):
    """Before v2 existed swin_t(version="v2") built a v1 model without a word.  The v2 embedding of the fixture's images is far from
    the v1 engine's embedding of the same images - by far more than any parity bar."""
    x = synth.images_f32(int(g["n"]), int(g["seed"]))
    eng.set_precision(0)
    eng.load_swin(*weights.pack_swin(synth.swin_state_dict(0))[:2])
    v1 = eng.swin_embed_f32_nchw(x)
    eng.load_swin(*weights.pack_swin(sd2)[:2])
    v2 = eng.swin_embed_f32_nchw(x)
    gap = 1 - (v1 * v2).sum(1) / np.linalg.norm(v1, axis=1) / np.linalg.norm(v2, axis=1)
    print("swin v2 vs v1 engine, 1 - cos per image:", gap)
    assert gap.min() > 1e-3
    assert _cos_err(v2, g["emb"]) < 1e-5


def test_v2_model_object_runs_the_v2_engine(eng, g):
    """The public surface: swin_t(version="v2") / build_model(..., version="v2") embed with the v2 blocks."""
    from reid_amd import models
    x = synth.images_f32(int(g["n"]), int(g["seed"]))
    m = models.build_model("swin_transformer", num_classes=751, loss="triplet", pretrained=False, precision="f32", version="v2")
    logits, emb = m(x, return_logits=True)
    assert _cos_err(emb, g["emb"]) < 1e-5 and np.abs(logits - g["logits"]).max() / np.abs(g["logits"]).max() < 2e-4
    m3 = models.build_model("swin_transformer", num_classes=751, loss="triplet", pretrained=False, version="v2")   # the default mode: f16x3
    assert m3.precision == "f16x3" and _cos_err(m3(x), g["emb"]) < 1e-5


def test_v2_side_information_branch(eng):
    """swin_t(camera=4, version="v2")(img, view_index=...): the stem, and with it the side-information term, is v1's
    (swin_transformer.py:298-302).  Against the restatement, in the exact and the fp32-class mode; the indices matter."""
    from reid_amd.backbone import swin_t
    x = synth.images_f32(3, 4)
    view = np.asarray([2, 0, 3])
    try:
        for prec in ("f32", "f16x3"):
            m = swin_t(camera=4, version="v2", seed=4, precision=prec)
            sd = synth.swin_state_dict(4, views=4, version="v2")
            assert list(m.state_dict()) == list(sd) and list(sd)[0] == "sfe.side_info_embedding"
            got = m(x, view_index=view)
            ref = swin_v2_ref.forward(sd, torch.from_numpy(x), view_index=view)[0].numpy()
            plain = swin_v2_ref.forward(sd, torch.from_numpy(x))[0].numpy()
            assert np.abs(got - ref).max() / np.abs(ref).max() < 2e-4 and _cos_err(got, ref) < 1e-5, prec
            assert np.abs(ref - plain).max() / np.abs(ref).max() > 1e-2          # the term is not a no-op
    finally:
        eng.set_precision(0)


# ----------------------------------------------------------------------------- ranks
@pytest.mark.parametrize("layout", [64, 16, 24])
@pytest.mark.parametrize("precision", [0, 2])
def test_v2_ranks_against_reference_vectors(eng_v2, g, precision, layout):
    """64 images -> emb[64,96] -> (1 - cos) / 2 matrix -> row arg-min against what the reference's swin_t(version="v2") + cosine_dist
    gave, in one pass of 64, four passes of 16 and passes of 24 + 24 + 16.  Every row of the fixture is decided (reference top-2 gap
    above 2e-6, asserted here on the fixture), so no arg-min may differ: no allowlist."""
    gap = g["rank_gap"]
    assert float(gap.min()) > 2e-6
    base = synth.images_f32(64, int(g["rank_seed"]))
    eng_v2.set_precision(precision)
    eng_v2.set_chunk(layout)
    emb = eng_v2.swin_embed_f32_nchw(base)
    eng_v2.set_precision(0)
    eng_v2.set_chunk(1024)
    assert _cos_err(emb, g["rank_emb"]) < 1e-5
    dist = eng_v2.distmat(emb, emb, _ffi.METRIC_COS_HALF)
    err = np.abs(dist - _cosdist(g)).max()
    d = dist.copy()
    np.fill_diagonal(d, np.inf)
    flips = np.flatnonzero(d.argmin(1) != g["rank_argmin"])
    print("swin v2 ranks precision %d passes of %d: matrix error %.2e, %d arg-mins differ" % (precision, layout, err, len(flips)))
    assert err <= 2e-6                                                    # v1's matrix bar (test_swin_config_against_reference_vectors)
    assert len(flips) == 0, (flips, gap[flips])


# ----------------------------------------------------------------------------- invariance
def test_v2_embeddings_do_not_depend_on_the_pass_size(eng_v2):
    """12 images embedded in passes of 2, 5 and 12 agree bit for bit in every mode - through REID_SWIN_CHUNK_MAX in fresh processes
    (the mechanism of test_swin_embeddings_do_not_depend_on_the_pass_size) and through reid_ctx_set_chunk in this one."""
    import json
    import subprocess
    code = ("import sys, json, numpy as np; sys.path.insert(0, %r); from reid_amd import synth, weights; from reid_amd.engine import get_engine;"
            "eng = get_engine(0); eng.load_swin(*weights.pack_swin(synth.swin_state_dict(0, version='v2'))[:2]); eng.set_chunk(4096);"
            "x = synth.images_f32(12, 4); out = []\n"
            "for p in (0, 2, 1):\n"
            "    eng.set_precision(p); out.append(eng.swin_embed_f32_nchw(x).view(np.uint32).tolist())\n"
            "print(json.dumps(out))" % ROOT)

    def run(**env):
        out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, check=True).stdout
        return [np.asarray(v, np.uint32).view(np.float32) for v in json.loads(out.strip().splitlines()[-1])]

    ref = run(REID_SWIN_CHUNK_MAX="12")
    for cap in ("2", "5"):
        got = run(REID_SWIN_CHUNK_MAX=cap)
        for a, b in zip(got, ref):
            assert np.array_equal(a, b), cap
    x = synth.images_f32(12, 4)
    for mode, want in zip((0, 2, 1), ref):
        eng_v2.set_precision(mode)
        for chunk in (5, 2):
            eng_v2.set_chunk(chunk)
            assert np.array_equal(eng_v2.swin_embed_f32_nchw(x), want), (mode, chunk)
    assert np.abs(ref[1] - ref[0]).max() <= 2e-6 * np.abs(ref[0]).max()       # fp32-class against exact fp32, as for v1


# ----------------------------------------------------------------------------- mode-2 operand range
def test_v2_mode2_refuses_a_to_out_weight_it_cannot_split(eng, sd2):
    """The refusal path only (no activation is driven out of range): a v2 checkpoint with one to_out weight outside |w| 2^11 < 65504 is
    refused by name for mode 2, both ways round, and runs in mode 0."""
    from reid_amd._ffi import ReidHipError
    sd = dict(sd2)
    key = "stage3.layers.2.1.attention_block.fn.fn.to_out.weight"
    sd[key] = np.array(sd[key], copy=True)
    sd[key][5, 17] = 40.0
    bad = weights.pack_swin(sd)[:2]
    try:
        eng.set_precision(0)
        eng.load_swin(*bad)
        assert np.isfinite(eng.swin_embed_f32_nchw(synth.images_f32(1, 2))).all()
        assert not eng.precision_ok(1, 2)
        with pytest.raises(ReidHipError, match=r"s3\.b5\.out\.w"):
            eng.set_precision(2)
        eng.load_swin(*weights.pack_swin(sd2)[:2])
        eng.set_precision(2)
        with pytest.raises(ReidHipError, match=r"s3\.b5\.out\.w"):
            eng.load_swin(*bad)
    finally:
        eng.set_precision(0)
        eng.load_swin(*weights.pack_swin(synth.swin_state_dict(0))[:2])


# ----------------------------------------------------------------------------- the kernels alone
def _attn_case(h, w, heads, n, seed):
    rng = np.random.default_rng(seed)
    c = heads * 32
    qkv = rng.normal(0, 1.5, (n, h, w, 3 * c)).astype(np.float32)
    qkv[0, h // 2, w // 3, 0:32] = 0.0                     # an all-zero q row (head 0) ...
    qkv[0, h - 1, w - 2, c + 32:c + 64] = 0.0              # ... and an all-zero k row (head 1): the max(norm, 1e-12) rule
    bias = rng.normal(0, 1.5, (heads, 49, 49)).astype(np.float32)
    scale = np.exp(rng.uniform(np.log(2.0), np.log(100.0), heads)).astype(np.float32)
    scale[heads - 1] = np.float32(np.exp(np.float64(np.float32(np.log(100.0)))))     # a head at the clamp (100.00001 in fp32)
    return qkv, bias, scale


@pytest.mark.parametrize("shifted", [0, 1])
@pytest.mark.parametrize("geom", ["stage1", "stage4"])
def test_window_attn_cos_kernel_against_float64(eng, geom, shifted):
    """window_attn_cos_kernel alone against the formula in float64 (swin_v2_ref.window_attention): stage-1 (56 x 56 tokens, 3 heads) and
    stage-4 (7 x 7, 24 heads) geometry, shifted and not - shifted, the windows of the last row / column mask a query's row down to as
    few as 9 keys; at 7 x 7 the one window is both.  Bars: the fp32 build may err at most 4 times what the same formula evaluated
    in fp32 by torch on the CPU errs on the same inputs (another summation order); the pair build may add 2^-21 max|out| for its 22-bit
    result; the f16 build is compared on the f16-rounded inputs with 2^-10 max|out| added."""
    h, w, heads = (56, 56, 3) if geom == "stage1" else (7, 7, 24)
    qkv, bias, scale = _attn_case(h, w, heads, 2, 7 + shifted)
    tb, ts = torch.from_numpy(bias), torch.from_numpy(scale)

    def oracle(q):
        ref = swin_v2_ref.window_attention(torch.from_numpy(q).double(), heads, shifted, tb.double(), ts.double()).numpy()
        cpu = swin_v2_ref.window_attention(torch.from_numpy(q), heads, shifted, tb, ts).numpy()
        return ref, float(np.abs(cpu - ref).max())

    ref, cpu_err = oracle(qkv)
    amax = float(np.abs(ref).max())
    got0 = eng.debug_window_attn_cos(0, qkv, bias, scale, shifted)
    got2 = eng.debug_window_attn_cos(2, qkv, bias, scale, shifted)
    q16 = qkv.astype(np.float16).astype(np.float32)
    ref16, cpu_err16 = oracle(q16)
    got1 = eng.debug_window_attn_cos(1, qkv, bias, scale, shifted)
    e0, e2, e1 = float(np.abs(got0 - ref).max()), float(np.abs(got2 - ref).max()), float(np.abs(got1 - ref16).max())
    print("window_attn_cos %s shifted %d: max|out| %.3f; cpu fp32 error %.3e; kernel fp32 %.3e, pair %.3e (bar %.3e); f16 inputs: cpu %.3e, "
          "kernel %.3e (bar %.3e)" % (geom, shifted, amax, cpu_err, e0, e2, 4 * cpu_err + 2.0 ** -21 * amax, cpu_err16, e1,
                                      4 * cpu_err16 + 2.0 ** -10 * float(np.abs(ref16).max())))
    assert np.isfinite(got0).all() and np.isfinite(got2).all() and np.isfinite(got1).all()
    assert e0 <= 4 * cpu_err
    assert e2 <= 4 * cpu_err + 2.0 ** -21 * amax
    assert e1 <= 4 * cpu_err16 + 2.0 ** -10 * float(np.abs(ref16).max())


@pytest.mark.parametrize("c", [96, 192, 384, 768])
def test_post_norm_kernel_against_float64(eng, c):
    """post_norm_kernel alone: out = x + (LayerNorm(y) g + b) over a ragged number of rows (1003: neither 4 nor 8 divides it) of every
    stage's width, against float64.  Bar: 4 times the error of torch's fp32 evaluation on the CPU; the pair / f16 side output
    reconstructs out to 2^-21 / 2^-10 of max|out|; writing over x gives the same bits."""
    rng = np.random.default_rng(c)
    t = 1003
    x = rng.normal(0, 2.0, (t, c)).astype(np.float32)
    y = (rng.normal(0, 1.0, (t, c)) * rng.uniform(0.1, 8.0, (t, 1)) + rng.normal(0, 3.0, (t, 1))).astype(np.float32)
    gw, gb = rng.uniform(0.5, 1.5, c).astype(np.float32), rng.normal(0, 0.1, c).astype(np.float32)
    tx, ty, tg, tb = (torch.from_numpy(a) for a in (x, y, gw, gb))
    ref = swin_v2_ref.post_norm(tx.double(), ty.double(), tg.double(), tb.double()).numpy()
    cpu_err = float(np.abs(swin_v2_ref.post_norm(tx, ty, tg, tb).numpy() - ref).max())
    amax = float(np.abs(ref).max())
    out0, _ = eng.debug_post_norm(0, x, y, gw, gb)
    out1, side1 = eng.debug_post_norm(1, x, y, gw, gb)
    out2, side2 = eng.debug_post_norm(2, x, y, gw, gb)
    outp, _ = eng.debug_post_norm(0, x, y, gw, gb, in_place=True)
    errs = [float(np.abs(o - ref).max()) for o in (out0, out1, out2)]
    print("post_norm c %d: cpu fp32 error %.3e, kernel %s (bar %.3e); side f16 %.3e (bar %.3e), pair %.3e (bar %.3e)"
          % (c, cpu_err, ["%.3e" % e for e in errs], 4 * cpu_err, np.abs(side1 - out1).max(), 2.0 ** -10 * amax,
             np.abs(side2 - out2.astype(np.float64)).max(), 2.0 ** -21 * amax))
    for e in errs:
        assert e <= 4 * cpu_err
    assert np.array_equal(out0, out1) and np.array_equal(out0, out2) and np.array_equal(out0, outp)
    assert np.abs(side1 - out1).max() <= 2.0 ** -10 * amax
    assert np.abs(side2 - out2.astype(np.float64)).max() <= 2.0 ** -21 * amax
