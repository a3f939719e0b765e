"""The streaming forms of the block tails, bit for bit (csrc/elementwise.hip: se_tail_kernel, in_apply_pack_kernel, gem_neck_kernel from the
tail), through the debug harness (eng.debug_se_tail, eng.debug_norm_finish, eng.debug_gem_neck_fused).  tests/test_gpu_tail.py bounds these
kernels against float64 oracles at the network's layer shapes; here the shapes are small ones chosen by the launchers' own rules so that a
thread of the unrolled-by-four loops makes 1 / 2 (threads differ), 4, 5, 7, 8 and 10 trips, rows are 16, 64 and 128 chunks wide (and 24,
which takes the general loop), and the slices of a large pass are reached.  Every comparison is np.testing.assert_array_equal.

References are kernels this file's subject does not share code with: se_finalize_kernel + se_combine_kernel (SE tail form 0) and
in_apply_kernel (IBN finish form 1).

The gate of the SE operands.  se_finalize_kernel sums the hidden units' dot products one channel per lane, se_tail_kernel four channels per
lane: the two gates agree only to rounding on general operands (tests/test_gpu_tail.py bounds both), so form 0 is a bit-exact reference only
where no sum of the gate rounds.  gate="exact" operands are built that way - per-tile sums hw * {-1, 0, 1}, w1 in {-1, 0, 1}, w2 in
{-3 .. 3} times a power of two: every partial sum of either kernel is an integer (times that power) far below 2^24, so both form the same pre-sigmoid value
and the same expf of it - and every shape is checked against form 0 with them.  gate="random" operands round in the gate; with them the
three kernels of launch_se_tail (the rule's, <false>, <true>) are compared with one another, which holds the gate's operation order of the
two templates together as tests/test_gpu_tail.py::test_se_tail does at the layer shapes.
"""
import numpy as np
import pytest

from reid_amd import _ffi

gpu = pytest.mark.gpu

NF_IN_APPLY, NF_PACK, NF_PACK_IN = 1, 2, 3
SE_COMBINE, SE_RULE, SE_GENERAL, SE_SMALL = 0, 1, 4, 7   # + 0 fp32 out, + 1 packed, + 2 both


def tail_slices(n, hw):      # elementwise.hip tail_slices
    s = 1
    while n * s < 1024 and hw // (s * 2) >= 16 and hw % (s * 2) == 0:
        s *= 2
    return s


def pack_rows(n, hw):        # elementwise.hip launch_in_apply_pack
    rows = 128
    while n * (hw // rows) < 512 and rows > 16:
        rows >>= 1
    return rows


# (n, hw, c, mid): what a thread of the block does in the streaming loop (rows c/4 items over 256 threads)
SE_SHAPES = [
    ((3, 384, 64, 4), (24, "1-2")),      # 384 items: threads 0-127 make two trips, the others one (remainder loop only)
    ((128, 640, 64, 4), (80, "5")),      # one unrolled trip of four + one
    ((128, 896, 64, 4), (112, "7")),     # + three
    ((256, 640, 64, 4), (160, "10")),    # two unrolled + two
    ((1024, 128, 64, 4), (128, "8")),    # a large pass: one block per image, two unrolled trips
    ((2, 128, 512, 32), (16, "8")),      # rows of 128 chunks: two pixels per trip
    ((3, 128, 256, 16), (16, "4")),      # rows of 64 chunks
    ((2, 128, 96, 8), (16, "1-2")),      # rows of 24 chunks do not divide the block: the general loop
]


def trips(rows, c):
    items = rows * (c // 4)
    lo, hi = items // 256, -(-items // 256)
    return "%d" % hi if lo == hi else "%d-%d" % (lo, hi)


def test_shapes_reach_what_they_say():
    for (n, hw, c, mid), (rows, t) in SE_SHAPES:
        assert hw % tail_slices(n, hw) == 0 and hw // tail_slices(n, hw) == rows, (n, hw, rows)
        assert trips(rows, c) == t, (n, hw, c, trips(rows, c))
    # every remainder of an unroll by four, below and above one unrolled trip, and threads that differ
    assert {t for _, (_, t) in SE_SHAPES} >= {"1-2", "4", "5", "7", "8", "10"}
    for (n, hw, c, half), rows in PACK_SHAPES:
        assert pack_rows(n, hw) == rows, (n, hw, pack_rows(n, hw))


def split16(v):
    """[xh | xl'] of fp32 v [m, k]: xh = f16(v), xl' = f16((v - xh) 2^11), as uint16 bits."""
    v = np.asarray(v, np.float32)
    hi = v.astype(np.float16)
    lo = ((v - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return hi.view(np.uint16), lo.view(np.uint16)


@pytest.fixture(scope="module")
def eng():
    from reid_amd import synth, weights
    from reid_amd.engine import get_engine
    e = get_engine(0)
    blob, manifest, _ = weights.pack_seres18(synth.seres18_state_dict(0))
    e.load_seres18(blob, manifest)
    yield e
    e.clear_fault()


# ----------------------------------------------------------------------------- SE tail
def se_operands(n, hw, c, mid, tiles, gate, seed):
    rng = np.random.default_rng(seed)
    if gate == "exact":
        s0 = rng.integers(-1, 2, (n, tiles, c)).astype(np.float32) * np.float32(hw)
        w1 = rng.integers(-1, 2, (mid, c)).astype(np.float32)
        w2t = rng.integers(-3, 4, (mid, c)).astype(np.float32)
        pre = np.maximum(s0.sum(1) / hw @ w1.T, 0) @ w2t            # exact in fp32: integers below 2^24
        w2t = w2t * np.float32(2.0) ** -int(np.ceil(np.log2(pre.std())))   # a power of two: a pre-sigmoid spread of about one
    else:
        s0 = (rng.normal(size=(n, tiles, c)) * hw / tiles).astype(np.float32)
        w1 = (rng.normal(size=(mid, c)) / np.sqrt(c) * 2).astype(np.float32)
        w2t = (rng.normal(size=(mid, c)) / np.sqrt(mid) * 2).astype(np.float32)
    stats = np.stack([s0, np.ones_like(s0)], -1)
    y = rng.normal(size=(n, hw, c)).astype(np.float32)
    sc = rng.normal(size=(n, hw, c)).astype(np.float32)
    return stats, w1, w2t, y, sc


SE_CASES = [(s, t) for (s, _), t in zip(SE_SHAPES, (17, 5, 7, 1, 1, 1, 16, 2))]   # tiles of the partial sums: 1, some, 16 (one batch of loads), 17 (two)


@gpu
@pytest.mark.parametrize("shape,tiles", SE_CASES, ids=["n%d-hw%d-c%d-m%d" % s for s, _ in SE_CASES])
def test_se_tail_forms_equal_finalize_and_combine(eng, shape, tiles):
    n, hw, c, mid = shape
    stats, w1, w2t, y, sc = se_operands(n, hw, c, mid, tiles, "exact", n + hw)
    want, _, gate = eng.debug_se_tail(SE_COMBINE, stats, w1, w2t, y, sc)
    assert np.isfinite(want).all() and gate.min() < 0.4 and gate.max() > 0.6 and 0.2 < (want == 0).mean() < 0.8, \
        "the operands do not exercise the gate or the ReLU"
    hi, lo = split16(want.reshape(-1, c))
    for form in range(1, 10):
        out, pk, _ = eng.debug_se_tail(form, stats, w1, w2t, y, sc)
        what = "n=%d hw=%d c=%d mid=%d form %d" % (n, hw, c, mid, form)
        if (form - 1) % 3 != 1:
            np.testing.assert_array_equal(out, want, err_msg=what + ": fp32 out")
        else:
            assert out is None
        if (form - 1) % 3 != 0:
            np.testing.assert_array_equal(pk[:, :c], hi, err_msg=what + ": oh")
            np.testing.assert_array_equal(pk[:, c:], lo, err_msg=what + ": ol'")
        else:
            assert pk is None
    assert eng.fault_bits() == 0


@gpu
@pytest.mark.parametrize("shape,tiles", SE_CASES[:1] + SE_CASES[5:7], ids=["n%d-hw%d-c%d-m%d" % s for s, _ in SE_CASES[:1] + SE_CASES[5:7]])
def test_se_tail_kernels_agree_on_a_rounding_gate(eng, shape, tiles):
    n, hw, c, mid = shape
    stats, w1, w2t, y, sc = se_operands(n, hw, c, mid, tiles, "random", n + hw + 1)
    rule, rule_pk, _ = eng.debug_se_tail(SE_RULE + 2, stats, w1, w2t, y, sc)
    assert np.isfinite(rule).all()
    for form in (SE_GENERAL + 2, SE_SMALL + 2):
        out, pk, _ = eng.debug_se_tail(form, stats, w1, w2t, y, sc)
        np.testing.assert_array_equal(out, rule, err_msg="form %d fp32 out" % form)
        np.testing.assert_array_equal(pk, rule_pk, err_msg="form %d packed" % form)


# ----------------------------------------------------------------------------- IBN finish
# (n, hw, c, half): rows of launch_in_apply_pack
PACK_SHAPES = [
    ((2, 128, 64, 32), 16),       # in_only: 128 items for 256 threads; full: one trip
    ((600, 128, 64, 32), 128),    # a large pass: 128 rows, the most a block gets (in_only four trips, full eight)
    ((600, 256, 128, 64), 128),   # two slices per image (eight and sixteen trips)
    ((5, 384, 256, 128), 16),
    ((3, 128, 96, 48), 16),       # 12 / 24 chunks do not divide the block: the general loop
]
PACK_CASES = [(s, t) for (s, _), t in zip(PACK_SHAPES, (1, 16, 1, 16, 17))]


@gpu
@pytest.mark.parametrize("shape,tiles", PACK_CASES, ids=["n%d-hw%d-c%d-t%d" % (s[0], s[1], s[2], t) for s, t in PACK_CASES])
def test_in_apply_pack_equals_in_apply(eng, shape, tiles):
    n, hw, c, half = shape
    rng = np.random.default_rng(n + hw + c)
    x = rng.normal(size=(n, hw, c)).astype(np.float32)
    s1 = (rng.normal(size=(n, tiles, c)) * 0.3 * hw / tiles).astype(np.float32)
    s2 = (rng.uniform(1.0, 2.0, (n, tiles, c)) * hw / tiles).astype(np.float32)
    stats = np.stack([s1, s2], -1)
    gamma = rng.uniform(0.5, 1.5, half).astype(np.float32)
    beta = rng.normal(size=half).astype(np.float32)
    v32 = eng.debug_norm_finish(NF_IN_APPLY, x, stats, gamma, beta)[0]
    np.testing.assert_array_equal(v32[..., half:], x[..., half:])
    assert (v32[..., :half] == 0).mean() > 0.1 and (v32[..., :half] > 0).mean() > 0.1
    hi, lo = split16(v32[..., :half].reshape(-1, half))
    bh, bl = split16(x[..., half:].reshape(-1, c - half))
    for form in (NF_PACK, NF_PACK_IN):
        out, pk, _, _ = eng.debug_norm_finish(form, x, stats, gamma, beta)
        what = "n=%d hw=%d c=%d half=%d tiles=%d in_only=%d" % (n, hw, c, half, tiles, form == NF_PACK_IN)
        np.testing.assert_array_equal(out, x, err_msg=what + ": its fp32 input")
        np.testing.assert_array_equal(pk[:, :half], hi, err_msg=what + ": xh")
        np.testing.assert_array_equal(pk[:, c:c + half], lo, err_msg=what + ": xl'")
        if form == NF_PACK:
            np.testing.assert_array_equal(pk[:, half:c], bh, err_msg=what + ": BatchNorm half xh")
            np.testing.assert_array_equal(pk[:, c + half:], bl, err_msg=what + ": BatchNorm half xl'")
        else:
            assert (pk[:, half:c] == 0xffff).all() and (pk[:, c + half:] == 0xffff).all(), what + ": BatchNorm half written"
    assert eng.fault_bits() == 0


# ----------------------------------------------------------------------------- GeM from the tail
def gem_operands(hw, seed):
    n, c, mid = 3, 512, 32
    stats, w1, w2t, y, sc = se_operands(n, hw, c, mid, 1, "random", seed)
    rng = np.random.default_rng(seed + 1)
    scale = rng.uniform(-2, 2, c).astype(np.float32)
    shift = rng.normal(size=c).astype(np.float32)
    return stats, w1, w2t, y, sc, scale, shift


GEM_CASES = [(hw, p) for hw in (128, 1, 17, 200) for p in (3.0, 6.5)]


@gpu
@pytest.mark.parametrize("hw,p", GEM_CASES, ids=["hw%d-p%g" % c for c in GEM_CASES])
def test_gem_from_the_tail_equals_tail_then_gem(eng, hw, p):
    stats, w1, w2t, y, sc, scale, shift = gem_operands(hw, 300 + hw)
    x = eng.debug_se_tail(SE_GENERAL, stats, w1, w2t, y, sc)[0]
    assert (x == 0).mean() > 0.2 and (x > 0).mean() > 0.2
    g, e = eng.debug_gem_neck(x, p, scale, shift)
    fg, fe = eng.debug_gem_neck_fused(stats, w1, w2t, y, sc, p, scale, shift)
    np.testing.assert_array_equal(fg, g, err_msg="gem")
    np.testing.assert_array_equal(fe, e, err_msg="emb")
    assert eng.fault_bits() == 0


@gpu
def test_gem_from_the_tail_raises_the_embedding_fault(eng):
    stats, w1, w2t, y, sc, scale, shift = gem_operands(128, 77)
    y[1, 5, 77] = np.inf
    x = eng.debug_se_tail(SE_GENERAL, stats, w1, w2t, y, sc)[0]     # no packed store: no range guard, +inf passes the ReLU
    assert np.isinf(x[1, 5, 77])
    try:
        for call in (lambda: eng.debug_gem_neck(x, 3.0, scale, shift), lambda: eng.debug_gem_neck_fused(stats, w1, w2t, y, sc, 3.0, scale, shift)):
            with pytest.raises(_ffi.ReidHipError) as ei:
                call()
            assert ei.value.status == -3 and eng.fault_bits() == 2
            eng.clear_fault()
    finally:
        eng.clear_fault()
