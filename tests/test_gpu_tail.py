"""The kernels that finish a residual block and the neck, each launch form against a float64 oracle (debug harnesses
reid_debug_norm_finish, reid_debug_se_tail, reid_debug_gem_neck; csrc/elementwise.hip, csrc/elementwise_f16.hip).

Every call goes through the launcher the forward calls, so each case sees the forward's grid and slicing; TAIL_CASES records the
slices, rows and variant each (shape, batch) pair reaches.  Outputs a launch leaves alone read as NaN (0xffff): every output is checked
for that densely.  Run on an MI355X: pytest -m gpu tests/test_gpu_tail.py.

Error model: u = 2^-24 (fp32 unit roundoff), an f16 result carries a half-ulp of 2^-11 relative (2^-25 absolute below f16's normal range).
SAFETY = 2 (chosen) multiplies every derived bound.

InstanceNorm finish from given stats.  mean = s1/hw, var = max(s2/hw - mean^2, 0), a = g/sqrt(var + 1e-5), b = beta - mean a.  The device
sums the per-group fp32 partials and does this arithmetic in fp64, then rounds a and b once: a and b are within 1 fp32 ulp of the
float64 values (asserted as such).  An applied output relu(x a + b) is within |x| ulp(a) + ulp(b) + 2u (|x a| + |b|) (one rounding of
the product, one of the sum, or one of a fused multiply-add), plus the f16 half-ulp of the result for precision 1; ReLU is 1-Lipschitz.
The packed form [xh | xl'] equals, bit for bit, the split of the kernel's own fp32 value (taken from in_apply on the same operands, whose
arithmetic is the same expression), and xh + xl' 2^-11 is within bound + 2^-21 |v| + 2^-35 of the oracle (the rounding of xl').

InstanceNorm finish from the convolution's own stats (chained).  The convolution output v' is within b_v of the float64 output v
(test_gpu_conv.bound, SAFETY included).  Per (image, channel) over hw pixels:
  d_mean = (sum b_v + 128u sum|v|) / hw                             (conv error + the fp32 128-row group sums)
  d_var  = (sum (2|v| b_v + b_v^2) + 129u sum v^2) / hw + 2|mean| d_mean + d_mean^2
  rel(1/std) <= CANCEL + (d_var - 129u E[v^2]) / (2 (var + eps)),  CANCEL = 1/2 129u E[v^2] / (var + eps)
CANCEL is the variance cancellation of s2/hw - mean^2: it grows with (mean/std)^2.  The output y = relu(g (v - mean) / std + beta) is
then within |g|/std (b_v + d_mean) + |g (v - mean)|/std rel(1/std) + 2u (|v a| + |b|) + ulp(a)|v| + ulp(b).  Recorded on an MI355X
(not asserted against torch): the target mean/std 0 gives a median of 1.7-2.7 (x >= 1 leaves every channel a mean); "torch" is torch's
CPU fp32 instance_norm of the same fp32 convolution output, against the same float64 oracle.

  layer prec  mean/std  max |err|  err/bound  CANCEL max  torch fp32 max |err|
  l3    0      1.7      1.07e-5    <0.001     2.5e-4      1.07e-5
  l3    0      2.3      2.12e-5    <0.001     7.7e-4      1.17e-5
  l3    0     30.8      7.28e-4    <0.001     2.0e-2      5.94e-5
  l3    2      1.7      1.13e-5    <0.001     2.4e-4      8.01e-6
  l3    2      2.8      1.65e-5    <0.001     5.5e-4      9.14e-6
  l3    2     30.6      9.15e-4    <0.001     1.8e-2      3.08e-5
  l2    0      2.7      1.02e-5    <0.001     3.0e-4      6.82e-6
  l2    0      3.2      1.09e-5    <0.001     5.3e-4      8.59e-6
  l2    0     30.7      4.62e-4     0.001     1.5e-2      3.97e-5
  l2    2      2.6      6.97e-6    <0.001     2.8e-4      6.69e-6
  l2    2      3.2      1.93e-5    <0.001     7.1e-4      8.57e-6
  l2    2     30.2      2.77e-4     0.001     1.3e-2      3.22e-5
At mean/std 30 the device is 7-30x further from float64 than torch's CPU fp32 InstanceNorm: the s2/hw - mean^2 cancellation, which the
stats format (sum and sum of squares per 128-row group) sets.  The worst-case bound is far above what random rounding gives.

SE.  pooled = sum_t stats[..., 0] / hw, h = relu(W1 pooled), g = sigmoid(W2^T h), out = relu(g y + sc).  Hidden units: c u sum|w1||pooled|
(the fp32 dot product and the rounding of pooled); the gate: 1/4 (mid u sum|w2||h| + sum|w2| d_h) (sigmoid' <= 1/4) + 4u g for expf,
the add and the division (a few ulp, chosen); the output: |y| d_g + 2u (|g y| + |sc|), plus the f16 rounding for precision 1.
se_tail_kernel<true> is "the same operations in the same order" as <false>: asserted bit for bit wherever both are legal.

GeM + BNNeck.  m = mean(max(x, 1e-6)^p), g = m^(1/p), emb = g scale + shift.  Each term is positive, so the fp32 sum over hw pixels
(per thread, then 16 or 32 partials) is within (hw + 32) u of m relative, and a term's own relative error E_term adds to that:
p == 3: x x x, E_term = 2u; f16 and a trained p: ocml powf, E_term = 4u (chosen); fp32 and a trained p: exp2(p log2 x) on
v_log_f32 / v_exp_f32, E_term = E_EXP + ln2 (|p| E_LOG max(|log2 x|, 1) + u |p log2 x|); a trained-p term below 2^-126 (a clamped
1e-6 at p > 6.3) is a subnormal and adds 2^-150 / x^p.  No document on the build machine states the
accuracy of v_log_f32 / v_exp_f32, so E_LOG = E_EXP = 2^-22 is chosen, and test_trans_accuracy measures the composite on the device
(p = 1, one pixel: m = exp2(log2 x) exactly as the kernel forms it): on an MI355X its worst relative error over x in [1e-6, 1e3] was
1.42e-6 (24 u), 0.52 of the model.  Then rel(g) <= rel(m)/p + |ln m| u/p + 4u
(the rounding of 1/p, and powf / cbrtf: chosen), and emb is within |scale| g rel(g) + 2u (|g scale| + |shift|).

Range fault of the packed writers: an activation whose magnitude (as bits) reaches 65504 = 0x477fe000 before the ReLU raises fault bit 0
(value 1); 65503.996 does not.  A non-finite embedding raises fault bit 1 (value 2).  The calls fail with REID_ERR_STATE until cleared.
"""
import numpy as np
import pytest

from reid_amd import _ffi

gpu = pytest.mark.gpu

U = 2.0 ** -24
H16 = 2.0 ** -11            # f16 half-ulp, relative
H16_ABS = 2.0 ** -25        # ... and below f16's normal range
SAFETY = 2.0                # chosen
EPS = 1e-5
E_LOG = E_EXP = 2.0 ** -22  # chosen; test_trans_accuracy measures the composite (module docstring)
N_RANDOM_PIX = 64           # seeded pixels on top of the structural ones (chosen)

# name: (hw, c, half, mid) of the layers at 256 x 128 crops (layer 4 has no IBN)
LAYERS = {"l1": (2048, 64, 32, 8), "l2": (512, 128, 64, 8), "l3": (128, 256, 128, 16), "l4": (128, 512, None, 32),
          "syn": (128, 64, 4, 8), "syn128": (128, 64, 32, 8)}

NF_FINALIZE, NF_IN_APPLY, NF_PACK, NF_PACK_IN, NF_F16, NF_F16_AFFINE = range(6)
SE_COMBINE, SE_RULE, SE_GENERAL, SE_SMALL, SE_F16, SE_F16_COMBINE = 0, 1, 4, 7, 10, 11   # + 0 fp32 out, + 1 packed, + 2 both


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


def se_small(n, hw, c, mid):  # elementwise.hip launch_se_tail
    return tail_slices(n, hw) * n <= 512 and c >= 512 and mid <= 32


# (layer, n, what it reaches).  The batch sizes sit on both sides of launch_in_apply_pack's rows rule, tail_slices and launch_se_tail's
# SMALL rule; test_tail_cases_reach_what_they_say checks the column against the rules above.
TAIL_CASES = [
    ("l3", 127, "pack rows 16"), ("l3", 128, "pack rows 32"), ("l3", 255, "pack rows 32"), ("l3", 256, "pack rows 64"),
    ("l3", 511, "pack rows 64"), ("l3", 512, "pack rows 128"),
    ("l1", 16, "slices 64"), ("l1", 17, "slices 64"), ("l1", 31, "slices 64"), ("l1", 32, "slices 32"),
    ("l2", 3, "slices 32"), ("syn128", 1023, "slices 2"), ("syn128", 1024, "slices 1"), ("syn", 5, "slices 8"),
    ("l4", 1, "se small, slices 8"), ("l4", 64, "se small, slices 8"), ("l4", 65, "se general, slices 8"),
]


def reached(layer, n):
    hw, c, half, mid = LAYERS[layer]
    out = []
    if half and hw % 128 == 0:
        out.append("pack rows %d" % pack_rows(n, hw))
    out.append("slices %d" % tail_slices(n, hw))
    if c >= 512:
        out.append("se %s, slices %d" % ("small" if se_small(n, hw, c, mid) else "general", tail_slices(n, hw)))
    return out


def test_tail_cases_reach_what_they_say():
    for layer, n, what in TAIL_CASES:
        assert what in reached(layer, n), (layer, n, what, reached(layer, n))
    assert not se_small(65, 128, 512, 32) and se_small(64, 128, 512, 32) and not se_small(1, 128, 512, 33)


# ----------------------------------------------------------------------------- float64 oracles
def in_oracle(stats, hw, gamma, beta, bn_scale=None, bn_shift=None):
    """(a, b) [n, c] float64: InstanceNorm on the first len(gamma) channels from stats [n, tiles, c, 2], BatchNorm on the rest."""
    s = stats.astype(np.float64).sum(1)
    half = len(gamma)
    mean = s[:, :half, 0] / hw
    var = np.maximum(s[:, :half, 1] / hw - mean * mean, 0.0)
    a_in = np.asarray(gamma, np.float64) / np.sqrt(var + EPS)
    b_in = np.asarray(beta, np.float64) - mean * a_in
    n, c = s.shape[:2]
    a, b = np.empty((n, c)), np.empty((n, c))
    a[:, :half], b[:, :half] = a_in, b_in
    if c > half:
        a[:, half:], b[:, half:] = np.asarray(bn_scale, np.float64), np.asarray(bn_shift, np.float64)
    return a, b


def ulp32(v):
    return np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)


def applied(x, a, b, pix, f16=False):
    """relu(x a + b) on the flat pixels `pix` of x [n, hw, c] and its bound."""
    n, hw, c = x.shape
    img = pix // hw
    xv = x.reshape(-1, c)[pix].astype(np.float64)
    aa, bb = a[img], b[img]
    v = np.maximum(xv * aa + bb, 0.0)
    bound = np.abs(xv) * ulp32(aa) + ulp32(bb) + 2 * U * (np.abs(xv * aa) + np.abs(bb))
    if f16:
        bound = bound + H16 * v + H16_ABS
    return v, SAFETY * bound


def split16(v):
    """[xh | xl'] of fp32 v [m, k]: xh = f16(v), xl' = f16((v - xh) 2^11), as uint16 bits."""
    v = np.asarray(v, np.float32)
    hi = v.astype(np.float16)
    lo = ((v - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return hi.view(np.uint16), lo.view(np.uint16)


def se_oracle(stats, hw, w1, w2t):
    """(g [n, c], its bound) float64."""
    pooled = stats[..., 0].astype(np.float64).sum(1) / hw
    w1d, w2d = w1.astype(np.float64), w2t.astype(np.float64)
    c, mid = w1.shape[1], w1.shape[0]
    h = np.maximum(pooled @ w1d.T, 0.0)
    dh = c * U * (np.abs(pooled) @ np.abs(w1d).T)
    g = 1.0 / (1.0 + np.exp(-(h @ w2d)))
    dz = mid * U * (h @ np.abs(w2d)) + dh @ np.abs(w2d)
    return g, SAFETY * (0.25 * dz + 4 * U * g)


def se_out(y, sc, g, dg, pix, f16=False):
    n, hw, c = y.shape
    img = pix // hw
    yv, sv = y.reshape(-1, c)[pix].astype(np.float64), sc.reshape(-1, c)[pix].astype(np.float64)
    gy = g[img] * yv
    v = np.maximum(gy + sv, 0.0)
    bound = np.abs(yv) * dg[img] + SAFETY * 2 * U * (np.abs(gy) + np.abs(sv))
    if f16:
        bound = bound + SAFETY * (H16 * v + H16_ABS)
    return v, bound


def gem_oracle(x, p, scale, shift, f16=False):
    """(g, emb, bound of g, bound of emb) [n, c] float64 for x [n, hw, c]."""
    n, hw, c = x.shape
    f = np.maximum(x.astype(np.float64), float(np.float32(1e-6)))
    pd = float(np.float32(p))
    t = f ** pd
    if np.float32(p) == np.float32(3.0):
        e_term = 2 * U + 0 * t
    elif f16:
        e_term = 4 * U + 2.0 ** -150 / t
    else:
        l2 = np.abs(np.log2(f))
        e_term = E_EXP + np.log(2) * (abs(pd) * E_LOG * np.maximum(l2, 1.0) + U * abs(pd) * l2) + 2.0 ** -150 / t
    m = t.mean(1)
    rel_m = (hw + 32) * U + (e_term * t).sum(1) / t.sum(1) + U
    g = m ** (1.0 / pd)
    rel_g = rel_m / pd + np.abs(np.log(m)) * U / pd + 4 * U
    sc, sh = scale.astype(np.float64), shift.astype(np.float64)
    emb = g * sc + sh
    bg = SAFETY * rel_g * g
    be = SAFETY * (np.abs(sc) * g * rel_g + 2 * U * (np.abs(g * sc) + np.abs(sh)))
    return g, emb, bg, be


def sample_pix(n, hw, seed, dense_below=1 << 15):
    """Flat pixel indices to check: all of them for small launches; else every pixel of the first, last and a seeded image, the first and
    last pixel of every 16-row slice (the smallest slice any launcher makes) of every image, and seeded pixels."""
    m = n * hw
    if m <= dense_below:
        return np.arange(m)
    rng = np.random.default_rng(seed)
    imgs = {0, n - 1, int(rng.integers(n))}
    parts = [np.arange(i * hw, (i + 1) * hw) for i in imgs]
    starts = (np.arange(n)[:, None] * hw + np.arange(0, hw, 16)[None]).reshape(-1)
    parts += [starts, starts + 15, rng.choice(m, N_RANDOM_PIX, replace=False)]
    return np.unique(np.concatenate(parts))


def check(got, want, bound, what):
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), "%s: non-finite (unwritten?) output" % what
    err = np.abs(got - want)
    worst = np.unravel_index(np.argmax(err / np.maximum(bound, 1e-300)), err.shape)
    assert (err <= bound).all(), "%s: at %s got %r, float64 %r, bound %g" % (what, worst, got[worst], want[worst], bound[worst])
    return float((err / np.maximum(bound, 1e-300)).max())


def f16_bits(a):
    return np.asarray(a, np.float32).astype(np.float16).view(np.uint16)


def from16(bits):
    return np.asarray(bits, np.uint16).view(np.float16).astype(np.float64)


# ----------------------------------------------------------------------------- operands
def norm_operands(layer, n, seed, f16=False):
    """x [n, hw, c], stats [n, tiles, c, 2] (fp32 sums of x over 128-pixel groups), gamma / beta [half], bn scale / shift [c - half].
    Edges: channel 0 constant with its s2 rounded below hw mean^2 (the clamp), channel 1 at mean/std 1e3, gamma < 0 and = 0."""
    hw, c, half, _ = LAYERS[layer]
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, hw, c)) * rng.uniform(0.5, 2, c) + rng.normal(size=c)
    x[:, :, 0] = 7.25
    x[:, :, 1] = 1e3 + rng.normal(size=(n, hw))
    x = x.astype(np.float32)
    if f16:
        x = x.astype(np.float16).astype(np.float32)
    gr = x.reshape(n, hw // 128, 128, c).astype(np.float64)
    stats = np.stack([gr.sum(2), (gr * gr).sum(2)], -1).astype(np.float32)
    stats[:, :, 0, 1] = np.float32(128 * 7.25 * 7.25 * (1 - 4e-7))   # var = -4e-7 mean^2 = -2e-5 < -eps: without the clamp, NaN
    gamma = rng.uniform(0.5, 1.5, half).astype(np.float32)
    gamma[2 % half] = -1.25
    gamma[3 % half] = 0.0
    beta = rng.normal(size=half).astype(np.float32)
    bns = rng.uniform(-1.5, 1.5, c - half).astype(np.float32)
    bnh = rng.normal(size=c - half).astype(np.float32)
    return x, stats, gamma, beta, bns, bnh


def per_image_stats(stats):   # the c64 f16 layout: one group per image
    return stats.astype(np.float64).sum(1, keepdims=True).astype(np.float32)


# ----------------------------------------------------------------------------- CPU: the oracles
def test_in_oracle_is_instance_norm():
    import torch
    x, stats, gamma, beta, bns, bnh = norm_operands("syn128", 3, 1)
    hw, c, half, _ = LAYERS["syn128"]
    xd = x.astype(np.float64)
    g = xd.reshape(3, hw // 128, 128, c)
    st = np.stack([g.sum(2), (g * g).sum(2)], -1)        # exact sums: the oracle is then InstanceNorm
    a, b = in_oracle(st, hw, gamma, beta, bns, bnh)
    ref = torch.nn.functional.instance_norm(torch.from_numpy(xd[:, :, :half]).permute(0, 2, 1), None, None,
                                            torch.from_numpy(gamma.astype(np.float64)), torch.from_numpy(beta.astype(np.float64)),
                                            True, 0.0, EPS).permute(0, 2, 1).numpy()
    np.testing.assert_allclose(xd[:, :, :half] * a[:, None, :half] + b[:, None, :half], ref, rtol=1e-9, atol=1e-9)
    np.testing.assert_array_equal(a[:, half:], np.broadcast_to(bns.astype(np.float64), (3, c - half)))


def test_se_oracle_is_the_se_block():
    import torch
    from oracle import seres18
    rng = np.random.default_rng(2)
    n, hw, c, mid = 3, 256, 64, 8
    y = rng.normal(size=(n, hw, c))
    st = np.stack([y.reshape(n, 2, 128, c).sum(2), (y * y).reshape(n, 2, 128, c).sum(2)], -1)
    w1, w2t = rng.normal(size=(mid, c)) / 8, rng.normal(size=(mid, c)) / 3
    g, _ = se_oracle(st, hw, w1, w2t)
    sd = {"p.fc1.weight": torch.from_numpy(w1.reshape(mid, c, 1, 1)), "p.fc2.weight": torch.from_numpy(w2t.T.copy())}
    ref = seres18._se(sd, "p", torch.from_numpy(y).reshape(n, 16, 16, c).permute(0, 3, 1, 2)).reshape(n, c).numpy()
    np.testing.assert_allclose(g, ref, rtol=1e-12, atol=1e-14)
    z = np.linspace(-100, 100, 401)
    np.testing.assert_allclose(1.0 / (1.0 + np.exp(-z)), torch.sigmoid(torch.from_numpy(z)).numpy(), rtol=1e-14, atol=1e-300)


def test_sampled_oracle_equals_dense_oracle():
    """The pixel-restricted oracles are the dense ones, bit for bit, on a sample with every structural part."""
    n = 9
    x, stats, gamma, beta, bns, bnh = norm_operands("l3", n, 3)
    hw, c = x.shape[1], x.shape[2]
    a, b = in_oracle(stats, hw, gamma, beta, bns, bnh)
    pix = sample_pix(n, hw, 4, dense_below=0)
    assert len(pix) < n * hw and pix[0] == 0 and pix[-1] == n * hw - 1
    dense, dbound = applied(x, a, b, np.arange(n * hw))
    v, bd = applied(x, a, b, pix)
    np.testing.assert_array_equal(v, dense[pix])
    np.testing.assert_array_equal(bd, dbound[pix])
    g, dg = se_oracle(stats, hw, np.ones((4, c), np.float32) / c, np.ones((4, c), np.float32))
    dense, dbound = se_out(x, x, g, dg, np.arange(n * hw))
    v, bd = se_out(x, x, g, dg, pix)
    np.testing.assert_array_equal(v, dense[pix])
    np.testing.assert_array_equal(bd, dbound[pix])


def test_gem_oracle_is_gem():
    import torch
    rng = np.random.default_rng(5)
    x = rng.uniform(-0.5, 3, (2, 17, 64))
    for p in (3.0, 6.5):
        g, _, _, _ = gem_oracle(x, p, np.ones(64, np.float32), np.zeros(64, np.float32))
        t = torch.from_numpy(x).clamp(min=float(np.float32(1e-6))).pow(p).mean(1).pow(1.0 / p).numpy()
        np.testing.assert_allclose(g, t, rtol=1e-12)


# ----------------------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def eng():
    from reid_amd import synth, weights
    from reid_amd.engine import get_engine
    e = get_engine(0)
    blob, manifest, _ = weights.pack_seres18(synth.seres18_state_dict(0))   # a loaded checkpoint: precision 2's split convolutions
    e.load_seres18(blob, manifest)
    yield e
    e.clear_fault()


# ----------------------------------------------------------------------------- IN finish from given stats
FINISH_CASES = [("syn", 5), ("l1", 2), ("l2", 3), ("l3", 127), ("l3", 128), ("l3", 255), ("l3", 256), ("l3", 511), ("l3", 512),
                ("l1", 16), ("l1", 17), ("l1", 31), ("l1", 32), ("syn128", 1023), ("syn128", 1024)]


def finish_forms(layer, n):
    """Which forms a case runs: the packed forms at the in_apply_pack rows rule (l3), the f16 forms at the tail_slices rule, all at the
    small shapes."""
    if layer == "l3" and n > 100:
        return (NF_IN_APPLY, NF_PACK, NF_PACK_IN)
    if layer == "l1" and n >= 16 or layer == "syn128":
        return (NF_F16, NF_F16_AFFINE)
    return tuple(range(6))


@gpu
@pytest.mark.parametrize("layer,n", FINISH_CASES, ids=["%s-n%d" % c for c in FINISH_CASES])
def test_in_finish(eng, layer, n):
    hw, c, half, _ = LAYERS[layer]
    forms = finish_forms(layer, n)
    x, stats, gamma, beta, bns, bnh = norm_operands(layer, n, 100 + n, f16=NF_F16 in forms)   # f16 values: exact in both forms
    a, b = in_oracle(stats, hw, gamma, beta, bns, bnh)
    pix = sample_pix(n, hw, n)
    what = "%s n=%d" % (layer, n)
    if NF_FINALIZE in forms:
        _, _, ga, gb = eng.debug_norm_finish(NF_FINALIZE, None, stats, gamma, beta, bns, bnh, hw=hw)
        check(ga, a, ulp32(a), what + " norm_finalize a")
        check(gb, b, ulp32(b), what + " norm_finalize b")
    v32 = None
    if NF_IN_APPLY in forms:
        out = eng.debug_norm_finish(NF_IN_APPLY, x, stats, gamma, beta)[0]
        v, bd = applied(x[..., :half], a[:, :half], b[:, :half], pix)
        check(out[..., :half].reshape(-1, half)[pix], v, bd, what + " in_apply")
        np.testing.assert_array_equal(out[..., half:], x[..., half:], err_msg=what + " in_apply: BatchNorm half")
        v32 = out
    for form in (NF_PACK, NF_PACK_IN):
        if form not in forms:
            continue
        out, pk, _, _ = eng.debug_norm_finish(form, x, stats, gamma, beta)
        name = "%s in_apply_pack in_only=%d" % (what, form == NF_PACK_IN)
        np.testing.assert_array_equal(out, x, err_msg=name + ": its fp32 input")
        hi, lo = split16(v32[..., :half].reshape(-1, half))
        np.testing.assert_array_equal(pk[:, :half], hi, err_msg=name + ": xh")
        np.testing.assert_array_equal(pk[:, c:c + half], lo, err_msg=name + ": xl'")
        if form == NF_PACK:
            hi, lo = split16(x[..., half:].reshape(-1, c - half))
            np.testing.assert_array_equal(pk[:, half:c], hi, err_msg=name + ": BatchNorm half xh")
            np.testing.assert_array_equal(pk[:, c + half:], lo, err_msg=name + ": BatchNorm half xl'")
        else:
            assert (pk[:, half:c] == 0xffff).all() and (pk[:, c + half:] == 0xffff).all(), name + ": BatchNorm half written"
        v, bd = applied(x[..., :half], a[:, :half], b[:, :half], pix)
        recon = from16(pk[pix, :half]) + from16(pk[pix, c:c + half]) / 2048.0
        check(recon, v, bd + 2.0 ** -21 * v + 2.0 ** -35, name + ": xh + xl' 2^-11")
    xb = f16_bits(x)
    for form in (NF_F16, NF_F16_AFFINE):
        if form not in forms:
            continue
        for tiles_one in ((False, True) if layer in ("l1", "syn128") else (False,)):
            st = per_image_stats(stats) if tiles_one else stats
            aa, bb = in_oracle(st, hw, gamma, beta, bns, bnh)
            out, o16, ga, gb = eng.debug_norm_finish(form, xb, st, gamma, beta, bns, bnh)
            name = "%s %s tiles=%s" % (what, "norm_apply_f16" if form == NF_F16 else "norm_finalize + affine_relu_f16",
                                       1 if tiles_one else st.shape[1])
            assert (o16 != 0xffff).all(), name + ": unwritten"
            v, bd = applied(x, aa, bb, pix, f16=True)
            check(from16(o16.reshape(-1, c)[pix]), v, bd, name)
            if form == NF_F16_AFFINE:
                check(ga, aa, ulp32(aa), name + " a")
                check(gb, bb, ulp32(bb), name + " b")


# ----------------------------------------------------------------------------- IN finish chained to the convolution
RATIOS = (0.0, 3.0, 30.0)
CHAIN_CASES = [(layer, prec, r) for layer, n in (("l3", 4), ("l2", 3)) for prec in (0, 2) for r in RATIOS]


def _chain_offset(x, wt, target):
    """The centre-tap weight offset (always inside the image: no padding edge in the channel mean) that gives a median per-channel
    mean/std of about `target` for the float64 convolution."""
    import test_gpu_conv as tc
    if target == 0:
        return 0.0
    n, h, w, cin = x.shape
    cout = wt.shape[0]
    acc, _ = tc.conv_oracle(x, wt, 1, 1, np.arange(n * h * w))
    v0 = acc.reshape(n, h * w, cout)
    s = x.astype(np.float64).sum(-1).reshape(n, h * w, 1)      # what the offset multiplies: the centre tap's channel sum

    def ratio(off):
        v = v0 + off * s
        return np.median(np.abs(v.mean(1)) / v.std(1))
    lo, hi = 0.0, 1.0
    while ratio(hi) < target:
        hi *= 2
    for _ in range(30):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if ratio(mid) < target else (lo, mid)
    return 0.5 * (lo + hi)


@gpu
@pytest.mark.parametrize("layer,prec,ratio", CHAIN_CASES, ids=["%s-p%d-r%g" % c for c in CHAIN_CASES])
def test_in_finish_chained(eng, layer, prec, ratio):
    """IBN conv1 as the forward calls it in precisions 0 and 2 (BatchNorm + ReLU from C/2 on, stats), then the finish that precision
    uses (in_apply / in_apply_pack), against float64 InstanceNorm of the float64 convolution."""
    import torch
    import test_gpu_conv as tc
    n = dict(l3=4, l2=3)[layer]
    h, w, cin, cout, r, stride, pad = tc.LAYERS[layer]
    hw, half = h * w, cout // 2
    rng = np.random.default_rng(int(ratio) * 10 + prec)
    x = rng.uniform(1.0, 2.0, (n, h, w, cin)).astype(np.float32)        # non-negative, as the trunk feeds
    wt = (rng.normal(size=(cout, r, r, cin)) / np.sqrt(r * r * cin))
    wt[:, 1, 1, :] += _chain_offset(x, wt.astype(np.float32), ratio)
    wt = wt.astype(np.float32)
    sc = np.ones(cout, np.float32)
    sh = np.zeros(cout, np.float32)
    sc[half:] = rng.uniform(0.5, 1.5, cout - half)
    sh[half:] = rng.normal(size=cout - half)
    gamma = rng.uniform(0.5, 1.5, half).astype(np.float32)
    beta = rng.normal(size=half).astype(np.float32)
    eng.set_precision(prec)
    try:
        v32, _, st = eng.debug_conv_layer(x, wt, stride, pad, sc, sh, relu=True, relu_from=half, stats=True)
    finally:
        eng.set_precision(0)
    v32 = v32.reshape(n, hw, cout)
    st = st.reshape(n, hw // 128, cout, 2)
    if prec == 0:
        got = eng.debug_norm_finish(NF_IN_APPLY, v32, st, gamma, beta)[0][..., :half]
    else:
        pk = eng.debug_norm_finish(NF_PACK, v32, st, gamma, beta)[1]
        got = (from16(pk[:, :half]) + from16(pk[:, cout:cout + half]) / 2048.0).reshape(n, hw, half)
    # float64 oracle and the propagated bound
    rows = np.arange(n * hw)
    acc, ab = tc.conv_oracle(x, wt, stride, pad, rows)
    bv = tc.bound(acc, ab, wt, r * r * cin, prec == 2)[:, :half].reshape(n, hw, half)
    v = acc[:, :half].reshape(n, hw, half)
    mean, var = v.mean(1), v.var(1)
    inv = 1.0 / np.sqrt(var + EPS)
    want = np.maximum(gamma * (v - mean[:, None]) * inv[:, None] + beta, 0.0)
    d_mean = (bv.sum(1) + SAFETY * 128 * U * np.abs(v).sum(1)) / hw
    ev2 = (v * v).mean(1)
    d_var = ((2 * np.abs(v) * bv + bv * bv).sum(1) + SAFETY * 129 * U * (v * v).sum(1)) / hw + 2 * np.abs(mean) * d_mean + d_mean ** 2
    CANCEL = 0.5 * SAFETY * 129 * U * ev2 / (var + EPS)
    rel_inv = CANCEL + (d_var - SAFETY * 129 * U * ev2) / (2 * (var + EPS))
    a, b = gamma * inv, beta - mean * gamma * inv
    bound = (np.abs(gamma) * inv)[:, None] * (bv + d_mean[:, None]) + np.abs(gamma * (v - mean[:, None]) * inv[:, None]) * rel_inv[:, None] \
        + SAFETY * (2 * U * (np.abs(v * a[:, None]) + np.abs(b)[:, None]) + ulp32(a)[:, None] * np.abs(v) + ulp32(b)[:, None])
    if prec == 2:
        bound = bound + 2.0 ** -21 * want + 2.0 ** -35
    worst = check(got, want, bound, "%s p%d mean/std %g" % (layer, prec, ratio))
    # recorded: torch's CPU fp32 instance_norm on the same fp32 convolution output
    t = torch.nn.functional.instance_norm(torch.from_numpy(v32[..., :half]).permute(0, 2, 1), None, None, torch.from_numpy(gamma),
                                          torch.from_numpy(beta), True, 0.0, EPS).permute(0, 2, 1).numpy()
    t = np.maximum(t.astype(np.float64), 0.0)
    print("\nCHAINED %s p%d mean/std %.3g (median %.3g): device max err %.3e, err/bound %.3f, CANCEL max %.2e; torch fp32 max err %.3e"
          % (layer, prec, ratio, np.median(np.abs(mean) / np.sqrt(var)), np.abs(got - want).max(), worst, CANCEL.max(),
             np.abs(t - want).max()))


# ----------------------------------------------------------------------------- SE gate + combine
def se_operands(layer, n, seed, mid=None, f16=False, saturate=False):
    hw, c, _, mid0 = LAYERS[layer]
    mid = mid or mid0
    rng = np.random.default_rng(seed)
    tiles = hw // 128
    stats = np.stack([rng.normal(size=(n, tiles, c)) * 128, rng.uniform(1, 2, (n, tiles, c)) * 128], -1).astype(np.float32)
    w1 = (rng.normal(size=(mid, c)) / np.sqrt(c) * 2).astype(np.float32)
    w2t = (rng.normal(size=(mid, c)) / np.sqrt(mid) * 2).astype(np.float32)
    if saturate:    # channels 0..7 with pre-sigmoid values near +-100
        pooled = stats[..., 0].astype(np.float64).sum(1) / hw
        hsum = np.maximum(pooled @ w1.T.astype(np.float64), 0).sum(1).mean()
        w2t[:, 0:4] = 100.0 / hsum
        w2t[:, 4:8] = -100.0 / hsum
    y = rng.normal(size=(n, hw, c)).astype(np.float32)
    sc = rng.normal(size=(n, hw, c)).astype(np.float32)
    if f16:
        y, sc = y.astype(np.float16).astype(np.float32), sc.astype(np.float16).astype(np.float32)
    return stats, w1, w2t, y, sc


SE_CASES = [("l4", 1, 32, False), ("l4", 64, 32, False), ("l4", 65, 32, False), ("l4", 3, 33, False), ("l4", 2, 32, True),
            ("l1", 2, 8, False), ("l1", 16, 8, False), ("l1", 17, 8, False), ("l2", 3, 8, False), ("l3", 5, 16, False),
            ("syn128", 1023, 8, False), ("syn128", 1024, 8, False)]


@gpu
@pytest.mark.parametrize("layer,n,mid,sat", SE_CASES, ids=["%s-n%d-m%d%s" % (c[0], c[1], c[2], "-sat" if c[3] else "") for c in SE_CASES])
def test_se_tail(eng, layer, n, mid, sat):
    hw, c, _, _ = LAYERS[layer]
    stats, w1, w2t, y, sc = se_operands(layer, n, 200 + n, mid, f16=True, saturate=sat)
    g, dg = se_oracle(stats, hw, w1, w2t)
    pix = sample_pix(n, hw, n)
    what = "%s n=%d mid=%d" % (layer, n, mid)
    v, bd = se_out(y, sc, g, dg, pix)
    # se_finalize + se_combine: the gate itself, then the output
    out, _, gate = eng.debug_se_tail(SE_COMBINE, stats, w1, w2t, y, sc)
    assert np.isfinite(out).all(), what + ": se_combine left output unwritten"
    check(gate, g, dg, what + " se_finalize gate")
    check(out.reshape(-1, c)[pix], v, bd, what + " se_combine")
    # launch_se_tail: the rule's kernel, bit for bit with the forced one; the other kernel too where it is legal
    small = se_small(n, hw, c, mid)
    rule_out, _, _ = eng.debug_se_tail(SE_RULE, stats, w1, w2t, y, sc)
    assert np.isfinite(rule_out).all(), what + ": se_tail left fp32 output unwritten"
    check(rule_out.reshape(-1, c)[pix], v, bd, what + " se_tail")
    forced = eng.debug_se_tail(SE_SMALL if small else SE_GENERAL, stats, w1, w2t, y, sc)[0]
    np.testing.assert_array_equal(rule_out, forced, err_msg=what + ": the rule's launch vs the forced kernel")
    if mid <= 32:
        other = eng.debug_se_tail(SE_GENERAL if small else SE_SMALL, stats, w1, w2t, y, sc)[0]
        np.testing.assert_array_equal(other, rule_out, err_msg=what + ": se_tail_kernel<true> vs <false>")
    else:
        with pytest.raises(_ffi.ReidHipError) as ei:
            eng.debug_se_tail(SE_SMALL, stats, w1, w2t, y, sc)
        assert ei.value.status == -1
    # packed: bit for bit the split of the fp32 output; the packed-only launch writes the same
    for base in ((SE_RULE, SE_SMALL, SE_GENERAL) if mid <= 32 else (SE_RULE, SE_GENERAL)):
        both_out, both_pk, _ = eng.debug_se_tail(base + 2, stats, w1, w2t, y, sc)
        np.testing.assert_array_equal(both_out, rule_out, err_msg=what + ": fp32 out with the packed store (form %d)" % base)
        hi, lo = split16(rule_out.reshape(-1, c))
        np.testing.assert_array_equal(both_pk[:, :c], hi, err_msg=what + ": oh (form %d)" % base)
        np.testing.assert_array_equal(both_pk[:, c:], lo, err_msg=what + ": ol' (form %d)" % base)
        only_out, only_pk, _ = eng.debug_se_tail(base + 1, stats, w1, w2t, y, sc)
        assert only_out is None
        np.testing.assert_array_equal(only_pk, both_pk, err_msg=what + ": packed-only launch (form %d)" % base)
    # precision 1: se_tail_f16 and se_finalize + se_combine_f16
    yb, sb = f16_bits(y), f16_bits(sc)
    v16, bd16 = se_out(y, sc, g, dg, pix, f16=True)
    for form, name in ((SE_F16, "se_tail_f16"), (SE_F16_COMBINE, "se_finalize + se_combine_f16")):
        _, o16, gate = eng.debug_se_tail(form, stats, w1, w2t, yb, sb)
        assert (o16 != 0xffff).all(), "%s %s: unwritten" % (what, name)
        check(from16(o16.reshape(-1, c)[pix]), v16, bd16, "%s %s" % (what, name))
        if gate is not None:
            check(gate, g, dg, "%s %s gate" % (what, name))


# ----------------------------------------------------------------------------- GeM + BNNeck
GEM_CASES = [(f16, hw, p) for f16 in (False, True) for hw, p in ((128, 3.0), (128, float(np.nextafter(np.float32(3), np.float32(4)))),
                                                                  (128, 1.0), (128, 6.5), (1, 3.0), (17, 6.5), (200, 3.0), (200, 1.0))]


@gpu
@pytest.mark.parametrize("f16,hw,p", GEM_CASES, ids=["%s-hw%d-p%.8g" % ("f16" if c[0] else "f32", c[1], c[2]) for c in GEM_CASES])
def test_gem_neck(eng, f16, hw, p):
    n, c = 3, 512
    rng = np.random.default_rng(hw + int(p * 10))
    x = rng.uniform(0, 3, (n, hw, c)).astype(np.float32)
    x[:, :, :16] = 0.0                   # the clamp: zeros and negatives -> 1e-6
    x[:, :, 16:32] = -rng.uniform(0, 2, (n, hw, 16))
    x[:, :, 32:40] = rng.uniform(0, 1e-7, (n, hw, 8))
    if f16:
        x = x.astype(np.float16).astype(np.float32)
    scale = rng.uniform(-2, 2, c).astype(np.float32)
    shift = rng.normal(size=c).astype(np.float32)
    g, e = eng.debug_gem_neck(f16_bits(x) if f16 else x, p, scale, shift, f16=f16)
    assert eng.fault_bits() == 0
    go, eo, bg, be = gem_oracle(x, p, scale, shift, f16)
    what = "%s hw=%d p=%r" % ("f16" if f16 else "fp32", hw, p)
    check(g, go, bg, what + " gem")
    check(e, eo, be, what + " emb")


@gpu
def test_trans_accuracy(eng):
    """Measures exp2(log2 x) as the fp32 GeM kernel forms it (p = 1, one pixel: m = the term, g = powf(m, 1) = m) over x in
    [1e-6, 1e3]; the result is recorded in the module docstring and must lie inside the chosen E_LOG / E_EXP model."""
    n, c = 64, 512
    x = np.exp(np.random.default_rng(7).uniform(np.log(1e-6), np.log(1e3), (n, 1, c))).astype(np.float32)
    g, _ = eng.debug_gem_neck(x, 1.0, np.ones(c, np.float32), np.zeros(c, np.float32))
    xd = x[:, 0].astype(np.float64)
    rel = np.abs(g / xd - 1.0)
    model = E_EXP + np.log(2) * (E_LOG * np.maximum(np.abs(np.log2(xd)), 1.0) + U * np.abs(np.log2(xd)))
    print("\nTRANS exp2(log2 x): max relative error %.3e (%.2f u), max error/model %.3f" % (rel.max(), rel.max() / U, (rel / model).max()))
    assert (rel <= model).all()


@gpu
@pytest.mark.parametrize("f16", [False, True])
def test_gem_neck_nonfinite_embedding_faults(eng, f16):
    n, hw, c = 2, 128, 512
    x = np.ones((n, hw, c), np.float32)
    scale, shift = np.ones(c, np.float32), np.zeros(c, np.float32)
    eng.debug_gem_neck(f16_bits(x) if f16 else x, 3.0, scale, shift, f16=f16)
    assert eng.fault_bits() == 0
    x[1, 5, 77] = np.inf
    with pytest.raises(_ffi.ReidHipError) as ei:
        eng.debug_gem_neck(f16_bits(x) if f16 else x, 3.0, scale, shift, f16=f16)
    assert ei.value.status == -3 and eng.fault_bits() == 2
    x[1, 5, 77] = 1.0
    with pytest.raises(_ffi.ReidHipError):       # sticky
        eng.debug_gem_neck(x, 3.0, scale, shift)
    eng.clear_fault()
    assert eng.fault_bits() == 0
    g, _ = eng.debug_gem_neck(f16_bits(x) if f16 else x, 3.0, scale, shift, f16=f16)
    np.testing.assert_allclose(g, 1.0, rtol=1e-6)


# ----------------------------------------------------------------------------- range fault of the packed writers
BELOW = float(np.frombuffer(np.uint32(0x477fdfff).tobytes(), np.float32)[0])    # 65503.996
RANGE_CASES = [(BELOW, False), (65504.0, True), (-70000.0, True), (float("nan"), True)]


def _expect(eng, call, fault):
    if not fault:
        call()
        assert eng.fault_bits() == 0
        return
    with pytest.raises(_ffi.ReidHipError) as ei:
        call()
    assert ei.value.status == -3 and eng.fault_bits() == 1
    with pytest.raises(_ffi.ReidHipError):          # the word stays set until cleared
        call()
    eng.clear_fault()
    assert eng.fault_bits() == 0


@gpu
@pytest.mark.parametrize("val,fault", RANGE_CASES, ids=["%r" % c[0] for c in RANGE_CASES])
def test_range_fault_in_apply_pack(eng, val, fault):
    """The BatchNorm half passes through in_apply_pack unchanged (in_only = 0 packs it, in_only = 1 does not read it); an InstanceNorm
    channel with a ~ 1, b = 0 carries -70000 (which the ReLU zeroes) and NaN."""
    n = 2
    x, stats, gamma, beta, _, _ = norm_operands("l3", n, 300)
    hw, c, half, _ = LAYERS["l3"]
    x[0, 3, half + 9] = val
    _expect(eng, lambda: eng.debug_norm_finish(NF_PACK, x, stats, gamma, beta), fault)
    eng.debug_norm_finish(NF_PACK_IN, x, stats, gamma, beta)
    assert eng.fault_bits() == 0
    if val < 0 or val != val:
        x[0, 3, half + 9] = 0.5
        ch = 40
        stats[:, :, ch, 0] = 0.0
        stats[:, :, ch, 1] = np.float32(hw)      # mean 0, var 1
        gamma[ch], beta[ch] = 1.0, 0.0
        x[1, 77, ch] = val
        for form in (NF_PACK, NF_PACK_IN):
            _expect(eng, lambda: eng.debug_norm_finish(form, x, stats, gamma, beta), fault)


@gpu
@pytest.mark.parametrize("val,fault", RANGE_CASES, ids=["%r" % c[0] for c in RANGE_CASES])
def test_range_fault_se_tail(eng, val, fault):
    n = 2
    stats, w1, w2t, y, sc = se_operands("l4", n, 400)
    y[0, 100, 300], sc[0, 100, 300] = 0.0, val       # o = g 0 + sc = sc before the ReLU
    for form in (SE_RULE + 1, SE_RULE + 2, SE_GENERAL + 1, SE_SMALL + 2):
        _expect(eng, lambda: eng.debug_se_tail(form, stats, w1, w2t, y, sc), fault)
    eng.debug_se_tail(SE_RULE, stats, w1, w2t, y, sc)     # no packed store: no range guard
    assert eng.fault_bits() == 0
