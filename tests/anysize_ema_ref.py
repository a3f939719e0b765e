"""Float64 oracle of the EMA block tail of EMARes18-IBN for any map size (csrc/anysize_ema.h), its case table, the operand families, an
fp32 emulation of the kernels' documented order, and the per-element error bound of that order.

    out = relu(y * sigmoid(wt[h, w]) + shortcut)                     y, shortcut, out NHWC [n][H][W][C], 32 groups of cg = C / 32
    sig_h = sigmoid(conv1x1(mean over w of y)),  sig_w = sigmoid(conv1x1(mean over h of y))          consecutive channels
    p  = y sig_h sig_w ("x1pre"),  x1 = (p - mu) rstd gw + gb,  mu = mean(p), rstd = 1 / sqrt(var(p) + 1e-5) (biased) over the map
    x2 = conv3x3_pad1(y) + b3,  s1 = softmax_k(mean x1),  s2 = softmax_k(mean x2),  wt = sum_k s1[k] x2[k] + s2[k] x1[k]
    prm = conv1x1 w [cg][cg], b [cg] | conv3x3 w [cg][cg][3][3], b [cg] | GroupNorm weight [cg], bias [cg].

The kernels take s1 = softmax(gb): the mean of a GroupNorm output over the extent it was normalised on is the GroupNorm bias.  The oracle
computes mean(x1) the long way, so the identity is inside the bound (term "s1" below) and not assumed by it.

The bound, with u = 2^-24 (fp32 unit roundoff), v = 2^-53 (fp64), gamma(k) = k u / (1 - k u) for k fp32 roundings in a row, term by term in
the kernels' order (csrc/anysize_ema.h); "d" is an absolute error bound, every quantity on the right is the oracle's own:

  mean   a line of L values summed in fp64, divided, rounded once:       dm  <= L v mean|y| + u |m|
  1x1    cg fused multiply-adds on the bias:                              da  <= gamma(cg) (|b1| + sum|w1 m|) + sum|w1| dm
  sig    s = 1 / (1 + expf(-a)).  The sigmoid's slope is s (1 - s) <= 1/4 and half its second derivative at most 0.05; expf is within
         1 ulp (2 u relative) on e = exp(-a), which reaches s with the factor (1 - s); 1 + e rounds once and the division is within 2.5
         ulp whatever the compiler's division mode:                      ds  <= s (1 - s) da + 0.05 da^2 + 8 u s + 2^-126
         (the last term: a result below the normal range may be flushed).
  p      two products, each rounded:                                     dp  <= |y| (sig_w dsig_h + sig_h dsig_w) + 2 u |p|
  mu     the kernel averages ITS p (fp64 sum, one rounding):              dmu <= mean(dp) + hw v mean|p| + u |mu|
  rstd   the standard deviation is 1-Lipschitz in the root-mean-square norm, so |std(p') - std(p)| <= rms(dp), and
         S2 / hw = var + mu^2 carries the fp64 cancellation term:          dvar <= 2 std rms(dp) + rms(dp)^2 + (3 hw + 4) v (var + mu^2)
         rstd = (var + eps)^(-1/2) has slope rstd^3 / 2; one rounding:     dr  <= rstd^3 / 2 dvar + u rstd
         eps keeps this finite at var = 0 (the per-channel-constant family).
  x1     fmaf(((p - mu) * rstd), gw, gb) - the GroupNorm amplification rstd |gw| stands in front of every input error:
                                       de  = dp + dmu + u |p - mu|
                                       dt  = rstd de + |p - mu| dr + u |p - mu| rstd
                                       dx1 <= |gw| dt + u |x1|
  x2     9 cg fused multiply-adds on the bias, y exact:                    dx2 <= gamma(9 cg) (|b3| + sum|w3 y|)
  s2     a2 = mean(x2) (fp64 sum of the kernel's x2, one rounding):        da2 <= mean(dx2) + hw v mean|x2| + u |a2|
         softmax: d s_k / d a_j = s_k (delta_kj - s_j), so to first order ds_k <= s_k (da_k + sum_j s_j da_j); with D = max_j da_j the
         exact ratio is inside exp(+-2 D), which adds at most s_k (2 D)^2; the evaluation subtracts the maximum (rounding u |a - max|
         on numerator and denominator), takes expf (2 u), sums cg terms (cg u) and divides (5 u):
                                       ds2 <= s_k (da_k + sum_j s_j da_j + (2 D)^2) + s_k (2 range(a) + cg + 9) u + 2^-126
  s1     the same with da1 = |mean(x1) - gb| as the oracle itself finds it (its own rounding of the identity; nothing is measured on
         the device) - so a kernel that took another vector here would leave the bound.
  wt     2 cg fused multiply-adds and at most two additions across lanes:
                                       dwt <= gamma(2 cg + 2) sum(|s1 x2| + |s2 x1|) + sum(s1 dx2 + |x2| ds1 + s2 dx1 + |x1| ds2)
  gate   g = sigmoid(wt):                                                  dg  <= g (1 - g) dwt + 0.05 dwt^2 + 8 u g + 2^-126
  out    y * g rounds once, the sum with the shortcut once, relu does not expand an error:
                                       dout <= |y| dg + u |y g| + u |y g + shortcut|
Second-order products of these terms are covered by the factor 1.01 on every returned bound.

bounds(old=True) is the same derivation for ema_tail_kernel of csrc/attention_f32.hip, the slab-in-LDS kernel of the 256 x 128 forward
(tests/test_gpu_anysize_ema.py compares the two where the old one fits): a line is summed in fp32 one value after the other (L v becomes
gamma(L)); a sum over the map is 64 lanes of hw / 64 values each and a six-step tree (hw v becomes gamma(hw / 64 + 7)); the variance is the
mean of (p - mu)^2 around the rounded mean, so its fp32 term is gamma(hw / 64 + 9) var + dmu^2 and nothing cancels; multiply-adds are not
fused (two roundings each: gamma(2 cg), gamma(18 cg), gamma(4 cg + 1)); x1 takes four roundings; and agp(x1) is measured, so s1 carries
da1 = mean(dx1) + gamma(hw / 64 + 7) mean|x1| + u |a1|."""
import numpy as np

U = 2.0 ** -24
V = 2.0 ** -53
TINY = 2.0 ** -126
GROUPS = 32
EPS = 1e-5
# (H, W, C): the 3 x 3 window larger than the map with cg = 16; ...; odd W with a row longer than a wave; one-line maps both ways; the map
# the slab-in-LDS kernel cannot hold (n = 1 only)
CASES = ((2, 2, 512), (4, 2, 512), (6, 5, 256), (24, 18, 64), (56, 67, 64), (2, 128, 128), (128, 2, 128), (128, 128, 64))
BATCHES = {case: ((1,) if case == (128, 128, 64) else (1, 3)) for case in CASES}
FAMILIES = ("normal", "const", "saturate", "pixel")
MUTATIONS = ("var_unbiased", "eps6", "softmax_swapped", "swap_pools", "clamp_pad", "no_b1", "w3_transposed", "one_sigmoid", "no_affine",
             "interleaved", "shortcut_first")
NAMES = ("out", "sig", "mu", "rstd", "s1", "s2")


def prm_size(cg):
    return cg * cg * 10 + 4 * cg


def make_prm(c, seed):
    """The block's parameters as the loader packs them (Se18Block::ema), none of them trivial: a mutation that drops one shows."""
    cg = c // GROUPS
    rng = np.random.default_rng(2000 + seed)
    parts = (rng.normal(0.0, 1.0 / np.sqrt(cg), cg * cg), rng.normal(0.0, 0.3, cg), rng.normal(0.0, np.sqrt(2.0 / (9 * cg)), cg * cg * 9),
             rng.normal(0.0, 0.2, cg), rng.uniform(0.5, 1.5, cg), rng.normal(0.0, 0.3, cg))
    return np.concatenate(parts).astype(np.float32)


def unpack_prm(prm, cg):
    prm = np.asarray(prm).reshape(-1)
    assert prm.size == prm_size(cg)
    o = np.cumsum([0, cg * cg, cg, cg * cg * 9, cg, cg, cg])
    w1, b1, w3, b3, gw, gb = (prm[o[i]:o[i + 1]] for i in range(6))
    return w1.reshape(cg, cg), b1, w3.reshape(cg, cg, 3, 3), b3, gw, gb


def operands(case, n, family, seed=0):
    """y, shortcut [n][H][W][C] float32.  normal: what a folded BatchNorm leaves; const: one value per (image, channel) - the GroupNorm
    variance is 0 and x1 is the GroupNorm bias; saturate: magnitudes that drive the three sigmoids to 0 and 1; pixel: all zeros but ONE
    pixel per channel group - a corner, an edge or the interior by (image + group) mod 3 - which shows the border taps of the 3 x 3
    convolution and a variance far below eps.  An image's values depend on its index alone, not on n."""
    h, w, c = case
    cg = c // GROUPS
    ys, scs = [], []
    for i in range(n):
        rng = np.random.default_rng((seed * 7919 + h * 131 + w * 17 + c) * 10 + FAMILIES.index(family) + 1000003 * i)
        if family == "normal":
            y = rng.normal(0.0, 1.0, (h, w, c)) * rng.uniform(0.5, 2.0, (1, 1, c)) + rng.normal(0.0, 0.3, (1, 1, c))
        elif family == "const":
            y = np.broadcast_to(rng.normal(0.2, 1.0, (1, 1, c)), (h, w, c))
        elif family == "saturate":
            y = rng.normal(0.0, 12.0, (h, w, c)) + rng.normal(0.0, 12.0, (1, 1, c))
        elif family == "pixel":
            y = np.zeros((h, w, c))
            spots = ((0, 0), (0, w // 2), (h // 2, w // 2))
            for g in range(GROUPS):
                ph, pw = spots[(i + g) % 3]
                y[ph, pw, g * cg:(g + 1) * cg] = rng.normal(0.0, 2.0, cg)
        else:
            raise ValueError(family)
        ys.append(y)
        scs.append(rng.normal(0.0, 1.0, (h, w, c)))
    return np.ascontiguousarray(np.stack(ys), np.float32), np.ascontiguousarray(np.stack(scs), np.float32)


# ---------------------------------------------------------------------------------------------- float64 oracle
def _sigmoid(a):
    return 1.0 / (1.0 + np.exp(-a))


def _softmax(a):
    e = np.exp(a - a.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def _conv3(gx, w3, b3, clamp=False):
    """gx [n][H][W][G][ci] -> (x2, sum of the terms' magnitudes) [n][H][W][G][co]; cross-correlation, pad 1."""
    n, h, w = gx.shape[:3]
    pad = np.pad(gx, ((0, 0), (1, 1), (1, 1), (0, 0), (0, 0)), mode="edge" if clamp else "constant")
    acc = np.zeros(gx.shape, np.float64) + b3
    mag = np.zeros(gx.shape, np.float64) + np.abs(b3)
    for r in range(3):
        for s in range(3):
            win = pad[:, r:r + h, s:s + w]
            acc = acc + np.einsum("nhwgi,oi->nhwgo", win, w3[:, :, r, s])
            mag = mag + np.einsum("nhwgi,oi->nhwgo", np.abs(win), np.abs(w3[:, :, r, s]))
    return acc, mag


def tail(y, sc, prm, full=False, **mut):
    """Float64 oracle.  Returns a dict: out [n][H][W][C], sig [n][H + W][C], mu, rstd, s1, s2 [n][C] in the kernels' layouts (with
    full=True also the per-pixel intermediates, grouped [n][H][W][32][cg]).  The keywords are the mutations of
    tests/test_anysize_ema_host.py (MUTATIONS), each a subtly wrong tail."""
    assert set(mut) <= set(MUTATIONS)
    m = lambda k: bool(mut.get(k))   # noqa: E731
    y64, sc64 = np.asarray(y, np.float64), np.asarray(sc, np.float64)
    n, h, w, c = y64.shape
    cg = c // GROUPS
    w1, b1, w3, b3, gw, gb = (a.astype(np.float64) for a in unpack_prm(prm, cg))
    if m("interleaved"):                                   # channel c in group c % 32
        group = lambda a: a.reshape(a.shape[:-1] + (cg, GROUPS)).swapaxes(-1, -2)                  # noqa: E731
        flat = lambda a: a.swapaxes(-1, -2).reshape(a.shape[:-2] + (c,))                           # noqa: E731
    else:
        group = lambda a: a.reshape(a.shape[:-1] + (GROUPS, cg))                                   # noqa: E731
        flat = lambda a: a.reshape(a.shape[:-2] + (c,))                                            # noqa: E731
    gx = group(y64)                                        # [n][H][W][G][cg]
    vec = np.concatenate([gx.mean(1), gx.mean(2)] if m("swap_pools") else [gx.mean(2), gx.mean(1)], 1)   # [n][H + W][G][cg]
    a = np.einsum("njgi,oi->njgo", vec, w1) + (0.0 if m("no_b1") else b1)
    sig = _sigmoid(a)
    sh, sw = sig[:, :h, None], sig[:, None, h:]
    p = gx * sh if m("one_sigmoid") else gx * sh * sw
    hw = h * w
    mu = p.mean((1, 2))
    var = ((p - mu[:, None, None]) ** 2).sum((1, 2)) / ((hw - 1) if m("var_unbiased") else hw)
    rstd = 1.0 / np.sqrt(var + (1e-6 if m("eps6") else EPS))
    x1 = (p - mu[:, None, None]) * rstd[:, None, None]
    if not m("no_affine"):
        x1 = x1 * gw + gb
    x2, _ = _conv3(gx, w3.transpose(1, 0, 2, 3) if m("w3_transposed") else w3, b3, m("clamp_pad"))
    a1, a2 = x1.mean((1, 2)), x2.mean((1, 2))
    s1, s2 = _softmax(a1), _softmax(a2)                    # [n][G][cg]
    if m("softmax_swapped"):
        wt = (s1[:, None, None] * x1 + s2[:, None, None] * x2).sum(-1, keepdims=True)
    else:
        wt = (s1[:, None, None] * x2 + s2[:, None, None] * x1).sum(-1, keepdims=True)
    g = _sigmoid(wt)
    if m("shortcut_first"):
        out = np.maximum(flat((gx + group(sc64)) * g), 0.0)
    else:
        out = np.maximum(flat(gx * g) + sc64, 0.0)
    res = {"out": out, "sig": flat(sig), "mu": flat(mu), "rstd": flat(rstd), "s1": flat(s1), "s2": flat(s2)}
    if full:
        res.update(gx=gx, a=a, sigg=sig, p=p, mug=mu, var=var, rstdg=rstd, x1=x1, x2=x2, a1=a1, a2=a2, s1g=s1, s2g=s2, wt=wt, g=g)
    return res


# ---------------------------------------------------------------------------------------------- the bound
def _gamma(k):
    return k * U / (1.0 - k * U)


def _dsigmoid(s, da):
    return s * (1.0 - s) * da + 0.05 * da * da + 8 * U * s + TINY


def _dsoftmax(s, a, da, cg):
    big = da.max(-1, keepdims=True)
    rng = a.max(-1, keepdims=True) - a.min(-1, keepdims=True)
    return s * (da + (s * da).sum(-1, keepdims=True) + (2 * big) ** 2) + s * (2 * rng + cg + 9) * U + TINY


def bounds(y, sc, prm, old=False):
    """Per-element bounds, a dict with the keys and layouts of tail(): the kernels' documented order against the oracle (old=True: that of
    ema_tail_kernel, csrc/attention_f32.hip).  The derivation is the module's docstring."""
    y64, sc64 = np.asarray(y, np.float64), np.asarray(sc, np.float64)
    n, h, w, c = y64.shape
    cg, hw = c // GROUPS, h * w
    w1, b1, w3, b3, gw, gb = (a.astype(np.float64) for a in unpack_prm(prm, cg))
    t = tail(y, sc, prm, full=True)
    gx, ay = t["gx"], np.abs(t["gx"])
    flat = lambda a: a.reshape(a.shape[:-2] + (c,))        # noqa: E731
    # means, 1x1, sigmoids
    vec = np.concatenate([gx.mean(2), gx.mean(1)], 1)
    absvec = np.concatenate([ay.mean(2), ay.mean(1)], 1)
    ln = np.concatenate([np.full(h, float(w)), np.full(w, float(h))])[None, :, None, None]
    dm = (_gamma(ln) if old else ln * V) * absvec + U * np.abs(vec)
    da = _gamma(2 * cg if old else cg) * (np.abs(b1) + np.einsum("njgi,oi->njgo", np.abs(vec), np.abs(w1))) + np.einsum("njgi,oi->njgo", dm, np.abs(w1))
    sig = t["sigg"]
    dsig = _dsigmoid(sig, da)
    sh, sw, dsh, dsw = sig[:, :h, None], sig[:, None, h:], dsig[:, :h, None], dsig[:, None, h:]
    # p, mu, rstd, x1
    p, mu, var, rstd = t["p"], t["mug"], t["var"], t["rstdg"]
    dp = ay * (sw * dsh + sh * dsw) + 2 * U * np.abs(p)
    msum = _gamma(hw / 64.0 + 7) if old else hw * V        # a sum over the map
    dmu = dp.mean((1, 2)) + msum * np.abs(p).mean((1, 2)) + U * np.abs(mu)
    rms = np.sqrt((dp * dp).mean((1, 2)))
    dvar = 2 * np.sqrt(var) * rms + rms * rms + ((_gamma(hw / 64.0 + 9) * var + dmu * dmu) if old else (3 * hw + 4) * V * (var + mu * mu))
    dr = 0.5 * rstd ** 3 * dvar + U * rstd
    cen = np.abs(p - mu[:, None, None])
    de = dp + dmu[:, None, None] + U * cen
    dt = rstd[:, None, None] * de + cen * dr[:, None, None] + U * cen * rstd[:, None, None]
    x1, x2 = t["x1"], t["x2"]
    dx1 = np.abs(gw) * dt + U * np.abs(x1) + (U * np.abs(x1 - gb) if old else 0.0)
    # x2, softmaxes
    _, mag = _conv3(gx, w3, b3)
    dx2 = _gamma(18 * cg if old else 9 * cg) * mag
    da2 = dx2.mean((1, 2)) + msum * np.abs(x2).mean((1, 2)) + U * np.abs(t["a2"])
    s1, s2 = t["s1g"], t["s2g"]
    ds2 = _dsoftmax(s2, t["a2"], da2, cg)
    da1 = np.abs(t["a1"] - gb)
    if old:
        da1 = da1 + dx1.mean((1, 2)) + msum * np.abs(x1).mean((1, 2)) + U * np.abs(t["a1"])
    ds1 = _dsoftmax(s1, np.broadcast_to(gb, s1.shape), da1, cg)
    # weight, gate, out
    s1b, s2b, ds1b, ds2b = (a[:, None, None] for a in (s1, s2, ds1, ds2))
    dwt = _gamma(4 * cg + 1 if old else 2 * cg + 2) * (np.abs(s1b * x2) + np.abs(s2b * x1)).sum(-1, keepdims=True) + \
        (s1b * dx2 + np.abs(x2) * ds1b + s2b * dx1 + np.abs(x1) * ds2b).sum(-1, keepdims=True)
    g = t["g"]
    dg = _dsigmoid(g, dwt)
    yg = flat(gx * g)
    dout = flat(ay * dg) + U * np.abs(yg) + U * np.abs(yg + sc64)
    res = {"out": dout, "sig": flat(dsig), "mu": flat(dmu), "rstd": flat(dr), "s1": flat(ds1), "s2": flat(ds2)}
    return {k: 1.01 * v + 1e-44 for k, v in res.items()}


# ---------------------------------------------------------------------------------------------- fp32 emulation of the documented order
def _fma32(a, b, c):
    """fmaf on float32 arrays: the product is exact in float64, so one rounding to float64 and one to float32 remain."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(np.float32)


def _sigmoid32(a):
    one = np.float32(1.0)
    with np.errstate(over="ignore"):
        return (one / (one + np.exp(-a.astype(np.float32)))).astype(np.float32)


def _softmax32(a):
    a = a.astype(np.float32)
    e = np.exp(a - a.max(-1, keepdims=True)).astype(np.float32)
    den = np.zeros(a.shape[:-1] + (1,), np.float32)
    for k in range(a.shape[-1]):
        den = den + e[..., k:k + 1]
    return (e / den).astype(np.float32)


def emulate(y, sc, prm):
    """The kernels' arithmetic restated with numpy (csrc/anysize_ema.h): fp64 sums rounded once, cg fmaf for the 1x1 convolution, 9 cg
    fmaf in (quad of ci, tap, ci in the quad) order for the 3 x 3, float32 sigmoids and softmaxes, s1 = softmax(gb), p with both products
    rounded, x1 = fmaf((p - mu) * rstd, gw, gb), the weight by fmaf per channel and pairwise across a group's quads, the product and the
    sum of the output rounded on their own.  Returns a dict as tail() does, float32."""
    y32, sc32 = np.asarray(y, np.float32), np.asarray(sc, np.float32)
    n, h, w, c = y32.shape
    cg, hw = c // GROUPS, h * w
    w1, b1, w3, b3, gw, gb = (a.astype(np.float32) for a in unpack_prm(prm, cg))
    gx = y32.reshape(n, h, w, GROUPS, cg)
    g64 = gx.astype(np.float64)
    vec = np.concatenate([g64.sum(2) / w, g64.sum(1) / h], 1).astype(np.float32)          # [n][H + W][G][cg]
    acc = np.broadcast_to(b1, vec.shape).astype(np.float32)
    for ci in range(cg):
        acc = _fma32(w1[:, ci], vec[..., ci:ci + 1], acc)
    sig = _sigmoid32(acc)
    p = ((gx * sig[:, :h, None]).astype(np.float32) * sig[:, None, h:]).astype(np.float32)
    p64 = p.astype(np.float64)
    s1sum, s2sum = p64.sum((1, 2)), (p64 * p64).sum((1, 2))
    mean = s1sum / hw
    var = np.maximum((s2sum - s1sum * mean) / hw, 0.0)
    mu, rstd = mean.astype(np.float32), (1.0 / np.sqrt(var + EPS)).astype(np.float32)
    x1 = _fma32(((p - mu[:, None, None]).astype(np.float32) * rstd[:, None, None]).astype(np.float32), gw, gb)
    pad = np.pad(gx, ((0, 0), (1, 1), (1, 1), (0, 0), (0, 0)))
    x2 = np.broadcast_to(b3, gx.shape).astype(np.float32)
    for q0 in range(0, cg, 4):
        for tap in range(9):
            r, s = divmod(tap, 3)
            win = pad[:, r:r + h, s:s + w]
            for ci in range(q0, min(q0 + 4, cg)):
                x2 = _fma32(w3[:, ci, r, s], win[..., ci:ci + 1], x2)
    a2 = (x2.astype(np.float64).sum((1, 2)) / hw).astype(np.float32)
    s1 = np.broadcast_to(_softmax32(gb), a2.shape)
    s2 = _softmax32(a2)
    lanes = []
    for q0 in range(0, cg, 4 if cg >= 4 else 2):
        t = np.zeros(gx.shape[:-1], np.float32)
        for k in range(q0, min(q0 + 4, cg)):
            t = _fma32(s1[:, None, None, :, k], x2[..., k], t)
            t = _fma32(s2[:, None, None, :, k], x1[..., k], t)
        lanes.append(t)
    while len(lanes) > 1:
        lanes = [(lanes[i] + lanes[i + 1]).astype(np.float32) for i in range(0, len(lanes), 2)]
    g = _sigmoid32(lanes[0])[..., None]
    out = np.maximum(((gx * g).astype(np.float32).reshape(n, h, w, c) + sc32).astype(np.float32), np.float32(0.0))
    flat = lambda a: np.ascontiguousarray(a.reshape(a.shape[:-2] + (c,)), np.float32)     # noqa: E731
    return {"out": out, "sig": flat(sig), "mu": flat(mu), "rstd": flat(rstd), "s1": flat(s1), "s2": flat(s2)}
