"""Float64 oracle of the TripletAttention block tail of CARes18-IBN for any map size (csrc/anysize_ca.h), its case table, the operand
families, an fp32 emulation of the kernels' documented order, and the per-element error bound of that order.

    out = relu(1/3 * ((y s_hw[h, w] + y s_cw[c, w]) + y s_hc[h, c]) + shortcut)           y, shortcut, out NHWC [n][H][W][C]
    s_g = sigmoid(scale_g * conv7x7_pad3(ZPool_g) + shift_g),  ZPool channel 0 = unbiased std, channel 1 = mean,
    over C for the (H, W) plane of hw, over H for the (C, W) plane of cw, over W for the (H, C) plane of hc.
    prm [3 gates: cw, hc, hw][100] = conv weight [2][7][7], folded BN scale, shift.

The bound, with u = 2^-24 (fp32 unit roundoff), v = 2^-53 (fp64), L the length of a reduced line, term by term in the kernels' order:

  maps   s1 = sum x and s2 = sum x^2 in fp64 (every x^2 exact): |ds2| <= L v s2, and s1 mean = s1^2 / L <= s2 carries (2 L + 4) v, so
         d(s2 - s1 mean) <= (3 L + 4) v s2.  With s2 / (L - 1) = var + L / (L - 1) mean^2 this is the cancellation term
             dvar <= (3 L + 4) v var (1 + L / (L - 1) mean^2 / var),
         written without the division so that var = 0 (a constant line) keeps a finite bound.  std = sqrt(var):
             dstd <= min(dvar / std, sqrt(dvar)) + u std           (one rounding to fp32)
             dmean <= L v mean|x| + u |mean|                        (one rounding to fp32)
  conv   98 fused multiply-adds in fp32, one rounding each: |dacc| <= 98 u sum|w m| / (1 - 98 u) + sum|w| dm.
  affine a = fmaf(acc, scale, shift): da <= |scale| dacc + u |a|.
  gate   g = 1 / (1 + expf(-a)).  The sigmoid's slope is g (1 - g) <= 1/4 and its second derivative at most 0.0963, so the input error
         gives g (1 - g) da + 0.05 da^2.  expf is within 1 ulp (2 u relative) on e = exp(-a), which reaches g with the factor (1 - g); 1 + e
         rounds once (u) and the division is within 2.5 ulp whatever the compiler's division mode (5 u): dg <= ... + 8 u g.
  out    a_k = y g_k rounds once (u |a_k|) and carries |y| dg_k; (a + b) and (a + b) + d round once each; the constant float32(1/3) is
         within u of 1/3 and the product rounds once; t + shortcut rounds once; relu does not expand an error.
Second-order products of these terms are covered by the factor 1.01 on the total."""
import numpy as np

U = 2.0 ** -24
V = 2.0 ** -53
# (H, W, C): planes smaller than the 7 x 7 window; ...; odd sides with H != W != C, so a transposed plane shows; a VeRi layer-1 map
CASES = ((2, 3, 512), (7, 5, 256), (8, 9, 64), (13, 17, 128), (56, 67, 64))
FAMILIES = ("bn", "offset", "const")
GATE_ORDER = ("cw", "hc", "hw")          # prm's rows


def per_image(h, w, c):
    return h * w + c * w + h * c


def make_prm(seed):
    """Three gates as the loader packs them: conv weights of the module's init (std sqrt(2 / 49)), a folded BN(1)."""
    rng = np.random.default_rng(1000 + seed)
    prm = np.empty((3, 100), np.float32)
    prm[:, :98] = rng.normal(0.0, np.sqrt(2.0 / 49.0), (3, 98))
    prm[:, 98] = rng.uniform(0.6, 1.4, 3)
    prm[:, 99] = rng.normal(0.0, 0.3, 3)
    return prm


def operands(case, n, family, seed=0):
    """y, shortcut [n][H][W][C] float32.  bn: what a folded BatchNorm leaves; offset: mean 8, std 0.05 (the variance formula's cancellation
    term); const: every row of W pixels constant per channel, so the hc plane's std is exactly 0 in the oracle."""
    h, w, c = case
    rng = np.random.default_rng(seed * 7919 + h * 131 + w * 17 + c + {"bn": 0, "offset": 1, "const": 2}[family] * 100003)
    if family == "bn":
        y = rng.normal(0.0, 1.0, (n, h, w, c)) * rng.uniform(0.5, 2.0, (1, 1, 1, c)) + rng.normal(0.0, 0.3, (1, 1, 1, c))
    elif family == "offset":
        y = rng.normal(8.0, 0.05, (n, h, w, c))
    elif family == "const":
        y = np.broadcast_to(rng.normal(0.2, 1.0, (n, h, 1, c)), (n, h, w, c))
    else:
        raise ValueError(family)
    sc = rng.normal(0.0, 1.0, (n, h, w, c))
    return np.ascontiguousarray(y, np.float32), np.ascontiguousarray(sc, np.float32)


# ---------------------------------------------------------------------------------------------- float64 oracle
def _zpool(y, axis, biased=False):
    """(std, mean) over `axis` of y [n][H][W][C] float64."""
    return y.std(axis=axis, ddof=0 if biased else 1), y.mean(axis=axis)


def _planes(y, biased=False):
    """The three ZPool planes [n][2][P][Q] in float64: hw (H, W), cw (C, W), hc (H, C)."""
    s, m = _zpool(y, 3, biased)
    hw = np.stack([s, m], 1)
    s, m = _zpool(y, 1, biased)                                # [n][W][C] -> (C, W)
    cw = np.stack([s.transpose(0, 2, 1), m.transpose(0, 2, 1)], 1)
    s, m = _zpool(y, 2, biased)                                # [n][H][C]
    hc = np.stack([s, m], 1)
    return {"hw": hw, "cw": cw, "hc": hc}


def _conv7(plane, wts, replicate=False):
    """Cross-correlation of plane [n][2][P][Q] with wts [2][7][7], pad 3; returns (acc, sum |w m|)."""
    n, _, p, q = plane.shape
    pad = np.pad(plane, ((0, 0), (0, 0), (3, 3), (3, 3)), mode="edge" if replicate else "constant")
    acc = np.zeros((n, p, q), pad.dtype)
    mag = np.zeros((n, p, q), np.float64)
    for ch in range(2):
        for r in range(7):
            for t in range(7):
                term = wts[ch, r, t] * pad[:, ch, r:r + p, t:t + q]
                acc = acc + term
                mag += np.abs(term)
    return acc, mag


def pack_maps(planes):
    """-> [n][2 per] in the layout of csrc/anysize_ca.h: hw [2][H][W] | cw [2][C][W] | hc [2][H][C]."""
    n = planes["hw"].shape[0]
    return np.concatenate([planes[k].reshape(n, -1) for k in ("hw", "cw", "hc")], 1)


def pack_gates(g):
    """-> [n][per]: hw [H][W] | cw [W][C] (transposed) | hc [H][C]."""
    n = g["hw"].shape[0]
    return np.concatenate([g["hw"].reshape(n, -1), g["cw"].transpose(0, 2, 1).reshape(n, -1), g["hc"].reshape(n, -1)], 1)


def tail(y, sc, prm, biased=False, swap_channels=False, swap_cw_hc=False, transposed_plane=False, replicate=False, third_on_two=False,
         shortcut_first=False):
    """Float64 oracle.  Returns (out [n][H][W][C], maps [n][2 per], gates [n][per]) in the kernels' layouts.  The keywords are the mutations
    of tests/test_anysize_ca_host.py, each a subtly wrong tail."""
    y64, sc64, prm64 = np.asarray(y, np.float64), np.asarray(sc, np.float64), np.asarray(prm, np.float64).reshape(3, 100)
    n, h, w, c = y64.shape
    planes = _planes(y64, biased)
    gates = {}
    for k in ("hw", "cw", "hc"):
        row = GATE_ORDER.index(k)
        if swap_cw_hc and k != "hw":
            row = 1 - row
        wts = prm64[row, :98].reshape(2, 7, 7)
        plane = planes[k][:, ::-1] if swap_channels else planes[k]
        acc, _ = _conv7(plane, wts, replicate)
        gates[k] = 1.0 / (1.0 + np.exp(-(acc * prm64[row, 98] + prm64[row, 99])))
    ghc = gates["hc"]                                                       # [n][H][C]
    if transposed_plane:                                                    # the [H][C] buffer read as [C][H]
        ghc = ghc.reshape(n, c, h).transpose(0, 2, 1)
    a = y64 * gates["hw"][:, :, :, None]
    b = y64 * gates["cw"].transpose(0, 2, 1)[:, None, :, :]                 # (C, W) -> [w][c]
    d = y64 * ghc[:, :, None, :]
    if third_on_two:
        t = (a + b) / 3.0 + d
    else:
        t = ((a + b) + d) / 3.0
    out = np.maximum(((a + b) + d + sc64) / 3.0, 0.0) if shortcut_first else np.maximum(t + sc64, 0.0)
    return out, pack_maps(planes), pack_gates(gates)


# ---------------------------------------------------------------------------------------------- the bound
def bounds(y, sc, prm):
    """Per-element bounds (out [n][H][W][C], maps [n][2 per], gates [n][per]) of the kernels' documented order against tail(); the
    derivation is the module's docstring."""
    y64, sc64, prm64 = np.asarray(y, np.float64), np.asarray(sc, np.float64), np.asarray(prm, np.float64).reshape(3, 100)
    n, h, w, c = y64.shape
    planes = _planes(y64)
    absmean = {"hw": np.abs(y64).mean(3), "cw": np.abs(y64).mean(1).transpose(0, 2, 1), "hc": np.abs(y64).mean(2)}
    length = {"hw": c, "cw": h, "hc": w}
    dplanes, gates, dgates = {}, {}, {}
    for k in ("hw", "cw", "hc"):
        ln = length[k]
        std, mean = planes[k][:, 0], planes[k][:, 1]
        dvar = (3 * ln + 4) * V * (std * std + ln / (ln - 1.0) * mean * mean)
        with np.errstate(divide="ignore", invalid="ignore"):
            dstd = np.minimum(np.where(std > 0, dvar / std, np.inf), np.sqrt(dvar)) + U * std
        dmean = ln * V * absmean[k] + U * np.abs(mean)
        dplanes[k] = np.stack([dstd, dmean], 1) + 1e-44
        row = GATE_ORDER.index(k)
        wts = prm64[row, :98].reshape(2, 7, 7)
        acc, mag = _conv7(planes[k], wts)
        prop, _ = _conv7(dplanes[k], np.abs(wts))
        dacc = 98 * U / (1 - 98 * U) * mag + prop
        a = acc * prm64[row, 98] + prm64[row, 99]
        da = abs(prm64[row, 98]) * dacc + U * np.abs(a)
        g = 1.0 / (1.0 + np.exp(-a))
        gates[k] = g
        dgates[k] = g * (1 - g) * da + 0.05 * da * da + 8 * U * g
    ghw, gcw, ghc = gates["hw"][:, :, :, None], gates["cw"].transpose(0, 2, 1)[:, None, :, :], gates["hc"][:, :, None, :]
    dghw, dgcw, dghc = dgates["hw"][:, :, :, None], dgates["cw"].transpose(0, 2, 1)[:, None, :, :], dgates["hc"][:, :, None, :]
    ay = np.abs(y64)
    a, b, d = y64 * ghw, y64 * gcw, y64 * ghc
    dsum = ay * (dghw + dgcw + dghc) + U * (np.abs(a) + np.abs(b) + np.abs(d)) + U * np.abs(a + b) + U * np.abs(a + b + d)
    t = (a + b + d) / 3.0
    dout = dsum / 3.0 + 2 * U * np.abs(t) + U * np.abs(t + sc64)
    return 1.01 * dout + 1e-44, 1.01 * pack_maps(dplanes), 1.01 * pack_gates(dgates)


# ---------------------------------------------------------------------------------------------- fp32 emulation of the documented order
def _fma32(a, b, c):
    """fmaf on float32 arrays: the product is exact in float64, so one rounding to float64 and one to float32 remain."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def emulate(y, sc, prm):
    """The kernels' arithmetic restated with numpy: fp64 sums, var = (s2 - s1 mean) / (L - 1) clamped at 0, std and mean rounded once to
    float32, 98 fmaf in (channel, row, column) order, fmaf(acc, scale, shift), 1 / (1 + exp(-a)) in float32, every product and sum of the
    combine rounded on its own.  Returns (out, maps, gates) as tail() does, float32."""
    y32, sc32, prm32 = np.asarray(y, np.float32), np.asarray(sc, np.float32), np.asarray(prm, np.float32).reshape(3, 100)
    y64 = y32.astype(np.float64)
    n, h, w, c = y32.shape

    def stat(axis):
        ln = y64.shape[axis]
        s1, s2 = y64.sum(axis), (y64 * y64).sum(axis)
        mean = s1 / ln
        var = np.maximum((s2 - s1 * mean) / (ln - 1), 0.0)
        return np.sqrt(var).astype(np.float32), mean.astype(np.float32)
    s, m = stat(3)
    planes = {"hw": np.stack([s, m], 1)}
    s, m = stat(1)
    planes["cw"] = np.stack([s.transpose(0, 2, 1), m.transpose(0, 2, 1)], 1)
    s, m = stat(2)
    planes["hc"] = np.stack([s, m], 1)
    gates = {}
    for k in ("hw", "cw", "hc"):
        row = GATE_ORDER.index(k)
        wts = prm32[row, :98].reshape(2, 7, 7)
        plane = planes[k]
        _, _, p, q = plane.shape
        pad = np.pad(plane, ((0, 0), (0, 0), (3, 3), (3, 3)))
        acc = np.zeros((n, p, q), np.float32)
        for ch in range(2):
            for r in range(7):
                for t in range(7):
                    acc = _fma32(np.broadcast_to(wts[ch, r, t], acc.shape), pad[:, ch, r:r + p, t:t + q], acc)
        a = _fma32(acc, np.broadcast_to(prm32[row, 98], acc.shape), np.broadcast_to(prm32[row, 99], acc.shape))
        gates[k] = (np.float32(1.0) / (np.float32(1.0) + np.exp(-a))).astype(np.float32)
    a = y32 * gates["hw"][:, :, :, None]
    b = y32 * gates["cw"].transpose(0, 2, 1)[:, None, :, :]
    d = y32 * gates["hc"][:, :, None, :]
    t = np.float32(1.0 / 3.0) * ((a + b) + d)
    out = np.maximum(t + sc32, np.float32(0.0))
    assert out.dtype == np.float32
    return out, pack_maps(planes), pack_gates(gates)
