"""numpy float64 restatement of the three kernel families of libreid_hip_anysize.so (csrc/anysize.h) and the error model the GPU test
holds them to (tests/test_gpu_anysize.py); tests/test_anysize_host.py holds the restatement itself to torch.  Activations are NHWC
[n, hw, c] as the kernels see them.  Each function has ONE switch that breaks one rule, for the mutation checks.

Error model, u = 2^-24 (fp32 unit roundoff), SAFETY = 2 (chosen) on every bound.

any_norm.  The device adds x and x^2 (exact in fp64) over the hw pixels of an (image, channel) in fp64 and forms mean, var = max(s2 / hw -
mean^2, 0), inv = 1 / sqrt(var + 1e-5) there, so what the fp32 format would lose to cancellation is CANCEL64 = (hw + 4) 2^-53 (E[x^2] +
mean^2) / (var + eps), far below u.  a = gamma inv and b = beta - mean a are rounded to fp32 once: |da| <= |a| (u + CANCEL64),
|db| <= u |b| + |mean a| CANCEL64 (b is formed in fp64 from the unrounded a).  The output
relu(fma(x, a, b)) has one more rounding: |x| |da| + |db| + u |x a + b|; ReLU is 1-Lipschitz.  The BatchNorm half is fma(x, s, t): u |x s + t|.

any_se_tail.  pooled = fp32(sum64 / hw): u |pooled|.  A hidden unit is a chain of c / 64 fused multiply-adds per lane and six shuffle
additions: d_h <= (c / 64 + 8) u sum |w1| |pooled| (the 8: six additions, the rounding of pooled, one spare).  The gate's argument is a chain
of mid fused multiply-adds: mid u sum |w2| |h| + sum |w2| d_h; sigmoid' <= 1 / 4, and expf, the addition and the division add 4 u g (chosen, as
tests/test_gpu_tail.py).  out = relu(fma(g, y, sc)): |y| d_g + u |g y + sc|.

any_gem.  A term max(x, 1e-6)^p is formed in fp32 - p == 3: x x x, E_term = 2u; a trained p: exp2(p log2 x) on v_log_f32 / v_exp_f32,
E_term = E_EXP + ln2 (|p| E_LOG max(|log2 x|, 1) + u |p log2 x|) with E_LOG = E_EXP = 2^-22 as tests/test_gpu_tail.py chose and measured
(a term below 2^-126 is a subnormal and adds 2^-150 / x^p) - and added in fp64, m = fp32(sum64 / hw): rel(m) <= E_term + u + 2^-40.
g = cbrtf(m) or powf(m, 1 / p): rel(g) <= rel(m) / p + |ln m| u / p + 4u (the rounding of 1 / p; powf / cbrtf: chosen).  emb = fma(g, scale,
shift): |scale| g rel(g) + u (|g scale| + |shift|).
"""
import numpy as np

U = 2.0 ** -24
SAFETY = 2.0
EPS = 1e-5
E_LOG = E_EXP = 2.0 ** -22
GEM_EPS = 1e-6


def instance_norm(x, gamma, beta, half, bn_scale=None, bn_shift=None, sample_variance=False):
    """relu(IBN(x)) in float64: x [n, hw, c]; channels < half InstanceNorm (biased variance), the rest x * bn_scale + bn_shift (or left as
    they are when bn_scale is None).  Returns (out, bound) - bound is the per-element limit of the module docstring, SAFETY included."""
    x64 = np.asarray(x, np.float64)
    n, hw, c = x64.shape
    out = x64.copy()
    bound = np.zeros_like(x64)
    xi = x64[:, :, :half]
    mean = xi.mean(axis=1, keepdims=True)
    ex2 = (xi * xi).mean(axis=1, keepdims=True)
    var = np.maximum(ex2 - mean * mean, 0.0)
    if sample_variance:
        var = var * hw / max(hw - 1, 1)
    g, b0 = np.asarray(gamma, np.float64)[None, None, :], np.asarray(beta, np.float64)[None, None, :]
    a = g / np.sqrt(var + EPS)
    b = b0 - mean * a
    pre = xi * a + b
    out[:, :, :half] = np.maximum(pre, 0.0)
    cancel = (hw + 4) * 2.0 ** -53 * (ex2 + mean * mean) / (var + EPS)
    da = np.abs(a) * (U + cancel)
    db = U * np.abs(b) + np.abs(mean * a) * cancel
    bound[:, :, :half] = np.abs(xi) * da + db + U * np.abs(pre)
    if bn_scale is not None and half < c:
        s, t = np.asarray(bn_scale, np.float64)[None, None, :], np.asarray(bn_shift, np.float64)[None, None, :]
        pre = x64[:, :, half:] * s + t
        out[:, :, half:] = np.maximum(pre, 0.0)
        bound[:, :, half:] = U * np.abs(pre)
    return out, SAFETY * bound + 1e-45


def se_tail(y, shortcut, w1, w2t, avg_over=None):
    """SEBlock + combine in float64: y / shortcut [n, hw, c], w1 [mid, c], w2t [mid, c] (fc2 transposed).  avg_over: the divisor of the
    average pool (None: hw).  Returns (out, gate, out_bound, gate_bound)."""
    y64, s64 = np.asarray(y, np.float64), np.asarray(shortcut, np.float64)
    w1, w2t = np.asarray(w1, np.float64), np.asarray(w2t, np.float64)
    n, hw, c = y64.shape
    mid = w1.shape[0]
    pooled = y64.sum(axis=1) / (hw if avg_over is None else avg_over)            # [n, c]
    pre_h = pooled @ w1.T                                                       # [n, mid]
    h = np.maximum(pre_h, 0.0)
    z = h @ w2t                                                                 # [n, c]
    gate = 1.0 / (1.0 + np.exp(-z))
    pre = gate[:, None, :] * y64 + s64
    out = np.maximum(pre, 0.0)
    d_h = (c / 64 + 8) * U * (np.abs(pooled) @ np.abs(w1).T)
    d_z = mid * U * (np.abs(h) @ np.abs(w2t)) + d_h @ np.abs(w2t)
    d_g = 0.25 * d_z + 4 * U * gate
    out_bound = np.abs(y64) * d_g[:, None, :] + U * np.abs(pre)
    return out, gate, SAFETY * out_bound + 1e-45, SAFETY * d_g


def gem(x, p, scale, shift, clamp=True):
    """GeM + BNNeck in float64: x [n, hw, c] -> (gem [n, c], emb [n, c], gem_bound, emb_bound)."""
    x64 = np.asarray(x, np.float64)
    n, hw, c = x64.shape
    p = float(np.float32(p))
    f = np.maximum(x64, GEM_EPS) if clamp else x64
    term = f ** p
    m = term.mean(axis=1)
    g = m ** (1.0 / p)
    scale, shift = np.asarray(scale, np.float64)[None, :], np.asarray(shift, np.float64)[None, :]
    emb = g * scale + shift
    if not clamp:
        return g, emb, None, None
    if p == 3.0:
        e_term = np.full_like(term, 2 * U)
    else:
        l2 = np.log2(f)
        e_term = E_EXP + np.log(2.0) * (abs(p) * E_LOG * np.maximum(np.abs(l2), 1.0) + U * np.abs(p * l2))
        e_term = e_term + np.where(term < 2.0 ** -126, 2.0 ** -150 / term, 0.0)
    rel_m = (term * e_term).mean(axis=1) / m + U + 2.0 ** -40
    rel_g = rel_m / abs(p) + np.abs(np.log(m)) * U / abs(p) + 4 * U
    emb_bound = np.abs(scale) * g * rel_g + U * (np.abs(g * scale) + np.abs(shift))
    return g, emb, SAFETY * g * rel_g, SAFETY * emb_bound


def pass_size(chunk, h, w):
    """Images per pass of the any-size forward (include/reid_hip.h): chunk * 256 * 128 / (h * w), clamped to 1 .. 4096."""
    return max(1, min(4096, chunk * 256 * 128 // (h * w)))


def stage_shapes(h, w):
    """(Ho, Wo, C) of the stem, the max-pool and the eight blocks for an h x w input (conv 7/2/3, pool 3/2/1, 3x3 convolutions p1)."""
    conv = lambda v, k, s, pad: (v + 2 * pad - k) // s + 1
    hh, ww = conv(h, 7, 2, 3), conv(w, 7, 2, 3)
    out = [(hh, ww, 64)]
    hh, ww = conv(hh, 3, 2, 1), conv(ww, 3, 2, 1)
    out.append((hh, ww, 64))
    for c, s in ((64, 1), (64, 1), (128, 2), (128, 1), (256, 2), (256, 1), (512, 1), (512, 1)):
        hh, ww = conv(hh, 3, s, 1), conv(ww, 3, s, 1)
        out.append((hh, ww, c))
    return out
