"""float64 oracles, error bounds, case tables and an fp16-storage restatement of the forward for libreid_hip_anysize_f16.so
(csrc/anysize_f16.h): ResNet18-IBN-SE at any input size in fp16 storage with fp32 accumulation.  tests/test_gpu_anysize_f16.py holds the
kernels to these on the MI355X; tests/test_anysize_f16_host.py holds the restatement to the reference fixture and shows, for each kernel
family, one mutation the GPU check would catch.

Notation: u = 2^-24 (fp32 unit roundoff), H = 2^-11 (f16 half-ulp, relative), 2^-25 (the same below f16's normal range, absolute),
SAFETY = 2 (chosen, as in tests/test_gpu_conv_f16.py and tests/anysize_ref.py).

Convolution and stem (the bound tests/test_gpu_conv_f16.py derives for f16 operands, fp32 accumulation, one f16 rounding at the store).
Operands are f16 values, so every product is exact in fp32's 48-bit product and the error is the accumulation's: with A = sum_k |x_k w_k|,
    e32 = SAFETY (|scale| K u A + 4u (|acc scale| + |shift| + |res|)),   bound = e32 + H (|v| + e32) + 2^-25,
v the float64 epilogue value; ReLU is 1-Lipschitz.  K = r r cin for the trunk, 147 for the stem (its 45 padding columns are zero).  On the
EXACT family (small integers, |sum of magnitudes| < 2^24) fp32 accumulation is exact in any order and the store is the single rounding of
an exactly known value: the kernel has to return float16(acc) bit for bit.

Max-pool: a maximum of stored f16 values is one of them: bit for bit.

Tails: statistics, gates and GeM are formed exactly as libreid_hip_anysize.so forms them (fp64 sums in a fixed order, fp32 gate), on
inputs that are f16 values; tests/anysize_ref.py's bounds b32 for the fp32 value apply unchanged, and the f16 store adds one rounding:
    bound = b32 + H (|v| + b32) + 2^-25.
GeM and the neck are stored in fp32: b32 as it is.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import anysize_ref as ref  # noqa: E402
import anysize_x3_ref as x3  # noqa: E402

U = 2.0 ** -24
H = 2.0 ** -11
H_ABS = 2.0 ** -25
SAFETY = 2.0

# ---- case tables
GEOMS = x3.GEOMS                                   # the eleven trunk geometries (module docstring of tests/anysize_x3_ref.py)
FORM_OF_COUT = {64: 1, 128: 2, 256: 2, 512: 2}     # anysize_f16.h: 128 x 64 tiles for 64 output channels, 128 x 128 above
RES_RELU = ("l1big", "l2", "l3", "l4")             # geometries run with a residual and ReLU
RELU_FROM_HALF = ("l1", "l2s")                     # ... with ReLU on the second half of the channels only (the IBN blocks' conv1)
STEM_SIZES = ((33, 47), (64, 32))                  # odd H1 / W1 with several ragged tiles; the smallest even case
STEM_N = 2
TAIL_HWS = (4, 8, 30, 108, 238)                    # 2 x 2 (less than a wavefront) .. more than one trip of the four-deep pixel walk
TAIL_CS = (64, 512)
TAIL_N = 3
FORWARD_CASES = (0, 1, 2)                          # tests/golden/anysize.npz: (64, 32), (96, 72), (224, 268)
COS_LIMIT, EMB_LIMIT, STAGE_LIMIT = 1e-4, 2e-2, 2e-2   # the mode-1 limits of tests/test_gpu_parity.py


def f16(v):
    """Round to float16 once (round to nearest even, subnormals kept) and return the values as float64."""
    return np.asarray(v, np.float64).astype(np.float16).astype(np.float64)


def store_bound(v, b32):
    return b32 + H * (np.abs(v) + b32) + H_ABS


# ---------------------------------------------------------------------------------------------- convolution
def conv_operands(name, seed):
    """Random f16 operands of geometry `name`: (x, w, scale, shift, res), x / w / res float16, scale / shift float32."""
    cin, cout, r, stride, h, w, n = GEOMS[name]
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, h, w, cin)).astype(np.float16)
    wt = rng.normal(0, np.sqrt(2.0 / (r * r * cin)), (cout, r, r, cin)).astype(np.float16)
    scale = rng.uniform(0.5, 1.5, cout).astype(np.float32)
    shift = rng.normal(size=cout).astype(np.float32)
    ho, wo = x3.out_hw(name)
    res = rng.normal(size=(n, ho, wo, cout)).astype(np.float16)
    return x, wt, scale, shift, res


def exact_operands(name, seed):
    """Small integers: x in -3 .. 3 kept with probability 0.25, w in -2 .. 2; every sum of magnitudes is an integer below 2^24."""
    cin, cout, r, stride, h, w, n = GEOMS[name]
    rng = np.random.default_rng(seed)
    x = rng.integers(-3, 4, (n, h, w, cin)) * (rng.random((n, h, w, cin)) < 0.25)
    wt = rng.integers(-2, 3, (cout, r, r, cin))
    return x.astype(np.float16), wt.astype(np.float16)


def conv_oracle(x, wt, stride, pad_mode="zero"):
    """(acc, A) in float64 on every output element [n ho wo, cout].  pad_mode "edge": padding taps read the nearest pixel (mutation)."""
    x64, w64 = np.asarray(x, np.float64), np.asarray(wt, np.float64)
    r = w64.shape[1]
    if pad_mode == "edge" and r == 3:
        n, h, w, c = x64.shape
        xp = np.pad(x64, ((0, 0), (1, 1), (1, 1), (0, 0)), mode="edge")
        ho, wo = (h + 2 - 3) // stride + 1, (w + 2 - 3) // stride + 1
        cols = [xp[:, ty:ty + (ho - 1) * stride + 1:stride, tx:tx + (wo - 1) * stride + 1:stride] for ty in range(3) for tx in range(3)]
        a = np.stack(cols, 3).reshape(n * ho * wo, 9 * c)
    else:
        a = x3.im2col(x64, r, stride)
    b = w64.reshape(w64.shape[0], -1).T
    return a @ b, np.abs(a) @ np.abs(b)


def epilogue(acc, scale=None, shift=None, res=None, relu=False, relu_from=0):
    v = np.array(acc, np.float64)
    if scale is not None:
        v = v * np.asarray(scale, np.float64)[None, :] + np.asarray(shift, np.float64)[None, :]
    if res is not None:
        v = v + np.asarray(res, np.float64).reshape(v.shape)
    if relu:
        v[:, relu_from:] = np.maximum(v[:, relu_from:], 0.0)
    return v


def conv_bound(acc, ab, k, v, scale=None, shift=None, res=None):
    sc = 1.0 if scale is None else np.abs(np.asarray(scale, np.float64))[None, :]
    sh = 0.0 if shift is None else np.abs(np.asarray(shift, np.float64))[None, :]
    rr = 0.0 if res is None else np.abs(np.asarray(res, np.float64).reshape(acc.shape))
    e32 = SAFETY * (sc * k * U * ab + 4 * U * (np.abs(acc * sc) + sh + rr))
    return store_bound(v, e32)


def conv_case(name, seed):
    """The GPU test's random case of geometry `name`: (kwargs of Engine.debug_any_conv_f16, x, wt, want float64, bound)."""
    cin, cout, r, stride, h, w, n = GEOMS[name]
    x, wt, scale, shift, res = conv_operands(name, seed)
    kw = dict(scale=scale, shift=shift)
    if name in RES_RELU:
        kw.update(res=res, relu=True)
    elif name in RELU_FROM_HALF:
        kw.update(relu=True, relu_from=cout // 2)
    acc, ab = conv_oracle(x, wt, stride)
    want = epilogue(acc, scale, shift, kw.get("res"), kw.get("relu", False), kw.get("relu_from", 0))
    return kw, x, wt, want, conv_bound(acc, ab, r * r * cin, want, scale, shift, kw.get("res"))


# ---------------------------------------------------------------------------------------------- stem and max-pool
def stem_pack16(w):
    """[64, 7, 7, 3] (cout, r, s, c) -> float16 [64, 192], k = r 24 + s 3 + c, zero padded: the f16 image of weights.stem_pack's rows."""
    out = np.zeros((64, 8, 24), np.float16)
    out[:, :7, :21] = np.asarray(w, np.float32).reshape(64, 7, 21).astype(np.float16)
    return out.reshape(64, 192)


def stem_operands(h, w, seed, n=STEM_N):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, h, w, 3)).astype(np.float32)
    wt = rng.normal(0, np.sqrt(2.0 / 147), (64, 7, 7, 3)).astype(np.float32)
    return x, wt, rng.uniform(0.5, 1.5, 64).astype(np.float32), rng.normal(size=64).astype(np.float32)


def stem_oracle(x, wt, scale, shift):
    """(want, bound) [n, H1, W1, 64] of conv 7x7 s2 p3 + BN on f16(x), f16(wt) in float64."""
    x16, w16 = f16(x), f16(wt)
    n, h, w, _ = x16.shape
    xp = np.zeros((n, h + 6, w + 6, 3))
    xp[:, 3:3 + h, 3:3 + w] = x16
    h1, w1 = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    cols = [xp[:, r:r + (h1 - 1) * 2 + 1:2, s:s + (w1 - 1) * 2 + 1:2] for r in range(7) for s in range(7)]
    a = np.stack(cols, 3).reshape(n * h1 * w1, 147)
    b = w16.reshape(64, 147).T
    acc, ab = a @ b, np.abs(a) @ np.abs(b)
    want = epilogue(acc, scale, shift)
    return want.reshape(n, h1, w1, 64), conv_bound(acc, ab, 147, want, scale, shift).reshape(n, h1, w1, 64)


def maxpool(x, pad_value=-np.inf):
    """MaxPool2d(3, 2, 1) on NHWC; pad_value 0: the padded border takes part as zeros (mutation)."""
    x = np.asarray(x)
    n, h, w, c = x.shape
    xp = np.full((n, h + 2, w + 2, c), pad_value, np.float64)
    xp[:, 1:1 + h, 1:1 + w] = x
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    out = np.full((n, ho, wo, c), -np.inf)
    for dy in range(3):
        for dx in range(3):
            out = np.maximum(out, xp[:, dy:dy + (ho - 1) * 2 + 1:2, dx:dx + (wo - 1) * 2 + 1:2])
    return out


# ---------------------------------------------------------------------------------------------- tails
def tail_data(hw, c, seed, n=TAIL_N):
    rng = np.random.default_rng(seed * 100003 + hw * 7 + c)
    x = (rng.normal(0.3, 1.0, (n, hw, c)) * rng.uniform(0.5, 2.0, (1, 1, c))).astype(np.float16)
    return rng, x


def norm_case(hw, c):
    rng, x = tail_data(hw, c, 1)
    half = c // 2
    gamma, beta = rng.uniform(0.5, 1.5, half).astype(np.float32), rng.normal(0, 0.2, half).astype(np.float32)
    return x, half, gamma, beta


def norm_oracle(x, gamma, beta, half, sample_variance=False):
    """IBN finish of channels < half on f16 values: (want, bound) [n, hw, half]."""
    v, b32 = ref.instance_norm(np.asarray(x, np.float64), gamma, beta, half, sample_variance=sample_variance)
    return v[:, :, :half], store_bound(v[:, :, :half], b32[:, :, :half])


def se_case(hw, c):
    rng, y = tail_data(hw, c, 2)
    sc = rng.normal(0, 1, y.shape).astype(np.float16)
    mid = max(c // 16, 8)
    w1 = rng.normal(0, 1 / np.sqrt(c), (mid, c)).astype(np.float32)
    w2t = rng.normal(0, 1 / np.sqrt(mid), (mid, c)).astype(np.float32)
    return y, sc, w1, w2t


def se_oracle(y, sc, w1, w2t, gate_first=False):
    """(out, gate, out_bound, gate_bound); gate_first: relu(gate * (y + shortcut)), the gate applied before the residual (mutation)."""
    y64, s64 = np.asarray(y, np.float64), np.asarray(sc, np.float64)
    out, gate, b32, gb = ref.se_tail(y64, s64, w1, w2t)
    if gate_first:
        out = np.maximum(gate[:, None, :] * (y64 + s64), 0.0)
    return out, gate, store_bound(out, b32), gb


def gem_case(hw, c):
    rng, x = tail_data(hw, c, 3)
    x[0, 0, :] = 0.0
    return x, rng.uniform(0.5, 1.5, c).astype(np.float32), rng.normal(0, 0.2, c).astype(np.float32)


# ---------------------------------------------------------------------------------------------- the forward, restated
def forward_f16(sd, x, taps=None):
    """oracle/seres18.py's seres18_ibn forward with the rounding points of the fp16-storage any-size forward, everything else float64:
    input, weights and every stored activation are rounded to f16 once; BatchNorm is the folded (scale, shift) pair in the producing
    convolution's epilogue; conv1 of an IBN block stores its InstanceNorm half raw and finished, its BatchNorm half finished;
    statistics, gates, GeM, neck and classifier are not rounded.  x: float32 [n, 3, h, w].  Returns (emb, logits) float64 and fills
    `taps` with the stage maps under oracle names (NCHW)."""
    import torch
    import torch.nn.functional as F
    from oracle import seres18

    def t(k):
        return seres18._t(sd, k).to(torch.float64)

    def r16(v):
        return v.to(torch.float16).to(torch.float64)

    def fold(prefix):
        s = t(prefix + ".weight") / torch.sqrt(t(prefix + ".running_var") + seres18.BN_EPS)
        return s.reshape(1, -1, 1, 1), (t(prefix + ".bias") - t(prefix + ".running_mean") * s).reshape(1, -1, 1, 1)

    with torch.no_grad():
        x = r16(torch.as_tensor(np.asarray(x)).to(torch.float64))
        s, b = fold("bn0")
        x = r16(F.conv2d(x, r16(t("conv0.weight")), None, 2, 3) * s + b)
        if taps is not None:
            taps["stem"] = x
        x = F.max_pool2d(x, 3, 2, 1)
        if taps is not None:
            taps["pool0"] = x
        for name, c, ibn, ds, stride in seres18.BLOCKS:
            pre = name + ".block_pre"
            acc = F.conv2d(x, r16(t(pre + ".conv1.weight")), None, stride, 1)
            if ibn:
                half = c // 2
                s, b = fold(pre + ".bn1.BN")
                raw = r16(acc[:, :half])
                bn = r16(F.relu(acc[:, half:] * s + b))
                inn = F.instance_norm(raw, None, None, t(pre + ".bn1.IN.weight"), t(pre + ".bn1.IN.bias"), True, 0.0, seres18.IN_EPS)
                h1 = torch.cat((r16(F.relu(inn)), bn), 1)
            else:
                s, b = fold(pre + ".bn1")
                h1 = r16(F.relu(acc * s + b))
            s, b = fold(pre + ".bn2")
            y = F.conv2d(h1, r16(t(pre + ".conv2.weight")), None, 1, 1) * s + b
            if ds:
                y = r16(y)
                s, b = fold(name + ".block_post.bn")
                sc = r16(F.conv2d(x, r16(t(name + ".block_post.conv.weight")), None, stride, 0) * s + b)
            else:
                y = r16(F.relu(y + x))
                sc = x
            n_, c_ = y.shape[:2]
            pooled = y.mean(dim=(2, 3))
            hid = F.relu(pooled @ t(name + ".seblock.fc1.weight").reshape(-1, c_).t())
            gate = torch.sigmoid(hid @ t(name + ".seblock.fc2.weight").t()).reshape(n_, c_, 1, 1)
            x = r16(F.relu(gate * y + sc))
            if taps is not None:
                taps[name] = x
        p = t("avgpooling.p")
        feat = x.clamp(min=seres18.GEM_EPS).pow(p).mean(dim=(2, 3)).pow(1.0 / p)
        if taps is not None:
            taps["gem"] = feat
        s = t("bnneck.weight") / torch.sqrt(t("bnneck.running_var") + seres18.BN_EPS)
        emb = feat * s + (t("bnneck.bias") - t("bnneck.running_mean") * s)
        logits = emb @ t("classifier.0.weight").t()
    return emb.numpy(), logits.numpy()
