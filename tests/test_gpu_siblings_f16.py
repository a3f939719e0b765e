"""The fp16-storage mode (precision 1) of CARes18-IBN and EMARes18-IBN: the two launchers of libreid_hip_siblings_f16.so
(csrc/siblings_f16.hip) through ctypes against a float64 oracle, and both models end to end against tests/golden/siblings.npz.
Run on an MI355X: pytest -m gpu tests/test_gpu_siblings_f16.py.

Kernel level.  The oracle restates the tails in float64 (triplet_attention.py:46-101 with CARes18.py:150-157; EMA_Res18.py:23-38 with
:79-86) on the same f16-rounded y and shortcut.  Shapes: the four geometries the forward produces, n = 1 and n = 3.  y is N(0,1)
times a per-channel scale in [0.25, 4] plus a per-channel mean in [-2, 2]; the shortcut is N(0,1); the "x8" cases multiply the conv
weights of the gates by 8, which pushes gates to 0 and 1.  Outputs are pre-filled with the f16 NaN pattern 0xffff and checked densely.

Error model: u = 2^-24.  out = relu(y g + sc) (EMA) or relu(y (g_hw + g_cw + g_hc) / 3 + sc) (TripletAttention), g the gates.  ReLU is
1-Lipschitz, so the bound is that of its argument v:
    |err| <= 2^-11 |v| + 2^-25            the one f16 rounding (2^-25 absolute below f16's normal range)
           + 8 u (|y| + |sc|)             the fp32 products, sums and the 1/3 in front of that rounding (at most 6 roundings; 8 chosen)
           + |y| d_gate                   the error of the gate
d_gate cannot be derived here: nothing on the build machine states the accuracy of the device's expf, and the conditioning of the
std / GroupNorm statistics depends on the implementation.  It is measured, per case, on the exact-fp32 tails of attention_f32.hip
(reid_debug_sibling_tail) against the same oracle on the same inputs: e32 = max |out32 - oracle| / |y| over the elements with
|y| >= 1 whose oracle value is above zero, and d_gate = SAFETY e32 with SAFETY = 2 (the factor tests/test_gpu_tail.py chose).  The
bound never comes from the kernels under test.  "e16" below is the same figure for the new kernels with the f16 rounding
taken out (max (|out16 - oracle| - 2^-11 |v| - 2^-25) / |y|), recorded, not asserted.  Every case prints its line (pytest -s).
Measured on an MI355X (profiles/siblings_f16_gpu_tests.log):

  tail  geometry      n  weights   e32 (fp32 tails)   e16 (new kernels)   worst |err| / bound
  ta    64x32x64      1  x1        1.836e-07          0.000e+00           0.992
  ta    64x32x64      3  x1        1.895e-07          1.961e-08           0.995
  ta    32x16x128     1  x1        1.834e-07          0.000e+00           0.990
  ta    32x16x128     3  x1        2.157e-07          1.228e-08           0.989
  ta    16x8x256      1  x1        2.149e-07          0.000e+00           0.994
  ta    16x8x256      3  x1        2.358e-07          0.000e+00           0.995
  ta    16x8x512      1  x1        1.854e-07          1.707e-08           0.991
  ta    16x8x512      3  x1        1.854e-07          1.707e-08           0.996
  ema   64x32x64      1  x1        3.058e-07          2.276e-09           0.984
  ema   64x32x64      3  x1        3.292e-07          1.032e-07           0.996
  ema   32x16x128     1  x1        3.038e-07          4.781e-08           0.997
  ema   32x16x128     3  x1        3.114e-07          4.781e-08           0.997
  ema   16x8x256      1  x1        2.119e-07          0.000e+00           0.989
  ema   16x8x256      3  x1        2.736e-07          1.579e-07           0.993
  ema   16x8x512      1  x1        2.436e-07          0.000e+00           0.987
  ema   16x8x512      3  x1        2.436e-07          1.635e-08           0.995
  ta    32x16x128     3  x8        7.538e-07          8.863e-10           0.997
  ema   16x8x512      3  x8        1.272e-06          2.533e-07           0.991

The f16 rounding is nearly the whole bound (worst |err| / bound 0.98 - 0.997: a value that lands next to an f16 tie); the new kernels' gate
error is at or below the fp32 tails' in every case.  So that a regression of the fp32 tails cannot loosen the bound unseen, e32 itself is
held to twice the worst value recorded above for its tail and weights (E32_RECORDED).
Image 0 of the n = 3 call equals the n = 1 call bit for bit (the slicing depends on the geometry alone).

End to end: weights and crops of test_sibling_backbones_match_reference_fixture, precision 1.  Block taps survive a round trip through
float16 (they are f16 values) and are within the bar test_seres18_f16_path_within_north_star_tolerance holds mode 1 of seres18_ibn to
(max |tap - ref| <= 1e-2 max |ref|); 1 - cos < 1e-4 (measured: cares18_ibn 6.0e-8, emares18_ibn 6.0e-8; through the production kernels of a large pass, debug_keep 2: 6.0e-8 and 1.2e-7; block taps 5.8e-4 - 2.4e-3); a single crop equals row 0 of the
batch to that test's 2e-3 max |emb|; mode 0 before and after the mode-1 call agree bit for bit; and without the library beside
libreid_hip.so the mode-1 embed raises ReidHipError naming it (a child process on a copy of the package).
"""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from reid_amd import _ffi, synth

gpu = pytest.mark.gpu

U = 2.0 ** -24
H16 = 2.0 ** -11
H16_ABS = 2.0 ** -25
SAFETY = 2.0            # chosen (tests/test_gpu_tail.py)
ARITH = 8.0             # fp32 roundings in front of the f16 one (module docstring)
# worst e32 of the fp32 tails recorded on an MI355X per (tail, x8 weights) - the module docstring's table; e32 is asserted <= 2x this
E32_RECORDED = {("ta", False): 2.358e-07, ("ema", False): 3.292e-07, ("ta", True): 7.538e-07, ("ema", True): 1.272e-06}

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "real-time-reid-tracking_amd")
SIB_LIB = "libreid_hip_siblings_f16.so"
GEOMS = [(64, 32, 64), (32, 16, 128), (16, 8, 256), (16, 8, 512)]
BLOCK_C = [64, 64, 128, 128, 256, 256, 512, 512]
BLOCK_HW = [(64, 32), (64, 32), (32, 16), (32, 16), (16, 8), (16, 8), (16, 8), (16, 8)]


# ----------------------------------------------------------------------------- float64 oracles
def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _conv2d(x, w, pad):
    """x [n, ci, P, Q], w [co, ci, k, k] -> [n, co, P, Q], zero padding, float64."""
    n, ci, P, Q = x.shape
    k = w.shape[-1]
    xp = np.zeros((n, ci, P + 2 * pad, Q + 2 * pad))
    xp[:, :, pad:pad + P, pad:pad + Q] = x
    out = np.zeros((n, w.shape[0], P, Q))
    for r in range(k):
        for s in range(k):
            out += np.einsum("oc,ncpq->nopq", w[:, :, r, s], xp[:, :, r:r + P, s:s + Q])
    return out


def ta_oracle(y, sc, wts):
    """y, sc [n, H, W, C] float64; wts [3][100] = (cw, hc, hw) x (conv [2][7][7], BN scale, BN shift).  Returns relu's argument."""
    def gate(std, mean, wt):                     # planes [n, P, Q]
        z = _conv2d(np.stack([std, mean], 1), wt[:98].reshape(1, 2, 7, 7), 3)[:, 0]
        return _sigmoid(z * wt[98] + wt[99])
    wts = np.asarray(wts, np.float64)
    s_hw = gate(y.std(3, ddof=1), y.mean(3), wts[2])                                              # [n, H, W]
    s_cw = gate(y.std(1, ddof=1).transpose(0, 2, 1), y.mean(1).transpose(0, 2, 1), wts[0])        # [n, C, W]
    s_hc = gate(y.std(2, ddof=1), y.mean(2), wts[1])                                              # [n, H, C]
    g = s_hw[:, :, :, None] + s_cw.transpose(0, 2, 1)[:, None, :, :] + s_hc[:, :, None, :]
    return y * g / 3.0 + sc


def ema_oracle(y, sc, prm):
    n, H, W, C = y.shape
    cg = C // 32
    prm = np.asarray(prm, np.float64)
    o = 0
    w1 = prm[o:o + cg * cg].reshape(cg, cg); o += cg * cg
    b1 = prm[o:o + cg]; o += cg
    w3 = prm[o:o + cg * cg * 9].reshape(cg, cg, 3, 3); o += cg * cg * 9
    b3 = prm[o:o + cg]; o += cg
    gw = prm[o:o + cg]; o += cg
    gb = prm[o:o + cg]
    g = y.reshape(n, H, W, 32, cg).transpose(0, 3, 4, 1, 2).reshape(n * 32, cg, H, W)
    cat = np.concatenate([g.mean(3), g.mean(2)], 2)                                              # [b, cg, H + W]
    sig = _sigmoid(np.einsum("oc,bcj->boj", w1, cat) + b1[None, :, None])
    x1 = g * sig[:, :, :H, None] * sig[:, :, None, H:]
    x2 = _conv2d(g, w3, 1) + b3[None, :, None, None]
    mu = x1.mean((2, 3), keepdims=True)
    var = x1.var((2, 3), keepdims=True)
    x1 = (x1 - mu) / np.sqrt(var + 1e-5) * gw[None, :, None, None] + gb[None, :, None, None]

    def softmax(a):
        e = np.exp(a - a.max(1, keepdims=True))
        return e / e.sum(1, keepdims=True)
    a1, a2 = softmax(x1.mean((2, 3))), softmax(x2.mean((2, 3)))
    wgt = (a1[:, :, None, None] * x2).sum(1) + (a2[:, :, None, None] * x1).sum(1)                # [b, H, W]
    out = g * _sigmoid(wgt)[:, None]
    return out.reshape(n, 32, cg, H, W).transpose(0, 3, 4, 1, 2).reshape(n, H, W, C) + sc


# ----------------------------------------------------------------------------- inputs, computed once per case
def _inputs(tail, H, W, C, n, x8):
    rng = np.random.default_rng([{"ta": 1, "ema": 2}[tail], H, W, C, int(x8)])     # n is not in the seed: image 0 is shared
    scale = rng.uniform(0.25, 4.0, C)
    mean = rng.uniform(-2.0, 2.0, C)
    y = (rng.standard_normal((3, H, W, C)) * scale + mean)[:n].astype(np.float16)
    sc = rng.standard_normal((3, H, W, C))[:n].astype(np.float16)
    k = 8.0 if x8 else 1.0
    if tail == "ta":
        prm = np.concatenate([rng.normal(0, 0.1, (3, 98)) * k, rng.uniform(0.5, 1.5, (3, 1)), rng.normal(0, 0.2, (3, 1))], 1)
    else:
        cg = C // 32
        prm = np.concatenate([rng.normal(0, cg ** -0.5, cg * cg) * k, rng.normal(0, 0.1, cg), rng.normal(0, (9 * cg) ** -0.5, cg * cg * 9) * k,
                              rng.normal(0, 0.1, cg), rng.uniform(0.5, 1.5, cg), rng.normal(0, 0.2, cg)])
    return y, sc, np.ascontiguousarray(prm, np.float32)


_CACHE = {}


def _case(tail, H, W, C, n, x8):
    """(y16, sc16, prm, oracle argument of the ReLU) - the oracle of a case is computed once and shared, read-only."""
    key = (tail, H, W, C, n, x8)
    if key not in _CACHE:
        y, sc, prm = _inputs(tail, H, W, C, n, x8)
        ref = (ta_oracle if tail == "ta" else ema_oracle)(y.astype(np.float64), sc.astype(np.float64), prm)
        for a in (y, sc, prm, ref):
            a.setflags(write=False)
        _CACHE[key] = (y, sc, prm, ref)
    return _CACHE[key]


@pytest.fixture(scope="module")
def eng():
    from reid_amd.engine import get_engine
    return get_engine(0)


@pytest.fixture(scope="module")
def sib():
    lib = ctypes.CDLL(os.path.join(PKG, SIB_LIB))
    lib.siblings_f16_ta_workspace_bytes.restype = ctypes.c_size_t
    lib.siblings_f16_ta_workspace_bytes.argtypes = [ctypes.c_int] * 4
    vp, i = ctypes.c_void_p, ctypes.c_int
    lib.siblings_f16_ta_tail.argtypes = [vp, vp, vp, i, i, i, i, vp, vp, vp]
    lib.siblings_f16_ema_tail.argtypes = [vp, vp, vp, i, i, i, i, vp, vp]
    return lib


def _run16(sib, tail, y, sc, prm):
    """The launcher on the null stream; out pre-filled with f16 NaNs.  Returns the f16 result [n, H, W, C]."""
    import torch
    n, H, W, C = y.shape
    dy, dsc = torch.from_numpy(y.copy()).cuda(), torch.from_numpy(sc.copy()).cuda()
    dp = torch.from_numpy(prm.copy()).cuda()
    dout = torch.full((n, H, W, C), -1, dtype=torch.int16, device="cuda")                        # 0xffff: an f16 NaN
    torch.cuda.synchronize()
    if tail == "ta":
        nbytes = sib.siblings_f16_ta_workspace_bytes(n, H, W, C)
        assert nbytes > 0
        ws = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        rc = sib.siblings_f16_ta_tail(None, dy.data_ptr(), dsc.data_ptr(), n, H, W, C, dp.data_ptr(), ws.data_ptr(), dout.data_ptr())
    else:
        rc = sib.siblings_f16_ema_tail(None, dy.data_ptr(), dsc.data_ptr(), n, H, W, C, dp.data_ptr(), dout.data_ptr())
    assert rc == 0, "hipError %d" % rc
    torch.cuda.synchronize()
    return dout.cpu().numpy().view(np.float16)


CASES = [(t, g, n, False) for t in ("ta", "ema") for g in GEOMS for n in (1, 3)] + [("ta", GEOMS[1], 3, True), ("ema", GEOMS[3], 3, True)]


@gpu
@pytest.mark.parametrize("tail,geom,n,x8", CASES, ids=["%s-%dx%dx%d-n%d%s" % (t, g[0], g[1], g[2], n, "-x8" if x else "") for t, g, n, x in CASES])
def test_f16_tail_against_float64(eng, sib, tail, geom, n, x8):
    H, W, C = geom
    y, sc, prm, ref = _case(tail, H, W, C, n, x8)
    y64, sc64 = y.astype(np.float64), sc.astype(np.float64)
    # the yardstick: the exact-fp32 tail of attention_f32.hip on the same (f16-valued) inputs
    out32 = eng.debug_sibling_tail(1 if tail == "ta" else 2, prm, y.astype(np.float32), sc.astype(np.float32)).astype(np.float64)
    assert not np.isnan(out32).any()
    sel = (np.abs(y64) >= 1.0) & (ref > 0.0)
    assert sel.sum() > 1000
    e32 = (np.abs(out32 - ref)[sel] / np.abs(y64)[sel]).max()
    assert e32 <= 2.0 * E32_RECORDED[(tail, x8)], (e32, E32_RECORDED[(tail, x8)])     # the yardstick itself has not drifted
    d_gate = SAFETY * e32
    out16 = _run16(sib, tail, y, sc, prm)
    assert not np.isnan(out16).any(), "%d outputs left unwritten" % int(np.isnan(out16).sum())
    err = np.abs(out16.astype(np.float64) - np.maximum(ref, 0.0))
    round16 = H16 * np.abs(ref) + H16_ABS
    bound = round16 + ARITH * U * (np.abs(y64) + np.abs(sc64)) + np.abs(y64) * d_gate
    e16 = (np.maximum(err - round16, 0.0)[sel] / np.abs(y64)[sel]).max()
    print("siblings_f16 %-3s %2dx%2dx%-3d n=%d %s  e32 %.3e  e16 %.3e  worst err/bound %.3f  max|err| %.3e" %
          (tail, H, W, C, n, "x8" if x8 else "x1", e32, e16, (err / bound).max(), err.max()))
    worst = np.unravel_index(np.argmax(err / bound), err.shape)
    assert (err <= bound).all(), (worst, err[worst], bound[worst], e32)
    gates_spread = np.abs(out32 - sc64)[sel] / np.abs(y64)[sel]         # ~ the gate where the ReLU is open
    if x8:
        assert (gates_spread < 0.2).any() and (gates_spread > 0.8).any()     # the x8 weights do reach both ends


@gpu
@pytest.mark.parametrize("tail", ["ta", "ema"])
@pytest.mark.parametrize("geom", GEOMS, ids=["%dx%dx%d" % g for g in GEOMS])
def test_f16_tail_does_not_depend_on_the_batch(sib, tail, geom):
    H, W, C = geom
    y3, sc3, prm, _ = _case(tail, H, W, C, 3, False)
    y1, sc1, prm1, _ = _case(tail, H, W, C, 1, False)
    assert np.array_equal(y3[:1], y1) and np.array_equal(prm, prm1)
    o3, o1 = _run16(sib, tail, y3, sc3, prm), _run16(sib, tail, y1, sc1, prm)
    assert np.array_equal(o3[:1].view(np.uint16), o1.view(np.uint16))
    assert not np.array_equal(o3[1].view(np.uint16), o3[0].view(np.uint16))


# ----------------------------------------------------------------------------- end to end
def _model(name, sd_fn, precision):
    from reid_amd.models import build_model
    model = build_model(name, num_classes=751, loss="triplet", pretrained=False, use_gpu=True, precision=precision)
    model.load_state_dict(sd_fn(0), strict=True)
    return model


@gpu
@pytest.mark.parametrize("tag,name,sd_fn", [("ca", "cares18_ibn", synth.cares18_state_dict), ("ema", "emares18_ibn", synth.emares18_state_dict)])
def test_sibling_f16_mode_end_to_end(eng, golden_dir, tag, name, sd_fn):
    import torch
    from oracle import seres18
    g = np.load(os.path.join(golden_dir, "siblings.npz"))
    x = seres18.preprocess_u8(synth.smooth_crops_u8(3, 7)).numpy()
    m0 = _model(name, sd_fn, 0)
    before = m0(x)                                                       # mode 0, before anything ran in mode 1
    model = _model(name, sd_fn, 1)
    assert model.precision == "f16"
    eng.debug_keep(1)
    try:
        emb, logits = model(x, return_logits=True)
        for i, blk in enumerate(b[0] for b in synth.SERES18_BLOCKS):
            c, (h, w) = BLOCK_C[i], BLOCK_HW[i]
            tap = eng.debug_stage(2 + i, 3)
            assert np.array_equal(tap.astype(np.float16).astype(np.float32), tap), blk       # (a) the taps are f16 values
            t = torch.from_numpy(tap.reshape(3, h, w, c)).permute(0, 3, 1, 2)
            got = t[:, :: max(1, c // 8), :: max(1, h // 8), :: max(1, w // 4)].numpy()
            ref = g["%s_tap_%s" % (tag, blk)]
            rel = np.abs(got - ref).max() / np.abs(ref).max()
            print("siblings_f16 e2e %s tap %s rel max err %.3e" % (name, blk, rel))
            assert rel < 1e-2, (blk, rel)
    finally:
        eng.debug_keep(0)
    ref_emb = g[tag + "_emb"]
    cos = (emb * ref_emb).sum(1) / np.linalg.norm(emb, axis=1) / np.linalg.norm(ref_emb, axis=1)
    print("siblings_f16 e2e %s 1 - cos %.3e" % (name, (1 - cos).max()))
    assert (1 - cos).max() < 1e-4                                        # (b)
    assert np.abs(emb - ref_emb).max() / np.abs(ref_emb).max() < 1e-2
    assert np.abs(logits - g[tag + "_logits"]).max() / np.abs(g[tag + "_logits"]).max() < 1e-2
    # the production kernels of a large pass - fused stem, the per-image layer-1 convolutions without SE statistics - on the same crops
    eng.debug_keep(2)
    try:
        emb2 = model(x)
        for i, blk in enumerate(b[0] for b in synth.SERES18_BLOCKS):
            c, (h, w) = BLOCK_C[i], BLOCK_HW[i]
            t = torch.from_numpy(eng.debug_stage(2 + i, 3).reshape(3, h, w, c)).permute(0, 3, 1, 2)
            got = t[:, :: max(1, c // 8), :: max(1, h // 8), :: max(1, w // 4)].numpy()
            ref = g["%s_tap_%s" % (tag, blk)]
            assert np.abs(got - ref).max() / np.abs(ref).max() < 1e-2, blk
    finally:
        eng.debug_keep(0)
    cos2 = (emb2 * ref_emb).sum(1) / np.linalg.norm(emb2, axis=1) / np.linalg.norm(ref_emb, axis=1)
    print("siblings_f16 e2e %s 1 - cos %.3e (production kernels)" % (name, (1 - cos2).max()))
    assert (1 - cos2).max() < 1e-4
    e1 = model(x[:1])                                                    # (c)
    np.testing.assert_allclose(e1, emb[:1], rtol=0, atol=2e-3 * np.abs(emb).max())
    eng.set_precision(0)                                                 # (d) mode 1 leaves nothing behind
    after = m0(x)
    assert np.array_equal(before.view(np.uint32), after.view(np.uint32))
    assert not np.array_equal(before, emb)                               # ... and mode 1 was another path


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from reid_amd import _ffi, synth
from reid_amd.models import build_model
assert _ffi.LIB_PATH.startswith(sys.argv[1]), _ffi.LIB_PATH
model = build_model("cares18_ibn", num_classes=751, loss="triplet", pretrained=False, use_gpu=True, precision=1)
model.load_state_dict(synth.cares18_state_dict(0), strict=True)
x = np.zeros((1, 3, 256, 128), np.float32)
try:
    model(x)
except _ffi.ReidHipError as e:
    print("RAISED", e)
    sys.exit(0 if "libreid_hip_siblings_f16.so" in str(e) else 3)
sys.exit(4)
"""


@gpu
def test_missing_library_is_an_error_of_the_mode1_embed(tmp_path):
    """A copy of the package without libreid_hip_siblings_f16.so, in a fresh child process: the mode-1 embed of a sibling returns
    REID_ERR_STATE naming the library before anything is launched; there is no fp32 fall back."""
    shutil.copytree(os.path.join(ROOT, "reid_amd"), tmp_path / "reid_amd", ignore=shutil.ignore_patterns("__pycache__"))
    shutil.copytree(PKG, tmp_path / "real-time-reid-tracking_amd", ignore=shutil.ignore_patterns("__pycache__", "csrc", SIB_LIB))
    assert not (tmp_path / "real-time-reid-tracking_amd" / SIB_LIB).exists()
    env = dict(os.environ)
    r = subprocess.run([sys.executable, "-c", _CHILD, str(tmp_path)], capture_output=True, text=True, timeout=300, cwd=str(tmp_path), env=env)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "RAISED" in r.stdout and SIB_LIB in r.stdout
