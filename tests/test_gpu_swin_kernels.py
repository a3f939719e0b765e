"""The Swin v1 kernels that are not GEMMs, and the trunk's geometric convolutions, each against a float64 oracle (debug harnesses
reid_debug_window_attn, _layernorm, _ln_linear, _swin_sfe, _swin_tail, _swin_merge, _swin_fuse; csrc/swin.hip, csrc/two_linear_f16.hip).

Every call goes through the function the forward calls (launch_window_attn, launch_layernorm<...>, launch_ln_linear, launch_sfe_norm_fc,
launch_swin_tail, swin_merge, swin_fuse), so each case sees the forward's kernel choice, grid, row stride and weight repacking.  Outputs a
launch leaves alone read as NaN (0xffff): check() refuses them.  Run on an MI355X: pytest -m gpu tests/test_gpu_swin_kernels.py.

Error model: u = 2^-24 (fp32 unit roundoff); an f16 result carries 2^-11 relative (2^-25 absolute below f16's normal range); a packed pair
[yh | yl'] reconstructs its fp32 value to 2^-22 |y| + 2^-36; a three-product split contraction drops 3 2^-22 per product (E_SPLIT of
test_gpu_conv.py) plus 2^-36 per operand below f16's normal range.  SAFETY = 2 (chosen) multiplies every derived bound.  No constant is
fitted to observed errors; the "recorded" ratios below are a record of one MI355X run.

Window attention, per output element o_d = sum_j p_j v_jd of a query, A_d = sum_j p_j |v_jd|, x_j = max_j s_j - s_j.
  score   delta_j = (32 + C_DOT) u scale sum|q||k_j| + C_ADD u (|s_j| + |bias_j|): a 32-term fp32 accumulation in any order (the VALU
          kernel's fmaf chain, 16 chained v_mfma_f32_32x32x2_f32, two v_mfma_f32_32x32x16_f16 on exact f16 products); C_DOT = 2 (the fp32
          rounding of the constant 32^-0.5 and of the product with it), C_ADD = 1 (the sum with the bias).  The split kernel adds
          E_SPLIT scale sum|q||k_j| + 2^-36 scale (sum|q| + sum|k_j|) and C_DOT = 2 + 3 (its correction accumulator and the fmaf that folds it).
  softmax a score error moves every p_j by at most 2 max_j delta_j relative.  exp: term j carries E_j = 4u + u x_j for expf (4u chosen for
          ocml's expf; u x_j is the rounding of s_j - max carried through the exponent), and for softmax_scores<true> E_j = E_EXP + log2e u
          x_j with E_EXP = 2^-22, the v_exp_f32 model of tests/test_gpu_tail.py (test_trans_accuracy measures it on the device).  The term
          enters o_d as sum_j p_j |v_jd| E_j; through the denominator it enters as A_d sum_j p_j E_j <= A_d (4 + 6) u (sum_j p_j x_j is at
          most the entropy, ln 49 < 4, times log2e).  The denominator's sum (48 sequential adds, or 31 + 1 across the lane pair), its
          reciprocal (2u, chosen) and the product p_j = e_j / den (1u) add 51u: C_DEN = 51 + 10 = 61.  P.V: 49 fmaf (VALU) or 64
          accumulated products (matrix cores, padded keys are zero): C_PV = 64 covers both.  A score that underflows (x_j > 87) leaves
          2^-126 |v_jd| at most.
          bound = (2 max_j delta_j + (C_PV + C_DEN) u) A_d + sum_j p_j |v_jd| E_j + 2^-126 sum_j |v_jd|
  forms   2 / 3 (f16 in, f16 out): the oracle runs on the f16-rounded qkv; + 2^-11 |o| + 2^-25.  Form 3 rounds P to f16: + 2^-11 A_d +
          2^-25 sum_j |v_jd| (probabilities below f16's normal range).  Forms 1 / 4 (packed out): + 2^-22 |o| + 2^-36.  Form 4's P.V:
          + E_SPLIT A_d + 2^-36 (sum_j |v_jd| + 1).
  recorded (one MI355X run, worst error / bound over the eight cases; every line is in profiles/swin_v1_kernels_gpu_tests.log):
          valu_f32 0.017, valu_packed 0.017, valu_f16 0.46, mfma_f16 0.39, mfma_split 0.014, mfma_f32 0.017 (the f16 forms sit at half
          their bound because the output's own rounding, 2^-11 |o| of a SAFETY 2^-10 |o|, is most of it).

LayerNorm (two-pass).  The mean and the centred sum of squares are summed in a tree of depth D = 2 (the in-lane quad (x + y) + (z + w)) +
chunks per lane + log2(lanes per token): 2 + 1 + 5 = 8 at c = 96, 2 + 3 + 6 = 11 above (layernorm_v4_kernel); 2 + c / 8 + 1 in
ln_linear_f16x3_kernel's prologue; 1 + 6 = 7 in the tail (a channel pair per lane, a wave per token).
  d_mean = D u sum|x| / c + u |mean|;  sum (x - mean')^2 / c = var + d_mean^2 exactly, the roundings of x - mean', its square and the tree add
  (D + 3) u (var + d_mean^2), the division and the eps 2u (var + eps): rel(rstd) = d_var / (2 (var + eps)) + 2u (sqrtf, reciprocal).
  y = (x - mean') rstd g + b:  |g| rstd (d_mean + u |x - mean|) + |(x - mean) rstd g| (rel(rstd) + 2u) + u (|(x - mean) rstd g| + |b|).
  A constant row (var 0) has rstd = 1 / sqrt(eps): the d_mean term is what it may show.  f16 out adds 2^-11 |y| + 2^-25, packed out
  2^-22 |y| + 2^-36; f16 = round(fp32 result) and the packed pair reconstructs the fp32 result to its own bound.

ln_linear.  The LayerNorm error e_i pushed through sum_i e_i |w_ni|, plus (E_SPLIT + K u) sum_i |LN(x)_i| |w_ni| + 2^-36 sum_i |w_ni| for the
split contraction (K = c) and 4u (|out| + |bias|) for the epilogue.

SFE.  ab: sums in double (a thread's hw / 256 terms, 6 shuffles, 3 adds: depth DD), var = s2 / hw - mean^2 in double, one fp32 rounding
each: rel(a) = u + d_var / (2 (var + eps)), d_var = (DD + 3) 2^-53 (E[v^2] + mean^2); b = beta - mean a: u |b| + |mean| |a| d_var / (2 (var
+ eps)) + |a| DD 2^-53 |mean|.  Tokens: in = relu(c1 a + b) is off by 2u (|c1 a| + |b|) + |c1| d_a + d_b (the input-affine term); then
the convolution model of test_gpu_conv.py twice with K = 48: e_mid = K u sum|w2||in| + 4u (|mid| + |b2|) + sum|w2| e_in, and the same
for the Linear.

Tail.  LN(96, eps 1e-6) with D = 7; z = max(y, 1e-6) (1-Lipschitz); term t = z^p with E_term = 2u for p == 3 (z z z), else E_EXP + ln2 (|p|
E_LOG max(|log2 z|, 1) + u |p log2 z|) (tests/test_gpu_tail.py); |d_t| <= (z + e_y)^p - z^p + E_term t (p >= 1: convex).  The sum over the
tokens of positive terms: (ntok / 64 + 1 + 3 + 16 + 1) u relative (a wave's share of a slice, four waves, sixteen slices, the division).
g = m^(1/p): rel(g) = rel(m) / p + |ln m| u / p + 4u (powf, chosen); emb: |bn_s| g rel(g) + 2u (|g bn_s| + |bn_t|).

Merge / fuse.  test_gpu_conv.bound's model on the loaded checkpoint's own tensors: K u A + 4u (|acc| + |bias| + |res|); mode 2 adds E_SPLIT A +
2^-36 sum|w|; mode 1 (f16 x and w) 2 2^-11 A + 2^-25 sum|w|, and 2^-11 |v| + 2^-25 where the output map is f16.  Each fusion step is checked
against the oracle applied to the kernel's own previous map.

Recorded on one MI355X (worst error / bound; a record, not the source of any constant): LayerNorm fp32 0.12-0.21, f16 0.50, packed
0.13-0.21; ln_linear 0.025 (c = 96), 0.010 (c = 192); SFE ab 0.39-0.45 (the mean-100 channel: one fp32 rounding of a ~ 95 and b ~ -9500),
tokens 0.010; tail gem 0.013-0.035, emb 0.019-0.043 (p = 3: 0.031 / 0.043 at 199 tokens); merge mode 0 0.007, mode 1 0.061, mode 2 0.005;
fuse mode 0 0.004, mode 1 0.12 (a0) / 0.06, mode 2 0.003; the forward with the default exponent 1.0e-7 / 2.0e-4 / 1.6e-7 of max |ref| in
modes 0 / 1 / 2.  The worst-case bounds are far above what random rounding gives; the mutation tests show what still leaves them.

Found while this module was written: swin_tail_partial_kernel clamped with fmaxf(y, 1e-6), which returns 1e-6 for a NaN, so a token
that reaches the tail non-finite (a NaN or an inf in it makes its LayerNorm NaN) left as a finite 1e-6 term and no fault was raised;
torch's clamp keeps the NaN.  The kernel now clamps with a comparison (same result for every finite value);
test_tail_nonfinite_embedding_faults holds it.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from reid_amd import _ffi, synth, weights

gpu = pytest.mark.gpu

U = 2.0 ** -24
H16 = 2.0 ** -11            # f16 half-ulp, relative
H16_ABS = 2.0 ** -25        # ... and below f16's normal range
PK_REL, PK_ABS = 2.0 ** -22, 2.0 ** -36   # a packed pair [yh | yl'] against its fp32 value
E_SPLIT = 3 * 2.0 ** -22    # test_gpu_conv.py
ABS_X = 2.0 ** -36
E_LOG = E_EXP = 2.0 ** -22  # tests/test_gpu_tail.py (test_trans_accuracy measures the composite)
LOG2E = 1.4426950408889634
SAFETY = 2.0                # chosen
C_DOT, C_ADD, C_DEN, C_PV = 2, 1, 61, 64
TINY = 2.0 ** -126
SCALE = 32.0 ** -0.5

A_F32, A_PACK, A_F16, A_MFMA16, A_SPLIT, A_MFMA32 = range(6)
ATTN_NAMES = ["valu_f32", "valu_packed", "valu_f16", "mfma_f16", "mfma_split", "mfma_f32"]
LN_F32, LN_F16, LN_PACK = range(3)


def f16r(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def unpack16(o16, c):
    f = o16.view(np.float16)
    return f[:, :c].astype(np.float64) + f[:, c:].astype(np.float64) / 2048.0


def check(got, want, bound, what):
    got = np.asarray(got, np.float64).reshape(want.shape)
    assert np.isfinite(got).all(), "%s: %d unwritten / non-finite outputs" % (what, int((~np.isfinite(got)).sum()))
    err = np.abs(got - want)
    ratio = err / np.maximum(bound, 1e-300)
    i = int(np.argmax(ratio))
    print("\n%s: max |err| %.3e, worst err/bound %.4f over %d elements" % (what, err.max(), ratio.flat[i], err.size))
    assert ratio.flat[i] <= 1.0, "%s: element %d is %.3e off, bound %.3e" % (what, i, err.flat[i], bound.flat[i])
    return float(ratio.flat[i])


# ----------------------------------------------------------------------------- window attention: inputs
# (n, H, W, heads): one window that is last row and last column, 3 tasks (ragged last block), ldq 320 != 288; all four mask classes in both
# orders of H != W; 24 heads on one window
ATTN_GEOMS = [(1, 7, 7, 3), (1, 14, 21, 3), (2, 21, 14, 6), (1, 7, 7, 24)]
Q_ZERO, Q_WIDE, Q_MASKED = 5, 11, 0      # window positions of the special queries (window (0, 0) / the last window)


def _to_windows(t, n, H, W, heads):      # [n, H, W, heads 32] in window space -> [n, nh, nw, heads, 49, 32]
    nh, nw = H // 7, W // 7
    return t.reshape(n, nh, 7, nw, 7, heads, 32).transpose(0, 1, 3, 5, 2, 4, 6).reshape(n, nh, nw, heads, 49, 32)


def _from_windows(t, n, H, W, heads):
    nh, nw = H // 7, W // 7
    return t.reshape(n, nh, nw, heads, 7, 7, 32).transpose(0, 1, 4, 2, 5, 3, 6).reshape(n, H, W, heads * 32)


@functools.lru_cache(maxsize=None)
def attn_inputs(geom, shifted):
    """(qkv fp32 [n, H, W, 3C], pos fp32 [13, 13], copies): q, k, v ~ N(0, 1.5), an asymmetric table ~ N(0, 1.5); built in window space (what
    the kernel sees after the shift) and rolled back.  copies: (dst, src) window indices (img, wy, wx) holding identical q, k, v."""
    n, H, W, heads = geom
    nh, nw = H // 7, W // 7
    C = heads * 32
    rng = np.random.default_rng(1000 + 10 * ATTN_GEOMS.index(geom) + shifted)
    qkv = rng.normal(0.0, 1.5, (3, n, nh, nw, heads, 49, 32))
    pos = rng.normal(0.0, 1.5, (13, 13)).astype(np.float32)
    q, k, v = qkv
    q[0, 0, 0, :, Q_ZERO] = 0.0                                   # an all-zero query: its scores are the bias alone
    q[0, 0, 0, :, Q_WIDE] *= 12.0                                 # scores spanning > 100: some exponentials underflow
    lw = (n - 1, nh - 1, nw - 1)                                  # the last window: both masks when shifted
    far = np.arange(49) // 7 >= 4                                 # keys the last-row mask takes from query 0
    k[lw][:, far] = 2.0 * q[lw][:, Q_MASKED][:, None, :]          # ... which would otherwise carry most of the weight
    cls = lambda wy, wx: (bool(shifted) and wy == nh - 1, bool(shifted) and wx == nw - 1)
    copies = []
    wins = [(i, wy, wx) for i in range(n) for wy in range(nh) for wx in range(nw)]
    for dst in wins:
        if dst == (0, 0, 0) or dst == lw:
            continue
        src = next((s for s in wins if s < dst and cls(s[1], s[2]) == cls(dst[1], dst[2]) and s not in [c[0] for c in copies]), None)
        if src is not None and len(copies) < 4:
            for t in (q, k, v):
                t[dst] = t[src]
            copies.append((dst, src))
    ws = np.concatenate([_from_windows(t, n, H, W, heads) for t in (q, k, v)], -1).astype(np.float32)
    if shifted:
        ws = np.roll(ws, (3, 3), (1, 2))                           # window position (y', x') is token ((y' + 3) % H, (x' + 3) % W)
    assert ws.shape == (n, H, W, 3 * C)
    return np.ascontiguousarray(ws), pos, tuple(copies)


# ----------------------------------------------------------------------------- window attention: float64 oracle
def attn_oracle(qkv, pos, shifted, heads, mutate=None):
    """WindowAttention v1 (swin_transformer.py:191-232) between to_qkv and to_out, in float64: roll(-3, -3), 7 x 7 windows, 32^-0.5, the
    relative-position bias, synth._swin_mask on the last window row / column, softmax, P.V, roll back.  Returns (o [n, H, W, C], parts) with
    parts = the float64 pieces the bound is made of.  mutate: one deliberate error (test_attention_mutations_exceed_the_bound)."""
    x = np.asarray(qkv, np.float64)
    n, H, W, c3 = x.shape
    C = c3 // 3
    nh, nw = H // 7, W // 7
    sh = 3 if mutate == "shift" else -3
    if shifted:
        x = np.roll(x, (sh, sh), (1, 2))
    q, k, v = (_to_windows(x[..., i * C:(i + 1) * C], n, H, W, heads) for i in range(3))
    idx = np.arange(49)
    iy, ix = idx // 7, idx % 7
    p64 = np.asarray(pos, np.float64).reshape(13, 13)
    if mutate == "bias_transposed":
        bias = p64[iy[:, None] - iy[None, :] + 6, ix[:, None] - ix[None, :] + 6]
    else:
        bias = p64[iy[None, :] - iy[:, None] + 6, ix[None, :] - ix[:, None] + 6]          # [query i][key j]: key - query + 6
    dots = np.einsum("...id,...jd->...ij", q, k)
    absdots = np.einsum("...id,...jd->...ij", np.abs(q), np.abs(k))
    s = dots * SCALE + bias
    if shifted:
        ul, lr = synth._swin_mask(7, 3, True).astype(np.float64), synth._swin_mask(7, 3, False).astype(np.float64)
        if mutate == "mask_at_3":
            hi_r, hi_c = iy >= 3, ix >= 3
            ul = np.where(np.not_equal.outer(hi_r, hi_r), -np.inf, 0.0)
            lr = np.where(np.not_equal.outer(hi_c, hi_c), -np.inf, 0.0)
        if mutate == "masks_swapped":
            ul, lr = lr, ul
        s[:, nh - 1] += ul
        s[:, :, nw - 1] += lr
    mx = s.max(-1, keepdims=True)
    e = np.exp(s - mx)
    p = e / e.sum(-1, keepdims=True)
    o = p @ v
    back = lambda t: np.roll(_from_windows(t, n, H, W, heads), (-sh, -sh), (1, 2)) if shifted else _from_windows(t, n, H, W, heads)
    xgap = np.where(np.isfinite(s), mx - s, 0.0)
    parts = dict(p=p, v=v, q=q, k=k, s=np.where(np.isfinite(s), s, 0.0), absdots=absdots, bias=np.broadcast_to(np.abs(bias), s.shape), xgap=xgap,
                 o=o, back=back, span=float((mx - np.where(np.isfinite(s), s, np.inf).min(-1, keepdims=True)).max()))
    return back(o), parts


def attn_bound(parts, form):
    """The module docstring's bound for kernel `form`, [n, H, W, C] float64, SAFETY included."""
    p, v, o = parts["p"], parts["v"], parts["o"]
    fast = form == A_MFMA16
    split = form == A_SPLIT
    c_dot = C_DOT + (3 if split else 0)
    delta = (32 + c_dot) * U * SCALE * parts["absdots"] + C_ADD * U * (np.abs(parts["s"]) + parts["bias"])
    if split:
        sq, sk = np.abs(parts["q"]).sum(-1), np.abs(parts["k"]).sum(-1)
        delta = delta + E_SPLIT * SCALE * parts["absdots"] + ABS_X * SCALE * (sq[..., :, None] + sk[..., None, :])
    dmax = np.where(p > 0, delta, 0.0).max(-1)                                  # over the keys the query sees
    A = p @ np.abs(v)
    Ej = (E_EXP + LOG2E * U * parts["xgap"]) if fast else (4 * U + U * parts["xgap"])
    sv = np.abs(v).sum(-2)[..., None, :]                                        # sum_j |v_jd|
    b = (2 * dmax[..., None] + (C_PV + C_DEN) * U) * A + (p * Ej) @ np.abs(v) + TINY * sv
    if form in (A_F16, A_MFMA16):
        b = b + H16 * np.abs(o) + H16_ABS
    if form == A_MFMA16:
        b = b + H16 * A + H16_ABS * sv
    if form in (A_PACK, A_SPLIT):
        b = b + PK_REL * np.abs(o) + PK_ABS
    if split:
        b = b + E_SPLIT * A + ABS_X * (sv + 1.0)
    return SAFETY * parts["back"](b)


@functools.lru_cache(maxsize=None)
def _attn_reference(geom, shifted, f16_in):
    """The oracle of a case, computed once and shared (read-only) by the tests that need it."""
    qkv, pos, _ = attn_inputs(geom, shifted)
    o, parts = attn_oracle(f16r(qkv) if f16_in else qkv, pos, shifted, geom[3])
    o.setflags(write=False)
    return o, parts


# ----------------------------------------------------------------------------- window attention: CPU tests
def test_attention_oracle_equals_the_reference_restatement():
    """attn_oracle against oracle/swin.py's _attention (itself pinned to the reference's class by tests/golden/swin_*.npz) with identity
    to_out / post_proj: qkv = x W^T is made here in float64 and handed to attn_oracle."""
    from oracle import swin
    rng = np.random.default_rng(3)
    for (n, H, W, heads), shifted in (((1, 14, 21, 3), 1), ((2, 21, 14, 6), 1), ((1, 14, 21, 3), 0)):
        C = heads * 32
        x = rng.normal(size=(n, H, W, C))
        wq = rng.normal(0, C ** -0.5 * 3, (3 * C, C))
        pre = "a"
        sd = {pre + ".to_qkv.weight": torch.from_numpy(wq), pre + ".pos_embedding": torch.from_numpy(rng.normal(0, 1.5, (13, 13))),
              pre + ".to_out.weight": torch.eye(C, dtype=torch.float64), pre + ".to_out.bias": torch.zeros(C, dtype=torch.float64),
              pre + ".post_proj.weight": torch.eye(C, dtype=torch.float64), pre + ".post_proj.bias": torch.zeros(C, dtype=torch.float64),
              pre + ".upper_lower_mask": torch.from_numpy(synth._swin_mask(7, 3, True)).double(),
              pre + ".left_right_mask": torch.from_numpy(synth._swin_mask(7, 3, False)).double()}
        want = swin._attention(sd, pre, torch.from_numpy(x), heads, bool(shifted)).numpy()
        got, _ = attn_oracle(x @ wq.T, sd[pre + ".pos_embedding"].numpy(), shifted, heads)
        np.testing.assert_allclose(got, want, rtol=1e-10, atol=1e-12)


def test_attention_inputs_hold_their_special_rows():
    for geom in ATTN_GEOMS:
        for shifted in (0, 1):
            qkv, pos, copies = attn_inputs(geom, shifted)
            n, H, W, heads = geom
            _, parts = _attn_reference(geom, shifted, False)
            assert parts["span"] > 100.0, (geom, shifted, parts["span"])
            assert np.abs(parts["q"][0, 0, 0, :, Q_ZERO]).max() == 0.0
            assert not np.allclose(pos, pos.T)
            if shifted:   # the keys the mask removes would carry most of query 0's weight in the last window
                lw = (n - 1, H // 7 - 1, W // 7 - 1)
                raw = np.roll(np.asarray(qkv, np.float64), (-3, -3), (1, 2))
                _, pr = attn_oracle(raw, pos, 0, heads)               # same windows, no mask
                far = np.arange(49) // 7 >= 4
                assert pr["p"][lw][:, Q_MASKED][:, far].sum(-1).min() > 0.5
                assert parts["p"][lw][:, Q_MASKED][:, far].sum(-1).max() == 0.0
            if n * (H // 7) * (W // 7) > 2:
                assert len(copies) >= 1


ATTN_MUTATIONS = ["bias_transposed", "mask_at_3", "shift", "masks_swapped"]


@pytest.mark.parametrize("mutation", ATTN_MUTATIONS)
def test_attention_mutations_exceed_the_bound(mutation):
    """The oracle with one deliberate error, in float64 on the test's own inputs, leaves every form's bound somewhere: the bounds are not
    vacuous.  (14 x 21 shifted holds all four mask classes.)"""
    geom, shifted = ATTN_GEOMS[1], 1
    qkv, pos, _ = attn_inputs(geom, shifted)
    for form in range(6):
        f16_in = form in (A_F16, A_MFMA16)
        want, parts = _attn_reference(geom, shifted, f16_in)
        bad, _ = attn_oracle(f16r(qkv) if f16_in else qkv, pos, shifted, geom[3], mutate=mutation)
        over = np.abs(bad - want) > attn_bound(parts, form)
        assert over.mean() > 0.01, "%s slips under the bound of form %s" % (mutation, ATTN_NAMES[form])


# ----------------------------------------------------------------------------- LayerNorm model (shared by ln_linear and the tail)
def ln_model(x, g, b, eps, depth):
    """(y, bound without SAFETY, mean, rstd) in float64 for rows x [t, c]: the two-pass model of the module docstring."""
    x = np.asarray(x, np.float64)
    g, b = np.asarray(g, np.float64), np.asarray(b, np.float64)
    c = x.shape[1]
    mean = x.mean(1, keepdims=True)
    d = x - mean
    var = (d * d).mean(1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + eps)
    y = d * rstd * g + b
    d_mean = depth * U * np.abs(x).sum(1, keepdims=True) / c + U * np.abs(mean)
    d_var = d_mean ** 2 + (depth + 3) * U * (var + d_mean ** 2) + 2 * U * (var + eps)
    rel = d_var / (2 * (var + eps)) + 2 * U
    t = np.abs(d * rstd * g)
    bound = np.abs(g) * rstd * (d_mean + U * np.abs(d)) + t * (rel + 2 * U) + U * (t + np.abs(b))
    return y, bound, mean, rstd


def ln_depth(c):            # layernorm_v4_kernel: quad, chunks per lane, log2(lanes per token)
    return 2 + 1 + 5 if c <= 128 else 2 + 3 + 6


def ln_rows(t, c, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(t, c)) * rng.uniform(0.1, 8, (t, 1)) + rng.normal(0, 3, (t, 1))
    x[7] = 2.5                                                     # constant row: variance 0 -> 1 / sqrt(eps)
    x[t - 1] = -1.25                                               # ... and as the last row of the ragged last block
    x[13] = rng.normal(size=c) * 0.5 + 500.0                       # |mean| = 1e3 std
    x[21] = 0.0
    x[21, c // 2 + 1] = 300.0                                      # one spike
    return x.astype(np.float32), rng.uniform(0.5, 1.5, c).astype(np.float32), rng.normal(0, 0.3, c).astype(np.float32)


def test_layernorm_oracle_equals_torch():
    x, g, b = ln_rows(64, 96, 5)
    y, _, _, _ = ln_model(x, g, b, 1e-5, ln_depth(96))
    want = F.layer_norm(torch.from_numpy(x).double(), (96,), torch.from_numpy(g).double(), torch.from_numpy(b).double(), 1e-5).numpy()
    np.testing.assert_allclose(y, want, rtol=1e-9, atol=1e-9)      # (the constant row: torch's var is 0 up to its own rounding)


def test_layernorm_mutation_exceeds_the_bound():
    """eps 1e-6 instead of 1e-5 shows on the constant and the small rows."""
    x, g, b = ln_rows(64, 96, 5)
    x[30] *= 1e-3 / np.abs(x[30]).max()
    y, bd, _, _ = ln_model(x, g, b, 1e-5, ln_depth(96))
    bad, _, _, _ = ln_model(x, g, b, 1e-6, ln_depth(96))
    assert (np.abs(bad - y) > SAFETY * (bd + H16 * np.abs(y) + H16_ABS)).any()


# ----------------------------------------------------------------------------- SFE oracle
def sfe_operands(n, h1, w1, seed):
    rng = np.random.default_rng(seed)
    c1 = rng.normal(0, 1, (n, h1, w1, 12)).astype(np.float32)
    c1[..., 0] = 0.75                                              # an InstanceNorm channel that is constant: variance 0
    c1[0, ..., 1] = (100.0 + 0.01 * rng.normal(size=(h1, w1))).astype(np.float32)   # mean 100, std 0.01: c1 a + b cancels five digits, which the
                                                                                    # bound of image 0's tokens carries; image 1 keeps a tight one
    in_g, in_b = rng.uniform(0.5, 1.5, 6).astype(np.float32), rng.normal(0, 0.1, 6).astype(np.float32)
    bn_s = (rng.uniform(0.5, 1.5, 6) * np.array([1, -1, 1, -1, -1, 1])).astype(np.float32)    # negative BatchNorm scales
    bn_t = rng.normal(0, 0.3, 6).astype(np.float32)
    c2_w = rng.normal(0, np.sqrt(2.0 / 48), (48, 48)).astype(np.float32)    # [co][(kh, kw, c)]
    c2_b = rng.normal(0, 0.1, 48).astype(np.float32)
    fc_w = rng.normal(0, np.sqrt(2.0 / 48), (96, 48)).astype(np.float32)
    fc_b = rng.normal(0, 0.1, 96).astype(np.float32)
    return c1, in_g, in_b, bn_s, bn_t, c2_w, c2_b, fc_w, fc_b


def sfe_oracle(c1, in_g, in_b, bn_s, bn_t, c2_w, c2_b, fc_w, fc_b, unbiased=False):
    """(ab [n, 24], its bound, tok [n, h1/2, w1/2, 96], its bound) float64, SAFETY included."""
    x = np.asarray(c1, np.float64)
    n, h1, w1, _ = x.shape
    hw = h1 * w1
    f = lambda a: np.asarray(a, np.float64)
    xi = x[..., :6].reshape(n, hw, 6)
    mean = xi.mean(1)
    var = ((xi - mean[:, None]) ** 2).mean(1) * (hw / (hw - 1.0) if unbiased else 1.0)
    ex2 = (xi * xi).mean(1)
    a_in = f(in_g) / np.sqrt(var + 1e-5)
    b_in = f(in_b) - mean * a_in
    dd = -(-hw // 256) + 6 + 3
    d_var = (dd + 3) * 2.0 ** -53 * (ex2 + mean * mean)
    relv = d_var / (2 * (var + 1e-5))
    da_in = np.abs(a_in) * (U + relv)
    db_in = U * np.abs(b_in) + np.abs(mean * a_in) * relv + np.abs(a_in) * dd * 2.0 ** -53 * np.abs(mean)
    a = np.concatenate([a_in, np.broadcast_to(f(bn_s), (n, 6))], 1)
    b = np.concatenate([b_in, np.broadcast_to(f(bn_t), (n, 6))], 1)
    da = np.concatenate([da_in, np.zeros((n, 6))], 1)
    db = np.concatenate([db_in, np.zeros((n, 6))], 1)
    ab, dab = np.concatenate([a, b], 1), np.concatenate([da, db], 1)
    aa, bb, daa, dbb = (t[:, None, None, :] for t in (a, b, da, db))
    vin = np.maximum(x * aa + bb, 0.0)
    e_in = 2 * U * (np.abs(x * aa) + np.abs(bb)) + np.abs(x) * daa + dbb
    patch = lambda t: t.reshape(n, h1 // 2, 2, w1 // 2, 2, 12).transpose(0, 1, 3, 2, 4, 5).reshape(n, h1 // 2, w1 // 2, 48)   # (kh, kw, c)
    pin, pe = patch(vin), patch(e_in)
    w2, wf = f(c2_w), f(fc_w)
    pre = pin @ w2.T + f(c2_b)
    mid = np.maximum(pre, 0.0)
    e_mid = 48 * U * (pin @ np.abs(w2).T) + 4 * U * (np.abs(pre) + np.abs(f(c2_b))) + pe @ np.abs(w2).T
    tok = mid @ wf.T + f(fc_b)
    e_tok = 48 * U * (mid @ np.abs(wf).T) + 4 * U * (np.abs(tok) + np.abs(f(fc_b))) + e_mid @ np.abs(wf).T
    return ab, SAFETY * dab, tok, SAFETY * e_tok


def test_sfe_oracle_equals_torch_and_its_mutation_exceeds_the_bound():
    """sfe_oracle against torch's instance_norm / conv2d / linear in float64 (the ops of oracle/swin.py's forward); an unbiased InstanceNorm
    variance leaves the bound."""
    ops = sfe_operands(2, 14, 14, 11)
    c1, in_g, in_b, bn_s, bn_t, c2_w, c2_b, fc_w, fc_b = ops
    ab, dab, tok, dtok = sfe_oracle(*ops)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    x = t(c1).permute(0, 3, 1, 2)
    a = F.instance_norm(x[:, :6].contiguous(), None, None, t(in_g), t(in_b), True, 0.0, 1e-5)
    bb = x[:, 6:] * t(bn_s)[None, :, None, None] + t(bn_t)[None, :, None, None]
    y = F.relu(torch.cat((a, bb), 1))
    w2 = t(c2_w).reshape(48, 2, 2, 12).permute(0, 3, 1, 2).contiguous()          # (kh, kw, c) -> torch's (c, kh, kw)
    y = F.relu(F.conv2d(y, w2, t(c2_b), stride=2))
    want = F.linear(y.permute(0, 2, 3, 1), t(fc_w), t(fc_b)).numpy()
    np.testing.assert_allclose(tok, want, rtol=1e-6, atol=1e-6)
    bad_ab, _, bad_tok, _ = sfe_oracle(*ops, unbiased=True)
    assert (np.abs(bad_ab - ab) > dab).any() and (np.abs(bad_tok - tok) > dtok).any()


# ----------------------------------------------------------------------------- tail oracle
def tail_operands(n, ntok, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, ntok, 96)) * rng.uniform(0.2, 3, (n, ntok, 1)) + rng.normal(0, 1, (n, ntok, 1))
    x[n - 1, ntok // 3] *= 400.0                                   # one token of large norm
    g = rng.uniform(0.5, 1.5, 96).astype(np.float32)
    b = rng.normal(0, 0.1, 96).astype(np.float32)                  # LN outputs centred near 0: about half fall below the clamp
    g[5], b[5] = 0.5, -6.0                                         # a channel whose every token is clamped (|LN| <= sqrt(95)): gem = 1e-6
    bn_s = (rng.uniform(0.5, 1.5, 96) * rng.choice([-1.0, 1.0], 96)).astype(np.float32)
    bn_t = rng.normal(0, 0.3, 96).astype(np.float32)
    return x.astype(np.float32), g, b, bn_s, bn_t


def tail_oracle(x, g, b, p, bn_s, bn_t, mutate=None):
    """(gem [n, 96], its bound, emb, its bound, fraction of clamped LN outputs) float64, SAFETY included."""
    x = np.asarray(x, np.float64)
    n, ntok, c = x.shape
    p = float(np.float32(p))
    y, e_y, _, _ = ln_model(x.reshape(-1, c), g, b, 1e-5 if mutate == "eps" else 1e-6, 7)
    if mutate == "clamp_after":
        t = np.maximum(np.sign(y) * np.abs(y) ** p if p == 3.0 else np.where(y > 0, np.abs(y) ** p, 0.0), 1e-6)
        z = np.maximum(y, 1e-6)
    else:
        z = np.maximum(y, 1e-6)
        t = z ** p
    l2 = np.abs(np.log2(z))
    e_term = 2 * U if p == 3.0 else E_EXP + np.log(2) * (abs(p) * E_LOG * np.maximum(l2, 1.0) + U * abs(p) * l2)
    d_t = (z + e_y) ** p - z ** p + e_term * t
    t, d_t = t.reshape(n, ntok, c), d_t.reshape(n, ntok, c)
    m = t.mean(1)
    rel_m = d_t.mean(1) / m + (ntok / 64.0 + 1 + 3 + 16 + 1) * U
    gem = m ** (1.0 / p)
    rel_g = rel_m / p + np.abs(np.log(m)) * U / p + 4 * U
    s, sh = np.asarray(bn_s, np.float64), np.asarray(bn_t, np.float64)
    emb = gem * s + sh
    d_emb = np.abs(s) * gem * rel_g + 2 * U * (np.abs(gem * s) + np.abs(sh))
    return gem, SAFETY * gem * rel_g, emb, SAFETY * d_emb, float((y < 1e-6).mean())


def test_tail_oracle_equals_torch_and_its_mutations_exceed_the_bound():
    x, g, b, bn_s, bn_t = tail_operands(3, 199, 21)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    for p in (3.0, 2.5):
        gem, dg, emb, de, clamped = tail_oracle(x, g, b, p, bn_s, bn_t)
        assert 0.3 < clamped < 0.7
        tok = F.layer_norm(t(x), (96,), t(g), t(b), 1e-6)
        want = tok.clamp(min=1e-6).pow(p).mean(dim=1).pow(1.0 / p).numpy()          # oracle/swin.py:113-115
        np.testing.assert_allclose(gem, want, rtol=1e-10)
        for mutation in ("clamp_after", "eps"):
            bad = tail_oracle(x, g, b, p, bn_s, bn_t, mutate=mutation)
            assert (np.abs(bad[0] - gem) > dg).any(), (p, mutation)


# ----------------------------------------------------------------------------- merge / fuse oracles
def conv_bound(acc, A, wsum, k, mode, bias, res=None, f16_out=False):
    """test_gpu_conv.bound's model for an NHWC result acc [..., cout]: A = the same operation on absolute values, wsum = sum|w| per output
    channel, K = k accumulated products; SAFETY included."""
    mul = k * U + (E_SPLIT if mode == 2 else 0.0) + (2 * H16 if mode == 1 else 0.0)
    absx = ABS_X if mode == 2 else (H16_ABS if mode == 1 else 0.0)
    v = acc if res is None else acc + res
    b = mul * A + absx * wsum + 4 * U * (np.abs(acc) + np.abs(bias) + (0.0 if res is None else np.abs(res)))
    if f16_out:
        b = b + H16 * np.abs(v) + H16_ABS
    return SAFETY * b


def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64))).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def merge_oracle(sd, stage, x, mutate=None):
    """Patch merging in front of `stage` as a float64 conv2d from the state dict's own Linear weight ([C][(c, kh, kw)], nn.Unfold order)."""
    w = torch.from_numpy(np.asarray(sd["stage%d.patch_partition.linear.weight" % stage], np.float64))
    bias = np.asarray(sd["stage%d.patch_partition.linear.bias" % stage], np.float64)
    cout, cin = w.shape[0], w.shape[1] // 4
    w4 = w.reshape(cout, 2, 2, cin).permute(0, 3, 1, 2).contiguous() if mutate == "khkwc" else w.reshape(cout, cin, 2, 2)
    acc = _nhwc(F.conv2d(_nchw(x), w4, None, stride=2))
    A = _nhwc(F.conv2d(_nchw(np.abs(x)), w4.abs(), None, stride=2))
    return acc + bias, acc, A, w4.abs().sum((1, 2, 3)).numpy(), bias, 4 * cin


def align_oracle(sd, sfe):
    w = torch.from_numpy(np.asarray(sd["img_channel_align.weight"], np.float64))
    bias = np.asarray(sd["img_channel_align.bias"], np.float64)
    acc = _nhwc(F.conv2d(_nchw(sfe), w, None, stride=8))
    A = _nhwc(F.conv2d(_nchw(np.abs(sfe)), w.abs(), None, stride=8))
    return acc + bias, A, w.abs().sum((1, 2, 3)).numpy(), bias, 64 * 96


def convt_oracle(sd, name, x, mutate=None):
    """ConvTranspose2d(4, 2, 1) in float64 from the state dict's [ci][co][4][4] weight.  mutate: "parity" swaps the (py, px) output parities,
    "pad" puts the even output rows' padding on the other side (they move by one input row)."""
    w = torch.from_numpy(np.asarray(sd[name + ".weight"], np.float64))
    bias = np.asarray(sd[name + ".bias"], np.float64)
    acc = _nhwc(F.conv_transpose2d(_nchw(x), w, None, 2, 1))
    A = _nhwc(F.conv_transpose2d(_nchw(np.abs(x)), w.abs(), None, 2, 1))
    if mutate == "parity":
        sw = acc.copy()
        sw[:, 0::2, 1::2], sw[:, 1::2, 0::2] = acc[:, 1::2, 0::2], acc[:, 0::2, 1::2]
        acc = sw
    if mutate == "pad":
        full = _nhwc(F.conv_transpose2d(_nchw(x), w, None, 2, 0))
        acc = acc.copy()
        acc[:, 0::2] = full[:, 3::2][:, :x.shape[1], 1:-1]
    # an output element sums at most 2 x 2 taps of ci channels
    return acc + bias, A, w.abs().sum((0, 2, 3)).numpy(), bias, 4 * w.shape[0]


def fuse_maps(n, h1, w1, seed):
    """sfe and the four stage outputs, each at a scale of its own (a residual taken from the wrong stage shows)."""
    rng = np.random.default_rng(seed)
    mk = lambda s, scale: (rng.normal(size=(n, h1 >> s, w1 >> s, 96 << s)) * scale).astype(np.float32)
    return mk(0, 1.0), mk(0, 0.5), mk(1, 2.0), mk(2, 4.0), mk(3, 8.0)


def test_merge_and_fuse_oracles_equal_the_reference_restatement():
    """merge_oracle against oracle/swin.py's Unfold-order Linear; the fusion chain against its conv2d / conv_transpose2d lines (the same
    torch ops: this pins the argument order)."""
    sd = synth.swin_state_dict(0)
    rng = np.random.default_rng(2)
    x = rng.normal(size=(2, 8, 6, 96))
    n, h, w, c = x.shape
    u = torch.from_numpy(x).reshape(n, h // 2, 2, w // 2, 2, c).permute(0, 1, 3, 5, 2, 4).reshape(n, h // 2, w // 2, c * 4)   # oracle/swin.py:97
    want = F.linear(u, torch.from_numpy(sd["stage2.patch_partition.linear.weight"]).double(),
                    torch.from_numpy(sd["stage2.patch_partition.linear.bias"]).double()).numpy()
    np.testing.assert_allclose(merge_oracle(sd, 2, x)[0], want, rtol=1e-10, atol=1e-12)
    t = rng.normal(size=(1, 3, 2, 768))
    got = convt_oracle(sd, "stage4_channel_align", t)[0]
    ref = F.conv_transpose2d(_nchw(t), torch.from_numpy(sd["stage4_channel_align.weight"]).double(),
                             torch.from_numpy(sd["stage4_channel_align.bias"]).double(), 2, 1)
    np.testing.assert_allclose(got, _nhwc(ref), rtol=1e-12)


def test_merge_and_fuse_mutations_exceed_the_bound():
    sd = synth.swin_state_dict(0)
    rng = np.random.default_rng(4)
    x = rng.normal(size=(1, 8, 8, 96)).astype(np.float32)
    v, acc, A, wsum, bias, k = merge_oracle(sd, 2, x)
    bad = merge_oracle(sd, 2, x, mutate="khkwc")[0]
    assert (np.abs(bad - v) > conv_bound(acc, A, wsum, k, 1, bias)).mean() > 0.5
    t = rng.normal(size=(1, 4, 4, 768)).astype(np.float32)
    v, A, wsum, bias, k = convt_oracle(sd, "stage4_channel_align", t)
    bd = conv_bound(v - bias, A, wsum, k, 1, bias, f16_out=True)
    for mutation in ("parity", "pad"):
        bad = convt_oracle(sd, "stage4_channel_align", t, mutate=mutation)[0]
        assert (np.abs(bad - v) > bd).mean() > 0.25, mutation


# ----------------------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def eng():
    from reid_amd.engine import get_engine
    e = get_engine(0)
    e.set_precision(0)
    yield e
    e.clear_fault()
    e.set_precision(0)


@pytest.fixture(scope="module")
def swin_eng(eng):
    sd = synth.swin_state_dict(0)
    eng.load_swin(*weights.pack_swin(sd)[:2])
    return eng, sd


# ----------------------------------------------------------------------------- window attention on the device
ATTN_CASES = [(g, s) for g in ATTN_GEOMS for s in (0, 1)]
ATTN_IDS = ["n%d-%dx%d-h%d-%s" % (g + ("shifted" if s else "plain",)) for g, s in ATTN_CASES]


@gpu
@pytest.mark.parametrize("geom,shifted", ATTN_CASES, ids=ATTN_IDS)
def test_window_attention(eng, geom, shifted):
    """All six kernels on one case: each within its bound of the float64 oracle; forms 0 and 1 agree to the packed pair's own rounding;
    identical windows at different (image, wy, wx) of one mask class give bit-identical rows within a form."""
    n, H, W, heads = geom
    qkv, pos, copies = attn_inputs(geom, shifted)
    outs = {}
    for form in range(6):
        f16_in = form in (A_F16, A_MFMA16)
        want, parts = _attn_reference(geom, shifted, f16_in)
        got = eng.debug_window_attn(form, qkv, pos, shifted)
        assert eng.fault_bits() == 0
        outs[form] = got
        check(got, want, attn_bound(parts, form), "ATTN %s %s" % (ATTN_NAMES[form], ATTN_IDS[ATTN_CASES.index((geom, shifted))]))
        win = lambda t: _to_windows(np.roll(t, (-3, -3), (1, 2)) if shifted else t, n, H, W, heads)
        gw = win(np.asarray(got))
        for dst, src in copies:
            np.testing.assert_array_equal(gw[dst], gw[src], err_msg="%s: window %r vs its copy %r" % (ATTN_NAMES[form], dst, src))
    o0 = outs[A_F32].astype(np.float64)
    assert (np.abs(outs[A_PACK] - o0) <= PK_REL * np.abs(o0) + PK_ABS).all(), "packed store of the VALU kernel vs its fp32 store"


# ----------------------------------------------------------------------------- LayerNorm on the device
LN_T = 1003                 # neither 4 nor 8 divides it: a ragged last block in both block shapes


@gpu
@pytest.mark.parametrize("c", [96, 192, 384, 768])
def test_layernorm(eng, c):
    x, g, b = ln_rows(LN_T, c, 40 + c)
    y, bd, _, _ = ln_model(x, g, b, 1e-5, ln_depth(c))
    o32 = eng.debug_layernorm(LN_F32, x, g, b)
    check(o32, y, SAFETY * bd, "LN fp32 c=%d" % c)
    o16 = eng.debug_layernorm(LN_F16, x, g, b)
    assert (o16 != 0xffff).all()
    check(o16.view(np.float16).astype(np.float64), y, SAFETY * (bd + H16 * np.abs(y) + H16_ABS), "LN f16 c=%d" % c)
    pk = eng.debug_layernorm(LN_PACK, x, g, b)
    assert (pk != 0xffff).all()
    check(unpack16(pk, c), y, SAFETY * (bd + PK_REL * np.abs(y) + PK_ABS), "LN packed c=%d" % c)
    # the three forms hold one fp32 value
    np.testing.assert_array_equal(o16, o32.astype(np.float16).view(np.uint16), err_msg="f16 out != round(fp32 out)")
    o64 = o32.astype(np.float64)
    assert (np.abs(unpack16(pk, c) - o64) <= PK_REL * np.abs(o64) + PK_ABS).all(), "packed out vs fp32 out"
    assert eng.fault_bits() == 0


# ----------------------------------------------------------------------------- ln_linear on the device
@gpu
@pytest.mark.parametrize("t,c,n", [(1024 + 49, 96, 288), (784 + 16, 192, 576)])
def test_ln_linear(eng, t, c, n):
    """LayerNorm 1 + to_qkv in one kernel: rows repeated at other tile positions are bit-identical; every element within the derived bound."""
    rng = np.random.default_rng(t)
    x, g, b = ln_rows(t, c, 70 + c)
    rep = [(t - 1, 0), (t - 17, 3), (640, 3), (129, 7), (255, 13), (300, 21)]     # (dst, src): other tiles, other rows of a tile, the ragged tail
    for dst, src in rep:
        x[dst] = x[src]
    w = rng.normal(0, c ** -0.5, (n, c)).astype(np.float32)
    out = eng.debug_ln_linear(x, g, b, w)
    assert eng.fault_bits() == 0
    for dst, src in rep:
        np.testing.assert_array_equal(out[dst], out[src], err_msg="row %d vs its copy %d" % (dst, src))
    y, e_ln, _, _ = ln_model(x, g, b, 1e-5, 2 + c // 8 + 1)
    w64 = w.astype(np.float64)
    want = y @ w64.T
    bd = e_ln @ np.abs(w64).T + (E_SPLIT + c * U) * (np.abs(y) @ np.abs(w64).T) + ABS_X * np.abs(w64).sum(1) + 4 * U * np.abs(want)
    check(out, want, SAFETY * bd, "LN_LINEAR t=%d c=%d n=%d" % (t, c, n))


# ----------------------------------------------------------------------------- SFE on the device
@gpu
@pytest.mark.parametrize("h1,w1", [(14, 14), (112, 112), (224, 112)])
def test_sfe(eng, h1, w1):
    ops = sfe_operands(2, h1, w1, h1 + w1)
    ab, dab, tok, dtok = sfe_oracle(*ops)
    gab, gtok = eng.debug_swin_sfe(*ops)
    assert eng.fault_bits() == 0
    check(gab, ab, dab, "SFE ab %dx%d" % (h1, w1))
    check(gtok, tok, dtok, "SFE tokens %dx%d" % (h1, w1))


# ----------------------------------------------------------------------------- tail on the device
TAIL_CASES = [(p, ntok) for p in (3.0, 2.5, 3.5, 1.0) for ntok in (3136, 6272, 199)]


@gpu
@pytest.mark.parametrize("p,ntok", TAIL_CASES, ids=["p%g-ntok%d" % c for c in TAIL_CASES])
def test_tail(eng, p, ntok):
    ops = tail_operands(3, ntok, int(p * 10) + ntok)
    x, g, b, bn_s, bn_t = ops
    gem, dg, emb, de, clamped = tail_oracle(x, g, b, p, bn_s, bn_t)
    assert 0.3 < clamped < 0.7
    ggem, gemb = eng.debug_swin_tail(x, g, b, p, bn_s, bn_t)
    assert eng.fault_bits() == 0
    check(ggem, gem, dg, "TAIL gem p=%g ntok=%d (clamped %.2f)" % (p, ntok, clamped))
    check(gemb, emb, de, "TAIL emb p=%g ntok=%d" % (p, ntok))


@gpu
def test_tail_nonfinite_embedding_faults(eng):
    x, g, b, bn_s, bn_t = tail_operands(3, 199, 5)
    eng.debug_swin_tail(x, g, b, 3.0, bn_s, bn_t)
    assert eng.fault_bits() == 0
    bad = x.copy()
    bad[1, 77, 40] = np.nan
    with pytest.raises(_ffi.ReidHipError) as ei:
        eng.debug_swin_tail(bad, g, b, 3.0, bn_s, bn_t)
    assert ei.value.status == -3 and eng.fault_bits() == 2
    with pytest.raises(_ffi.ReidHipError):       # sticky
        eng.debug_swin_tail(x, g, b, 3.0, bn_s, bn_t)
    eng.clear_fault()
    assert eng.fault_bits() == 0
    gem, _ = eng.debug_swin_tail(x, g, b, 3.0, bn_s, bn_t)
    assert np.isfinite(gem).all()


@gpu
def test_forward_with_the_default_exponent(swin_eng):
    """A checkpoint without avgpool.p (the packer's default) and one with p = 3.0 run the cube branch: the same embeddings bit for bit, within
    the forward's bars of oracle.swin.forward in every mode."""
    from oracle import swin
    eng, sd0 = swin_eng
    sd3 = type(sd0)(sd0)
    sd3["avgpool.p"] = np.asarray([3.0], np.float32)
    sd_none = type(sd0)((k, v) for k, v in sd0.items() if k != "avgpool.p")
    x = synth.images_f32(2, 9)
    ref = swin.forward(sd3, torch.from_numpy(x))[0].numpy()
    embs = {}
    try:
        for name, sd in (("none", sd_none), ("3.0", sd3)):
            eng.set_precision(0)
            eng.load_swin(*weights.pack_swin(sd)[:2])
            for mode in (0, 1, 2):
                eng.set_precision(mode)
                embs[name, mode] = eng.swin_embed_f32_nchw(x)
    finally:
        eng.set_precision(0)
        eng.load_swin(*weights.pack_swin(sd0)[:2])      # what the module's other tests run on
    for mode in (0, 1, 2):
        np.testing.assert_array_equal(embs["none", mode], embs["3.0", mode])
        rel = np.abs(embs["3.0", mode] - ref).max() / np.abs(ref).max()
        print("\nFORWARD p=3 mode %d: max |err| / max |ref| %.3e" % (mode, rel))
        assert rel < (1e-2 if mode == 1 else 2e-4)


# ----------------------------------------------------------------------------- merge / fuse on the device (the loaded checkpoint's weights)
MERGE_SIZES = [(56, 56), (112, 56), (56, 112)]


@gpu
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_merge(swin_eng, mode):
    eng, sd = swin_eng
    eng.set_precision(mode)
    try:
        for stage in (2, 3, 4):
            for n in (1, 3):
                for h, w in MERGE_SIZES:
                    hs, ws_ = h >> (stage - 2), w >> (stage - 2)
                    x = (np.random.default_rng(stage * 100 + n + h).normal(size=(n, hs, ws_, 48 << (stage - 1))) * 1.5).astype(np.float32)
                    v, acc, A, wsum, bias, k = merge_oracle(sd, stage, x)
                    got = eng.debug_swin_merge(stage, x)
                    assert eng.fault_bits() == 0
                    check(got, v, conv_bound(acc, A, wsum, k, mode, bias), "MERGE mode %d stage %d n=%d %dx%d" % (mode, stage, n, hs, ws_))
    finally:
        eng.set_precision(0)


@gpu
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("n,h1,w1", [(1, 56, 56), (3, 56, 56), (1, 112, 56), (1, 56, 112)])
def test_fuse(swin_eng, mode, n, h1, w1):
    """a0 = x4 + Conv8x8s8(sfe), then three ConvTranspose2d(4, 2, 1) + stage outputs: every element of every map, each step against the
    oracle applied to the kernel's own previous map."""
    eng, sd = swin_eng
    sfe, x1, x2, x3, x4 = fuse_maps(n, h1, w1, n * 1000 + h1 + 2 * w1)
    eng.set_precision(mode)
    try:
        a0, f3, f2, f1 = eng.debug_swin_fuse(sfe, x1, x2, x3, x4)
    finally:
        eng.set_precision(0)
    assert eng.fault_bits() == 0
    what = "FUSE mode %d n=%d %dx%d " % (mode, n, h1, w1)
    f16 = mode == 1
    v, A, wsum, bias, k = align_oracle(sd, sfe)
    res = x4.astype(np.float64)
    check(a0, v + res, conv_bound(v - bias, A, wsum, k, mode, bias, res, f16), what + "a0")
    prev = a0
    for name, res, got, last in (("stage4_channel_align", x3, f3, False), ("stage3_channel_align", x2, f2, False),
                                 ("stage2_channel_align", x1, f1, True)):
        v, A, wsum, bias, k = convt_oracle(sd, name, prev.astype(np.float64))
        res = res.astype(np.float64)
        check(got, v + res, conv_bound(v - bias, A, wsum, k, mode, bias, res, f16 and not last), what + name)
        prev = got
