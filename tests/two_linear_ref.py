"""Float64 oracle, per-element bounds, exact operand families and the case table of the tests of the fused pair of linears
(csrc/two_linear_f16.hip, two_linear_f16x3_kernel; tests/test_two_linear_host.py on the CPU, tests/test_gpu_two_linear.py on an MI355X):
    out = res + W2 . act(W1 . [LN](x) + b1) + b2        x, res, out [T][C]; W1 [hid][C]; W2 [C][hid]; fp32-class arithmetic
in its four builds (ACT, LN) - the Swin block's to_out -> post_proj (packed [xh | xl'] input, no activation) and its MLP (LayerNorm 2 in the
prologue, GELU, and ONE buffer as x32, res and out).

Why three views.  A worst-case bound pushed through both layers (view 3) is a few hundred times what the kernel's roundings give: dropping
the low half hl' of every hidden value (2^-12 relative) or a tanh-form GELU stays under it.  So each layer is looked at through operands
that expose it, where the project's single-layer bounds apply (tests/linear_ref.py, whose terms are not restated here).

View 1, the hidden layer exposed.  W2[n, (n + off) % hid] = 1 and 0 elsewhere, off = 0, C, 2C .. < hid, so that
    out[t, n] = res + b2[n] + g[t, u],   g = act(W1 . [LN](x) + b1),   u = (n + off) % hid
shows every hidden unit in some launch, in the output column the W2 image's k position (two_linear_w2_tiles_kernel's kpos) sends it
to.  With a 0/1 W2 GEMM 2 sums hh 2^11 + hl' (22 significant bits: exact in fp32) and zeros.  Per element, before SAFETY:
    e_h  = linear_ref.bound(layer 1 as a precision-2 Linear with K = C, with or without GELU) / SAFETY
           + L (e_LN @ |W1|^T)     LN builds: ln_model's bound of the normalised row through the layer, L = GELU_LIP with GELU, else 1
                                   (depth 2 + C / 8 + 1 of token_fragments_ln, as test_ln_linear of tests/test_gpu_swin_kernels.py has it)
           + PK_REL |g| + PK_ABS   the [hh | hl'] split of the hidden value (2^-22 relative; PK_ABS = ABS_X below f16's normal range)
    e    = e_h + 4u (|g| + |b2| + |res|)          fmaf(acc 2^-11, b2) and the residual's addition
    bound = SAFETY e
View 2, layer 2 exact.  W1[j, j % C] = 1 (h_j = x[j % C]), b1 = 0, no activation, no LN; x, b2, res = integers 2^-p, W2 integers: the
output must be the float64 result bit for bit (exact_layer2, where the ranges are derived).  Its mirror for layer 1: W2 a selection
as in view 1, integer W1 and b1 (exact_layer1).  A rounding bound of layer 2 cannot see a dropped hl' under its K u A term; equality can.
View 3, both layers random: the composed worst-case bound - a SANITY bound, stated as what it is -
    SAFETY (e_h @ |W2|^T + (E_SPLIT + hid u) (|g| @ |W2|^T) + ABS_X sum_j |W2[n, j]| + 4u (|acc2| + |b2| + |res|))
and the global figure 1.5e-6 max |ref| of test_fused_pair_of_linears_matches_float64_and_is_position_invariant (tests/test_gpu_parity.py),
taken from there and not re-derived, over global_rows(): the rows as well conditioned as that test's, since no fp32 LayerNorm brings
ln_rows' |mean| = 1e3 std row there.

Constants: U, E_SPLIT, ABS_X, SAFETY of tests/test_gpu_conv.py; PK_REL, PK_ABS and ln_model / ln_rows / check of
tests/test_gpu_swin_kernels.py; GELU_LIP, AS_ERR, AS_CHAIN inside linear_ref.bound.  None is new and none is fitted to observed errors.
"""
import collections
import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import linear_ref as lref  # noqa: E402
from linear_ref import AS_CHAIN, AS_ERR, GELU_LIP, exact_operands  # noqa: E402,F401
from test_gpu_conv import ABS_X, E_SPLIT, SAFETY, U  # noqa: E402
from test_gpu_swin_kernels import PK_ABS, PK_REL, check, ln_model, ln_rows  # noqa: E402,F401

GLOBAL_TOL = 1.5e-6          # tests/test_gpu_parity.py, the present test's tolerance relative to max |ref|
LN_EPS = 1e-5
TOKENS_PER_BLOCK = 128       # launch_two_linear: four waves of 32 tokens


def ln_depth(c):
    """token_fragments_ln: a quad, c / 8 quads per lane (two float4 per 16 columns), one exchange with the partner lane"""
    return 2 + c // 8 + 1


# ----------------------------------------------------------------------------------------------------- oracle and bounds
Hidden = collections.namedtuple("Hidden", "g e_h")


def hidden(x, w1, b1, act, ln=None, eps=LN_EPS):
    """(g, e_h): the hidden layer in float64 and its error bound WITHOUT SAFETY, [T, hid] (the module docstring's e_h)."""
    c = w1.shape[1]
    w64 = np.asarray(w1, np.float64)
    if ln is None:
        y, e_ln = np.asarray(x, np.float64), None
    else:
        y, e_ln, _, _ = ln_model(x, ln[0], ln[1], eps, ln_depth(c))
    p = lref.oracle(y, w64, b1, None, act, precision=2)
    e = lref.bound(p, 2, c, act) / SAFETY
    if e_ln is not None:
        e = e + (GELU_LIP if act else 1.0) * (e_ln @ np.abs(w64).T)
    return Hidden(p.g, e + PK_REL * np.abs(p.g) + PK_ABS)


def selection_w2(c, hid, off):
    """View 1's W2 [c, hid]: output column n reads hidden unit (n + off) % hid."""
    w2 = np.zeros((c, hid), np.float32)
    w2[np.arange(c), (np.arange(c) + off) % hid] = 1.0
    return w2


def selection_offsets(c, hid):
    return list(range(0, hid, c))


def selection_w1(c, hid):
    """View 2's W1 [hid, c]: hidden unit j is x[j % c]."""
    w1 = np.zeros((hid, c), np.float32)
    w1[np.arange(hid), np.arange(hid) % c] = 1.0
    return w1


def view1(h, c, off, b2, res):
    """(want, bound) [T, c] of a launch with selection_w2(c, hid, off)."""
    u = (np.arange(c) + off) % h.g.shape[1]
    g, b2, res = h.g[:, u], np.asarray(b2, np.float64), np.asarray(res, np.float64)
    return g + b2 + res, SAFETY * (h.e_h[:, u] + 4 * U * (np.abs(g) + np.abs(b2) + np.abs(res)))


def view3(h, w2, b2, res):
    """(want, composed worst-case bound) [T, c] of a launch with a general W2."""
    w64, b2, res = np.asarray(w2, np.float64), np.asarray(b2, np.float64), np.asarray(res, np.float64)
    hid = w64.shape[1]
    acc = h.g @ w64.T
    e = h.e_h @ np.abs(w64).T + (E_SPLIT + hid * U) * (np.abs(h.g) @ np.abs(w64).T) + ABS_X * np.abs(w64).sum(1)
    return acc + b2 + res, SAFETY * (e + 4 * U * (np.abs(acc) + np.abs(b2) + np.abs(res)))


def reference(x, w1, b1, w2, b2, res, act, ln=None, eps=LN_EPS):
    """The plain float64 result (what tests/test_two_linear_host.py holds against torch)."""
    return hidden(x, w1, b1, act, ln, eps).g @ np.asarray(w2, np.float64).T + np.asarray(b2, np.float64) + np.asarray(res, np.float64)


# ----------------------------------------------------------------------------------------------------- operands
def _freeze(arrays):
    for a in arrays:
        a.setflags(write=False)
    return tuple(arrays)


def _ln_input(t, c, seed):
    """ln_rows' rows (a constant row, |mean| = 1e3 std, one spike, a zero row) at any t, every fourth row small, the constant -1.25 row
    last where t allows."""
    x, g, b = ln_rows(max(t, 32), c, seed)
    x = np.ascontiguousarray(x[:t])
    x[2::4] *= np.float32(2.0 ** -7)                              # variances of 1e-6 .. 4e-3: rows on which eps = 1e-5 matters
    if t > 22:
        x[t - 1] = -1.25
    return x, g, b


GLOBAL_MEAN_OVER_STD = 8.0   # tests/test_gpu_parity.py draws x = N(0, 1) s + m, s in [0.5, 3], m ~ N(0, 1): |mean| <= 4 sigma / 0.5 = 8 std


def global_rows(x, ln):
    """The rows the global figure covers: those of the class of inputs it was stated for, |mean| <= 8 std in LN builds.  Forming
    x - mean in fp32 leaves each normalised value |mean| / std u relative, in ANY fp32 LayerNorm (the emulation of
    tests/test_two_linear_host.py included): ln_rows' row 13 (|mean| = 1e3 std) sits at 6e-5, forty times the figure, and its rows of
    small scale (std 0.1, mean ~ 3) near it.  Those rows - and the constant ones, std = 0 - are held by the derived bounds only."""
    x = np.asarray(x, np.float64)
    if not ln:
        return np.ones(x.shape[0], bool)
    return np.abs(x.mean(1)) <= GLOBAL_MEAN_OVER_STD * x.std(1)


@functools.lru_cache(maxsize=None)
def operands(t, c, hid, ln, seed=0):
    """(x, w1, b1, w2, b2, res, gamma, beta) fp32, read-only.  Packed builds: linear_ref.operands' x ~ N(0, 1.5) and w1 ~ N(0, 1) /
    sqrt c with its two scaled rows; LN builds: ln_rows' rows, gamma, beta.  Either way pre-activations of unit scale, so GELU sees
    both tails.  w2 ~ N(0, 1) / sqrt hid with one scaled row; res ~ N(0, 1)."""
    rng = np.random.default_rng([t, c, hid, int(ln), 11 + seed])
    if ln:
        x, g, b = _ln_input(t, c, 300 + c + t + seed)
        w1 = (rng.normal(0.0, 1.0, (hid, c)) / math.sqrt(c)).astype(np.float32)
        w1[hid // 3] *= 4.0
        b1 = rng.normal(0.0, 0.5, hid).astype(np.float32)
    else:
        x, w1, b1, _ = (np.array(a) for a in lref.operands(t, hid, c, seed))
        g = b = np.zeros(0, np.float32)
    w2 = rng.normal(0.0, 1.0, (c, hid)) / math.sqrt(hid)
    w2[c // 3] *= 4.0
    out = [x, w1, b1, w2.astype(np.float32), rng.normal(0.0, 0.5, c).astype(np.float32), rng.normal(0.0, 1.0, (t, c)).astype(np.float32), g, b]
    return _freeze(out)


W_MAX = 2                    # |integer weights| of the exact families


def exact_bits(terms):
    """a: the integers n of x = n 2^-p range over [-2^a, 2^a] where `terms` products enter one fp32 accumulation (see exact_layer2)."""
    return int(math.floor(math.log2(2.0 ** 24 / (terms * W_MAX * (1.0 + 2.0 ** -12) + 2.0))))


@functools.lru_cache(maxsize=None)
def exact_layer2(t, c, hid, seed=0):
    """(x, w1, b1, w2, b2, res) for view 2; the output must equal the float64 result bit for bit.

    x = n 2^-p, n an integer in [-2^a, 2^a], p = a - 3 (|x| <= 8, lsb 2^-p >= 2^-14: every part is a normal f16 or an exact multiple of
    its subnormal step).  Such an x has up to a + 1 > 11 significant bits, so xl' = (x - xh) 2^11 is not zero, and at most 22, so it is an
    f16 exactly (x - xh is a multiple of 2^-p no larger than half an f16 ulp of x: <= 11 bits).
    GEMM 1 with W1 = selection_w1: acc = xh 2^11 + xl' + zeros = x 2^11, 22 bits: exact.  h = fmaf(acc, 2^-11, 0) = x; hh, hl' as above.
    GEMM 2 with integer |W2| <= W_MAX (w2l' = 0, w2h 2^11 <= 2^12 an f16): the terms hh w 2^11 and hl' w are multiples of q = 2^(11 - p)
    with |hh| <= 2^(a - p), |hl'| <= 2^(a - p - 1); any partial sum, in any order, is a multiple of q below
        hid W_MAX 2^(a - p) 2^11 (1 + 2^-12) <= 2^24 q      <=>      hid W_MAX 2^a (1 + 2^-12) <= 2^24,
    exact in fp32.  The epilogue adds b2 and res, multiples of 2^-p up to 2^(a - p) each: the `+ 2` of exact_bits keeps acc 2^-11 + b2 +
    res below 2^24 2^-p.  hid = 768: a = 13 (14-bit x); hid = 32: a = 17.  The hidden values stay below 8: no range guard."""
    a = exact_bits(hid)
    p = a - 3
    rng = np.random.default_rng([t, c, hid, 55 + seed])
    q = 2.0 ** -p
    x = rng.integers(-2 ** a, 2 ** a + 1, (t, c)) * q
    w2 = rng.integers(-W_MAX, W_MAX + 1, (c, hid))
    b2 = rng.integers(-2 ** a, 2 ** a + 1, c) * q
    res = rng.integers(-2 ** a, 2 ** a + 1, (t, c)) * q
    out = [x.astype(np.float32), selection_w1(c, hid), np.zeros(hid, np.float32), w2.astype(np.float32), b2.astype(np.float32), res.astype(np.float32)]
    assert all(np.array_equal(o.astype(np.float64), s) for o, s in zip((out[0], out[4], out[5]), (x, b2, res)))
    return _freeze(out)


@functools.lru_cache(maxsize=None)
def exact_layer1(t, c, hid, off=0, seed=0):
    """(x, w1, b1, w2, b2, res) for the mirror of view 2: W2 = selection_w2(c, hid, off), integer |W1| <= W_MAX, no activation.

    x = n 2^-p as in exact_layer2.  GEMM 1's terms xh w 2^11 and xl' w (w1l' = 0) are multiples of 2^(11 - p); the hidden value
    h = sum_k x_k w_k + b1 is a multiple of 2^-p and must itself split exactly into [hh | hl']: at most 22 significant bits,
        c W_MAX 2^a (1 + 2^-12) + 2^a <= 2^22      (b1 = integers 2^-p up to 2^(a - p))
    which a = exact_bits(4 c) satisfies (asserted below): a = 14 at c = 96 (p = 11), 13 at c = 192 - and keeps GEMM 1's partial sums
    (x 2^11) below 2^24 2^(11 - p) a fortiori.  |h| < 2^(22 - p) <= 2^12: far inside f16's range.  GEMM 2 sums hh 2^11 + hl' = h 2^11 and zeros; b2 and res (multiples of
    2^-p up to 2^(a - p)) leave |h + b2 + res| < 2^24 2^-p."""
    a = exact_bits(4 * c)
    assert c * W_MAX * 2 ** a * (1.0 + 2.0 ** -12) + 2 ** a <= 2 ** 22
    p = a - 3
    rng = np.random.default_rng([t, c, hid, off, 66 + seed])
    q = 2.0 ** -p
    x = rng.integers(-2 ** a, 2 ** a + 1, (t, c)) * q
    w1 = rng.integers(-W_MAX, W_MAX + 1, (hid, c))
    b1 = rng.integers(-2 ** a, 2 ** a + 1, hid) * q
    b2 = rng.integers(-2 ** a, 2 ** a + 1, c) * q
    res = rng.integers(-2 ** a, 2 ** a + 1, (t, c)) * q
    out = [x.astype(np.float32), w1.astype(np.float32), b1.astype(np.float32), selection_w2(c, hid, off), b2.astype(np.float32), res.astype(np.float32)]
    return _freeze(out)


# ----------------------------------------------------------------------------------------------------- case table
# alias: the forward's aliasing (flags bit 2 of reid_debug_two_linear_form) - LN builds: x32 == res == out; packed builds: res == out
Row = collections.namedtuple("Row", "c hid t act ln alias")
BUILDS = [(0, 0), (1, 0), (0, 1), (1, 1)]                      # (ACT, LN): to_out -> post_proj; test-only; test-only; the MLP
CS = (96, 192)
TS = (1, 31, 33, 127, 129, 257, 1024 + 49)                     # one token; a ragged wave; a full and a ragged wave; a ragged / a full and a
#                                                                ragged block; two blocks and a row; eight blocks and 49 rows (a 7 x 7 window)
RAGGED_IN_PLACE = (1, 31, 33, 129)                             # the in-place LN rows whose clamped lanes re-read a row being overwritten


def hid_classes(c):
    """hid = 32: NG = 1, the step(1, N, Y, N) branch; 64: no steady-state trip; 96: one trip; C: to_out -> post_proj; 4 C: the MLP."""
    return sorted({32, 64, 96, c, 4 * c})


def _table():
    rows = []
    for ci, c in enumerate(CS):
        hids = hid_classes(c)
        for bi, (act, ln) in enumerate(BUILDS):
            for ti, t in enumerate(TS):                        # every T meets the build; the hid classes rotate through them
                alias = 1 if (ln and t in RAGGED_IN_PLACE) else (ti + bi) % 2
                rows.append(Row(c, hids[(ti + bi + ci) % len(hids)], t, act, ln, alias))
        for t in (257, 1024 + 49):                             # the forward's two call shapes (csrc/swin.hip, the precision-2 branch)
            rows.append(Row(c, c, t, 0, 0, 0))                 # to_out -> post_proj: packed input, res = xin, out = xcur
            rows.append(Row(c, 4 * c, t, 1, 1, 1))             # LayerNorm 2 -> fc1 -> GELU -> fc2: x32 == res == out
    seen, out = set(), []
    for r in rows:
        if r not in seen:
            seen.add(r)
            out.append(r)
    return out


TABLE = _table()


def row_id(r):
    return "c%d-hid%d-t%d-%s%s%s" % (r.c, r.hid, r.t, "ln" if r.ln else "packed", "-gelu" if r.act else "", "-inplace" if r.alias else "")
