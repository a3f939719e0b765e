"""Float64 oracle, derived per-element bound, dispatch predicates and the case table of the Linear-layer tests (tests/test_linear_host.py on
the CPU, tests/test_gpu_linear.py on an MI355X).  The layers are y = act(x . w^T + bias) + res through linear() / linear16() of
csrc/swin.hip: the Swin trunk's to_qkv / to_out / post_proj / fc1 / fc2 and the classifiers, in the three precisions (0 exact fp32, 1 fp16
storage, 2 fp32-class on split f16 operands).

Oracle.  acc = x @ w.T and A = |x| @ |w|.T in float64, h = acc + bias, g = GELU(h) = 0.5 h (1 + erf(h / sqrt 2)) with math.erf, v = g + res.
Precision 1 runs on the f16-rounded x and w (what the kernel is given), as tests/test_gpu_swin_kernels.py does for its f16 forms.

Bound, per element (u = U = 2^-24; E_SPLIT, ABS_X, SAFETY of tests/test_gpu_conv.py; H16, H16_ABS, PK_REL, PK_ABS of
tests/test_gpu_swin_kernels.py; nothing is fitted to observed errors):
  contraction  con = K u A: a K-term fp32 accumulation of exact products, in any order.  Precision 2 adds E_SPLIT A + ABS_X sum_k |w_nk| (three
               f16 products per multiply).  Precision 1 adds nothing: the oracle has the rounded operands and their products are exact in fp32.
  epilogue     pre = con + 4u (|acc| + |bias|); without GELU the element is off by pre + 4u |res|.
  GELU         c = GELU_LIP = 1.13 > max |GELU'| = 1.1290 (at |h| = sqrt 2), so a pre-activation error e leaves c e.  The function's own error
               enters as |h| / 2 times the error of erf, E_erf, plus P u |g| for the roundings of the products:
               precision 0: erff of the device library, ERFF_ULPS = 16 ulp = 32u relative (chosen: the OpenCL full-profile limit of erf,
                 which the library is written to) + 1u for the rounding of h 2^-1/2 (two roundings, 2u relative, through z erf'(z) <= 0.49) +
                 2u for the sum 1 + erf; P = 3 (0.5 v, the product, its rounding).
               precisions 1, 2: gelu_f16_storage / gelu2_f16_storage of csrc/lin_math.h (bit-identical by construction), erf(z) = 1 - q^-16,
                 q = 1 + a1 z + .. + a6 z^6 (Abramowitz-Stegun 7.1.28, |error| <= AS_ERR = 3e-7).  z = |v| 2^-1/2: 1u absolute as above.  The
                 Horner chain is six fmaf on positive terms: 6u relative.  Each of the four squarings doubles the relative error and adds its
                 own u: 6 -> 13 -> 27 -> 55 -> 111 u.  v_rcp_f32 is good to 1 ulp = 2u (chosen): r = q^-16 carries AS_CHAIN = 113 u relative,
                 i.e. 113 u (1 - |erf z|) absolute; the subtraction 1 - r adds 1u.  h = 0.5 v is exact and the final fmaf rounds once: P = 1.
               With GELU the element is off by c pre + (|h| / 2) E_erf + P u |g| + u |v| + 4u |res|.
  output form  f16 rows: + H16 |v| + H16_ABS; the packed pair [yh | yl']: + PK_REL |v| + PK_ABS.
  bound = SAFETY times the sum.

Recorded (one MI355X run; worst error / bound over the table's rows per launch form, every line in profiles/linear_gpu_tests.log; a
record, not the source of any constant):
  precision 0: gemm_f32_dma<64> 0.030, gemm_f32_kernel<64> 0.137, <128> 0.135 (both on the K = 4 / K = 8 rows, where K u A is only 4 - 8
               roundings wide; the rows with K >= 28 stay below 0.06);
  precision 1: lin64323 0.475, lin128323 0.469, lin256324 0.308 (f16 rows sit at half their bound: the output's own rounding, 2^-11 |v| of
               a SAFETY 2^-10 |v|, is most of it);
  precision 2: lin_x3 0.017, lin64323 0.018, lin128323 0.020, lin256642 0.005, lin256324 0.003; the unpacked-x row on gemm_f32_dma<64> 0.016.
  gemm_f32_dma_kernel and gemm_f32_kernel agreed bit for bit on 305 x 384 x 96 with bias, GELU and residual.

Found while this module was written: with GELU AND a residual in one launch, gemm_f32_dma_kernel's buffer epilogue (full tiles) compiled
0.5 v (1 + erf) + res into one fma and its element-by-element epilogue (the ragged last tile) into a product and a sum, so a row's bits
depended on its tile.  The forward makes no such launch and its results are unchanged; the epilogues now share gelu_erf_f32 (csrc/lin_math.h)
and test_equal_rows_give_equal_bits_in_every_tile_position holds it.

Dispatch.  linear_form() restates launch_gemm_f32 / gemm_f32_dma_supported / launch_epi / launch_bn (csrc/gemm_f32.hip, gemm_f32_dma.hip),
lin_x3_supported (csrc/conv3x3_x3.hip) and the LIN branch of launch_any (csrc/gemm_f16.hip); the value is what the launchers leave in
reid_ctx::conv_form (include/reid_hip_debug.h, reid_debug_swin_linear).
"""
import collections
import functools
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_conv import ABS_X, E_SPLIT, SAFETY, U  # noqa: E402
from test_gpu_swin_kernels import H16, H16_ABS, PK_ABS, PK_REL  # noqa: E402

GELU_LIP = 1.13
ERFF_ULPS = 16
AS_ERR = 3e-7
AS_CHAIN = 113

# ----------------------------------------------------------------------------------------------------- launch forms
DMA64, F32_64, F32_128 = 5064320, 6064000, 6128000            # gemm_f32_dma_kernel<64, E_BIAS>; gemm_f32_kernel<A_DENSE, E_BIAS, 64 | 128>
LIN64, LIN128, LIN256, LIN256_BK32 = 64323, 128323, 256642, 256324   # gemm_f16_kernel<A16_DENSE, BN, BK, NST, 0, LIN>
X3 = 7128000                                                   # lin_x3_kernel<128>
FORM_NAMES = {DMA64: "gemm_f32_dma64", F32_64: "gemm_f32_64", F32_128: "gemm_f32_128", LIN64: "lin64323", LIN128: "lin128323",
              LIN256: "lin256642", LIN256_BK32: "lin256324", X3: "lin_x3"}
DEFAULT_SWITCHES = {"f32_conv": 1, "lin_x3": 1, "f16_lin_256": 1, "f16_cfg": 0}
OUT_F32, OUT_F16, OUT_PACKED = 0, 1, 2


def ceil64(n):
    return (n + 63) // 64 * 64


def attn_ldq(precision, c):
    """swin_attn_ldq: the row stride of the qkv buffer"""
    return ceil64(3 * c) if precision == 1 else 3 * c


def linear_form(precision, m, n, k, out_form=OUT_F32, switches=None, x_fp32=False):
    """The kernel linear() / linear16() launch, as the code the launcher leaves in reid_ctx::conv_form."""
    sw = dict(DEFAULT_SWITCHES)
    sw.update(switches or {})
    if precision == 0 or (precision == 2 and (x_fp32 or k % 32 != 0)):
        # linear()'s exact branch: launch_gemm_f32(A_DENSE, E_BIAS) with lda = ldb = K = k (the harness's buffers are 16-byte aligned)
        if k % 4 != 0:
            raise ValueError("launch_gemm_f32 refuses K % 4 != 0")
        if sw["f32_conv"] == 1 and k % 32 == 0 and 128 * k * 4 < 0x7fff0000:
            return DMA64                                       # launch_epi: E_BIAS takes the 64-wide tile at every width
        return F32_64 if n <= 64 else F32_128                  # launch_bn
    if k % 32 != 0:
        raise ValueError("launch_gemm_f16 refuses K % 32 != 0")
    N, K = ceil64(n), (3 * k if precision == 2 else k)
    if precision == 2 and sw["lin_x3"] and N % 128 == 0 and n == N:
        return X3                                              # lin_x3_supported: K % 96 == 0 holds for every k % 32 == 0
    cfg = sw["f16_cfg"]
    if cfg == 0 or N % ((cfg % 1000000) // 1000) != 0:         # launch_any with p.lin
        k64 = K % 64 == 0
        bn = 128 if N % 128 == 0 else 64
        if sw["f16_lin_256"] and precision == 2 and N % 256 == 0 and k64 and K >= 1152:
            bn = 256
        if not k64:
            cfg = bn * 1000 + 320 + (4 if bn == 256 else 3)
        elif bn == 128 and N == 128:
            cfg = 128323
        else:
            cfg = 256642 if bn == 256 else bn * 1000 + 323
    if cfg not in (LIN64, LIN128, LIN256, LIN256_BK32):
        raise ValueError("no linear-epilogue build of tile configuration %d" % cfg)
    return cfg


def epilogue_paths(form, m, n, out_form):
    """The epilogue code paths of a launch: gemm_f32_dma's bias_lean on full 128-row tiles and bias_general on the rest; the LIN builds' LDS-
    staged store (f16 / packed rows with n % 8 == 0), buffer stream (fp32 rows of full 256-row tiles) and general loop."""
    if form == DMA64:
        return ({"lean"} if m >= 128 else set()) | ({"general"} if m % 128 else set())
    if form in (F32_64, F32_128):
        return {"general"}
    if form == X3:
        return {"tail"}                                        # x3m16_tail: one path, rows past M dropped by the output descriptors
    if out_form != OUT_F32:
        return {"staged"} if n % 8 == 0 else {"general"}
    return ({"stream"} if m >= 256 else set()) | ({"general"} if m % 256 else set())


# ----------------------------------------------------------------------------------------------------- oracle and bound
_erf = np.frompyfunc(math.erf, 1, 1)


def f16r(a):
    return np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


Parts = collections.namedtuple("Parts", "acc A w1 bias h erf g res v")


def oracle(x, w, bias=None, res=None, act=False, precision=0):
    """Float64 pieces of y = act(x . w^T + bias) + res; precision 1: on the f16-rounded x and w."""
    if precision == 1:
        x, w = f16r(x), f16r(w)
    x64, w64 = np.asarray(x, np.float64), np.asarray(w, np.float64)
    acc = x64 @ w64.T
    A = np.abs(x64) @ np.abs(w64).T
    w1 = np.abs(w64).sum(1)
    b = np.zeros(w64.shape[0]) if bias is None else np.asarray(bias, np.float64)
    h = acc + b
    if act:
        erf = _erf(h / math.sqrt(2.0)).astype(np.float64)
        g = 0.5 * h * (1.0 + erf)
    else:
        erf, g = None, h
    r = np.zeros_like(acc) if res is None else np.asarray(res, np.float64).reshape(acc.shape)
    return Parts(acc, A, w1, np.broadcast_to(np.abs(b), acc.shape), h, erf, g, r, g + r)


def bound(p, precision, k, act=False, out_form=OUT_F32, split=None):
    """The module docstring's model on the oracle's pieces.  split: the three-product contraction (default: precision 2)."""
    split = precision == 2 if split is None else split
    con = k * U * p.A
    if split:
        con = con + E_SPLIT * p.A + ABS_X * p.w1[None, :]
    pre = con + 4 * U * (np.abs(p.acc) + p.bias)
    if act:
        if precision == 0 and not split:
            e_erf, prods = ERFF_ULPS * 2 * U * np.abs(p.erf) + 3 * U, 3
        else:
            e_erf, prods = AS_ERR + U + AS_CHAIN * U * (1.0 - np.abs(p.erf)) + U, 1
        b = GELU_LIP * pre + 0.5 * np.abs(p.h) * e_erf + prods * U * np.abs(p.g) + U * np.abs(p.v) + 4 * U * np.abs(p.res)
    else:
        b = pre + 4 * U * np.abs(p.res)
    if out_form == OUT_F16:
        b = b + H16 * np.abs(p.v) + H16_ABS
    elif out_form == OUT_PACKED:
        b = b + PK_REL * np.abs(p.v) + PK_ABS
    return SAFETY * b


@functools.lru_cache(maxsize=None)
def operands(m, n, k, seed=0):
    """(x, w, bias, res) fp32: x ~ N(0, 1.5), w ~ N(0, 1) / sqrt k - pre-activations of unit scale, so GELU sees both tails - and two rows /
    columns of larger scale; read-only."""
    rng = np.random.default_rng([m, n, k, seed])
    x = rng.normal(0.0, 1.5, (m, k))
    w = rng.normal(0.0, 1.0, (n, k)) / math.sqrt(k)
    x[m // 2] *= 3.0
    w[n // 3] *= 4.0
    out = [a.astype(np.float32) for a in (x, w, rng.normal(0.0, 0.5, n), rng.normal(0.0, 1.0, (m, n)))]
    for a in out:
        a.setflags(write=False)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def exact_operands(m, n, k, seed=0):
    """Integer-valued x, w in [-8, 8], bias and res in [-64, 64]: every product and partial sum is exact in fp32 (|sum| <= 64 k < 2^24) and
    in the f16 hi parts (w 2^11 <= 2^14), so every precision must give the float64 result bit for bit."""
    rng = np.random.default_rng([m, n, k, 77 + seed])
    out = [rng.integers(-8, 9, (m, k)), rng.integers(-8, 9, (n, k)), rng.integers(-64, 65, n), rng.integers(-64, 65, (m, n))]
    out = [a.astype(np.float32) for a in out]
    for a in out:
        a.setflags(write=False)
    return tuple(out)


# ----------------------------------------------------------------------------------------------------- case table
# res: 0 none, 1 an fp32 residual, 2 the same with the residual aliased to the output (the launch must equal the non-aliased one bit for bit)
Row = collections.namedtuple("Row", "precision m n k act res out_form ldc switches form x_fp32")


def R(precision, m, n, k, act, res, out_form, ldc, switches, form, x_fp32=False):
    return Row(precision, m, n, k, act, res, out_form, ldc, tuple(sorted(switches.items())), form, x_fp32)


F, H, P = OUT_F32, OUT_F16, OUT_PACKED
NO_DMA, NO_X3 = {"f32_conv": 0}, {"lin_x3": 0}
LINEAR_TABLE = [
    # ------------------------------------------------------------------ precision 0: gemm_f32_dma_kernel<64, E_BIAS> (k % 32 == 0)
    R(0, 1, 288, 96, 0, 0, F, 288, {}, DMA64),        # a single token: one ragged tile, general epilogue; 288 = 4.5 column tiles
    R(0, 49, 96, 96, 0, 1, F, 96, {}, DMA64),         # one window: general epilogue with residual
    R(0, 127, 384, 96, 1, 0, F, 384, {}, DMA64),      # one row short of a tile: general epilogue with GELU
    R(0, 128, 288, 96, 0, 0, F, 288, {}, DMA64),      # exactly one full tile: lean epilogue, plain; the half column tile is cut by the descriptor
    R(0, 128, 384, 96, 1, 0, F, 384, {}, DMA64),      # lean epilogue, GELU (fc1 of stage 1)
    R(0, 128, 96, 384, 0, 2, F, 96, {}, DMA64),       # lean epilogue, residual in place (fc2 of stage 1)
    R(0, 129, 96, 96, 1, 1, F, 96, {}, DMA64),        # lean epilogue, GELU + residual; one row in the ragged tile
    R(0, 305, 576, 192, 0, 0, F, 576, {}, DMA64),     # two full tiles and a ragged one (qkv of stage 2)
    R(0, 255, 384, 384, 0, 2, F, 384, {}, DMA64),     # stage 3 to_out / post_proj in place; 127 rows in the ragged tile
    R(0, 257, 1152, 384, 0, 0, F, 1152, {}, DMA64),   # qkv of stage 3
    R(0, 256, 1536, 384, 1, 0, F, 1536, {}, DMA64),   # fc1 of stage 3: lean GELU only
    R(0, 129, 384, 1536, 0, 2, F, 384, {}, DMA64),    # fc2 of stage 3 in place: 48 K-tiles
    R(0, 49, 768, 768, 0, 1, F, 768, {}, DMA64),      # stage 4: one image
    R(0, 305, 3072, 768, 1, 0, F, 3072, {}, DMA64),   # fc1 of stage 4: the widest launch
    R(0, 128, 768, 3072, 0, 2, F, 768, {}, DMA64),    # fc2 of stage 4: an A tile of 1.5 MiB (the row-major tile order, GM = 1)
    R(0, 5, 751, 96, 0, 0, F, 751, {}, DMA64),        # the Swin classifier: odd ldc, 47 columns in the last tile
    R(0, 129, 751, 96, 0, 0, F, 751, {}, DMA64),      # ... through the lean epilogue: rows that are not 16-byte aligned
    R(0, 3, 751, 512, 0, 0, F, 751, {}, DMA64),       # the ResNet classifier
    R(0, 49, 5, 96, 0, 0, F, 5, {}, DMA64),           # a small class count: five columns of one tile
    # ------------------------------------------------------------------ precision 0: gemm_f32_kernel<A_DENSE, E_BIAS, 64 | 128>
    R(0, 129, 5, 96, 0, 0, F, 5, NO_DMA, F32_64),     # f32_conv = 0, n <= 64: the 64-wide tile
    R(0, 305, 96, 96, 1, 1, F, 96, NO_DMA, F32_128),  # f32_conv = 0: the 128-wide tile with 96 columns, GELU + residual
    R(0, 129, 288, 96, 1, 0, F, 288, NO_DMA, F32_128),   # ... 2.25 column tiles
    R(0, 128, 96, 384, 0, 2, F, 96, NO_DMA, F32_128),    # ... residual in place
    R(0, 129, 96, 36, 0, 0, F, 96, {}, F32_128),      # k % 32 != 0 (what reid_gemm_nt's callers may pass): the K-tail guard in the second tile
    R(0, 49, 5, 36, 0, 1, F, 5, {}, F32_64),
    R(0, 33, 8, 4, 0, 0, F, 8, {}, F32_64),           # short K (reid_cam_debias: a camera of 1 .. 4 rows, d = 33 -> a 33 x 8 corner)
    R(0, 1, 96, 4, 0, 0, F, 96, {}, F32_128),
    R(0, 130, 8, 8, 0, 0, F, 8, {}, F32_64),          # K = 8: two of eight float4 columns of the only K-tile
    R(0, 129, 96, 8, 0, 0, F, 96, {}, F32_128),
    R(0, 5, 8, 28, 0, 0, F, 8, {}, F32_64),           # K = 28: the last float4 column of the tile is the guard's
    R(0, 49, 96, 28, 0, 0, F, 96, {}, F32_128),
    # ------------------------------------------------------------------ precision 2 with x left in fp32: the classifier stays exact
    R(2, 5, 751, 96, 0, 0, F, 751, {}, DMA64, True),
    # ------------------------------------------------------------------ precision 1 (linear16): 64-wide LIN build
    R(1, 49, 288, 96, 0, 0, H, 320, {}, LIN64),       # qkv of stage 1 into rows of swin_attn_ldq = 320: N = 320, staged store
    R(1, 257, 288, 96, 0, 0, H, 288, {}, LIN64),      # ... ldc = n; one row in the second tile
    R(1, 255, 192, 192, 0, 2, F, 192, {}, LIN64),     # stage 2 to_out / post_proj in place: general loop only (no full tile)
    R(1, 256, 576, 192, 0, 0, H, 576, {}, LIN64),     # qkv of stage 2 (ldq = 576 = n): K % 64 == 0 still takes BK 32
    R(1, 305, 192, 192, 0, 1, F, 192, {}, LIN64),     # buffer stream on the full tile, general loop on the ragged one
    # ------------------------------------------------------------------ precision 1: 128-wide LIN build
    R(1, 1, 96, 96, 0, 1, F, 96, {}, LIN128),         # n = 96 runs as N = 128; a single token
    R(1, 305, 96, 96, 0, 2, F, 96, {}, LIN128),       # ... in place, columns 96 .. 127 cut by the descriptor / the general loop
    R(1, 129, 384, 96, 1, 0, H, 384, {}, LIN128),     # fc1 of stage 1: GELU with f16 output
    R(1, 256, 96, 384, 0, 2, F, 96, {}, LIN128),      # fc2 of stage 1 in place
    R(1, 127, 1152, 384, 0, 0, H, 1152, {}, LIN128),  # qkv of stage 3
    R(1, 257, 384, 384, 0, 1, F, 384, {}, LIN128),
    R(1, 255, 1536, 384, 1, 0, H, 1536, {}, LIN128),  # fc1 of stage 3
    R(1, 49, 384, 1536, 0, 1, F, 384, {}, LIN128),    # fc2 of stage 3
    R(1, 49, 768, 768, 0, 1, F, 768, {}, LIN128),
    R(1, 305, 3072, 768, 1, 0, H, 3072, {}, LIN128),  # fc1 of stage 4
    R(1, 128, 768, 3072, 0, 2, F, 768, {}, LIN128),   # fc2 of stage 4 in place: 96 K-tiles
    R(1, 305, 768, 768, 0, 0, H, 768, {"f16_cfg": 256324}, LIN256_BK32),   # the 256-wide BK 32 build exists only behind f16_cfg
    # ------------------------------------------------------------------ precision 2 (linear, packed x): lin_x3_kernel<128>
    R(2, 49, 384, 96, 1, 0, P, 384, {}, X3),          # the shortest K loop (three virtual K-tiles), GELU with packed output
    R(2, 1, 768, 768, 0, 0, P, 768, {}, X3),          # a single token
    R(2, 305, 1152, 384, 0, 0, P, 1152, {}, X3),      # qkv of stage 3: nine column tiles, a full and a ragged row tile
    R(2, 256, 384, 384, 0, 2, F, 384, {}, X3),        # to_out / post_proj of stage 3 in place
    R(2, 257, 1536, 384, 1, 0, P, 1536, {}, X3),      # fc1 of stage 3
    R(2, 129, 384, 1536, 0, 2, F, 384, {}, X3),       # fc2 of stage 3 in place
    R(2, 255, 768, 768, 0, 1, F, 768, {}, X3),
    R(2, 305, 3072, 768, 1, 0, P, 3072, {}, X3),      # fc1 of stage 4
    R(2, 128, 768, 3072, 0, 2, F, 768, {}, X3),       # fc2 of stage 4 in place
    # ------------------------------------------------------------------ precision 2: the gemm_f16 LIN builds with split_terms = 3
    R(2, 49, 288, 96, 0, 0, P, 288, {}, LIN64),       # N = 320 is no multiple of 128: 64-wide; the low plane starts 288 columns in
    R(2, 257, 192, 192, 0, 2, F, 192, {}, LIN64),
    R(2, 305, 576, 192, 0, 0, P, 576, {}, LIN64),
    R(2, 129, 96, 96, 0, 2, F, 96, {}, LIN128),       # n = 96 as N = 128 (n_real != N keeps it off lin_x3)
    R(2, 256, 96, 384, 0, 1, F, 96, {}, LIN128),      # fc2 of stage 1: K = 1152 with N = 128
    R(2, 305, 96, 96, 0, 0, P, 96, {}, LIN128),       # packed output 96 wide: both planes inside one 128-wide tile's columns
    R(2, 305, 384, 96, 1, 0, P, 384, NO_X3, LIN128),  # n % 128 == 0 under lin_x3 = 0; K = 288 is no multiple of 64
    R(2, 127, 1152, 384, 0, 0, P, 1152, NO_X3, LIN128),   # 1152 % 256 != 0 keeps the 128-wide tile at K = 1152
    R(2, 257, 384, 384, 0, 2, F, 384, NO_X3, LIN128),
    R(2, 257, 768, 768, 0, 2, F, 768, NO_X3, LIN256),     # the 256 x 256 tile, BK 64: n % 256 == 0, 3 k = 2304
    R(2, 305, 3072, 768, 1, 0, P, 3072, NO_X3, LIN256),
    R(2, 49, 768, 3072, 0, 1, F, 768, NO_X3, LIN256),     # 144 K-tiles of 64
    R(2, 129, 1536, 384, 1, 0, P, 1536, NO_X3, LIN256),   # the smallest K the 256-wide tile takes: 3 k = 1152
    R(2, 257, 768, 768, 0, 1, F, 768, {"lin_x3": 0, "f16_lin_256": 0}, LIN128),   # f16_lin_256 = 0 puts the same shape on 128323
    R(2, 305, 768, 768, 0, 0, P, 768, {"lin_x3": 0, "f16_cfg": 256324}, LIN256_BK32),
]

# what the table must reach (tests/test_linear_host.py): (precision, form) and, per form, the epilogue paths and variants
REQUIRED_FORMS = {
    0: (DMA64, F32_64, F32_128),
    1: (LIN64, LIN128, LIN256_BK32),
    2: (X3, LIN64, LIN128, LIN256, LIN256_BK32, DMA64),
}


def row_id(r):
    s = "p%d-%s-%dx%dx%d" % (r.precision, FORM_NAMES[r.form], r.m, r.n, r.k)
    s += ("-gelu" if r.act else "") + ("", "-res", "-inplace")[r.res] + ("", "-f16", "-packed")[r.out_form]
    s += ("-ldc%d" % r.ldc if r.ldc != r.n else "") + ("-xfp32" if r.x_fp32 else "")
    return s + "".join("-%s%d" % kv for kv in r.switches)
