"""Case tables, oracles and bounds of libreid_hip_anysize_sib_f16.so (csrc/anysize_sib_f16.h): the TripletAttention tail of CARes18-IBN and
the EMA tail of EMARes18-IBN for any map size on f16 maps, and an fp16-storage restatement of both sibling forwards.
tests/test_gpu_anysize_sib_f16.py holds the kernels and the forward to these on the MI355X; tests/test_anysize_sib_f16_host.py holds the
restatement to the reference fixtures and shows one mutation per tail that the GPU check would catch.

Kernels.  The operands are those of tests/anysize_ca_ref.py / tests/anysize_ema_ref.py (operands, make_prm, CASES, FAMILIES) with y and
the shortcut rounded to float16 first; the float64 oracle (tail) and the fp32 bound b32 (bounds) of those modules are evaluated on the
rounded values - the tails form their statistics, gates and combine as the fp32 tails do, on inputs that happen to be f16 values.  The
returned fp32 statistics are held to b32 unchanged; the output is rounded to f16 once at its store, so with H = 2^-11 (f16 half-ulp,
relative) and 2^-25 (the same below f16's normal range, absolute)

    bound(out) = anysize_f16_ref.store_bound(v, b32) = b32 + H (|v| + b32) + 2^-25,      v the float64 oracle's output.

Forward.  The limits are the mode-1 limits of tests/anysize_f16_ref.py: 1 - cos < COS_LIMIT, embeddings, logits and block taps within
EMB_LIMIT / STAGE_LIMIT of the largest magnitude."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import anysize_ca_ref as ca  # noqa: E402
import anysize_ema_ref as ema  # noqa: E402
import anysize_f16_ref as f16r  # noqa: E402

COS_LIMIT, EMB_LIMIT, STAGE_LIMIT = f16r.COS_LIMIT, f16r.EMB_LIMIT, f16r.STAGE_LIMIT
F16_MAX = 65504.0
BATCHES = (1, 3)
# (H, W, C): every cg from 2 to 16, maps smaller than the 3 x 3 / 7 x 7 windows, odd widths, a 2-wide and a 128-long line, a slab split
CA_CASES = ca.CASES
EMA_CASES = ema.CASES
CA_FAMILIES = ca.FAMILIES
EMA_FAMILIES = ema.FAMILIES
EMA_NAMES = ema.NAMES
FORWARD_CASES = (0, 1, 2)                          # tests/golden/anysize_ca.npz, anysize_ema.npz: (64, 32), (96, 72), (224, 268)
ARCHS = {"cares18_ibn": "anysize_ca.npz", "emares18_ibn": "anysize_ema.npz"}


def batches(case):
    """n in (1, 3), except n = 1 alone at (128, 128, 64)."""
    return (1,) if case == (128, 128, 64) else BATCHES


def _rounded(y, sc):
    """-> (y16, sc16 float16, the same values as float32)."""
    y16, sc16 = np.ascontiguousarray(y, np.float16), np.ascontiguousarray(sc, np.float16)
    return y16, sc16, y16.astype(np.float32), sc16.astype(np.float32)


def ca_operands(case, n, family, seed=0):
    """(y16, sc16) float16 [n][H][W][C] and prm [3][100] of the TripletAttention tail."""
    y, sc = ca.operands(case, n, family, seed)
    return _rounded(y, sc)[:2] + (ca.make_prm(ca.CASES.index(case)),)


def ema_operands(case, n, family, seed=0):
    y, sc = ema.operands(case, n, family, seed)
    return _rounded(y, sc)[:2] + (ema.make_prm(case[2], ema.CASES.index(case)),)


def ca_case(case, n, family):
    """The GPU test's case: a dict with the operands (y, sc float16, prm), the float64 oracle (out, maps, gates) and the bounds (b_out =
    store_bound, b_maps, b_gates = b32)."""
    y16, sc16, prm = ca_operands(case, n, family)
    yv, sv = y16.astype(np.float32), sc16.astype(np.float32)
    out, maps, gates = ca.tail(yv, sv, prm)
    b_out, b_maps, b_gates = ca.bounds(yv, sv, prm)
    return {"y": y16, "sc": sc16, "prm": prm, "out": out, "maps": maps, "gates": gates, "b32_out": b_out,
            "b_out": f16r.store_bound(out, b_out), "b_maps": b_maps, "b_gates": b_gates}


def ema_case(case, n, family):
    """The GPU test's case: the operands, the float64 oracle as ema.tail returns it ("want"), b32 per name ("b32") and the output's
    store_bound ("b_out")."""
    y16, sc16, prm = ema_operands(case, n, family)
    yv, sv = y16.astype(np.float32), sc16.astype(np.float32)
    want, b32 = ema.tail(yv, sv, prm), ema.bounds(yv, sv, prm)
    return {"y": y16, "sc": sc16, "prm": prm, "want": want, "b32": b32, "b_out": f16r.store_bound(want["out"], b32["out"])}


def twice_rounded(stat):
    """The mutation of tests/test_anysize_sib_f16_host.py: a statistic that went through f16 on its way (a tail that keeps its statistics in
    f16 and so rounds what it stores twice)."""
    return f16r.f16(stat)


# ---------------------------------------------------------------------------------------------- the sibling forwards, restated
def forward_sib_f16(sd, x, arch, taps=None):
    """oracle/seres18.py's cares18_ibn / emares18_ibn forward with the rounding points of the fp16-storage any-size forward, everything else
    float64 (anysize_f16_ref.forward_f16 with the block tail exchanged): input, weights and every stored activation are rounded to f16
    once; the TripletAttention / EMA tail reads the stored y and shortcut and is not rounded inside - its statistics, gates and combine
    are float64 - until the block's output is stored.  x: float32 [n, 3, h, w].  Returns (emb, logits) float64 and fills `taps` with the
    stage maps under oracle names (NCHW)."""
    import torch
    import torch.nn.functional as F
    from oracle import seres18
    assert arch in ARCHS
    sd64 = {}
    for k, v in sd.items():
        t = v if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v))
        sd64[k] = t.to(torch.float64) if t.is_floating_point() else t

    def t(k):
        return seres18._t(sd64, k)

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
            if arch == "cares18_ibn":
                x = r16(F.relu(seres18._triplet(sd64, name + ".cablock", y) + sc))
            else:
                x = r16(F.relu(seres18._ema(sd64, name + ".emablock", y) + sc))
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


def sample_nchw(t):
    """tools/gen_golden_anysize_ca.py's sample of a block tap [n, c, ho, wo] (what the fixtures keep under tap_<block>)."""
    n, c, ho, wo = t.shape
    return t[:, :: max(1, c // 8), :: max(1, ho // 8), :: max(1, wo // 4)]
