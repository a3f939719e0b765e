"""Generates tests/golden/swin_v2.npz from the REFERENCE's own swin_t(version="v2") (CPU only; run where the reference tree is).

    python tools/gen_golden_swin_v2.py --reference /path/to/reference

The reference imports ``trunc_normal_`` and ``Mlp`` from timm (swin_transformer.py:12-13), which is absent here.  ``trunc_normal_``
is torch's; ``Mlp`` below is a stand-in of ours with timm's attribute names (fc1 / act / drop1 / fc2 / drop2), which is all the
state_dict keys and the eval-mode arithmetic depend on (the dropouts are identities in eval mode).  Nothing of the reference is
written to the repository: the fixture holds key names, shapes and numbers its classes produced.

Weights: synth.swin_state_dict(0, version="v2").  Contents of the fixture:
  keys / shapes          the reference's v2 state_dict(), in its order (keys: one newline-joined byte string)
  bias13_* / scale_*     for stage1.layers.0.0 (unshifted) and stage4.layers.0.1 (shifted): _relative_positional_encodings() and
                         exp(clamp(logit_scale, max=ln 100)).  The [heads][49][49] table has one value per relative offset; the
                         generator checks that bit for bit and stores the [heads][13][13] form (entry [dy + 6][dx + 6], d = query
                         - key), from which the test rebuilds the full table
  emb / logits / tap_* / mean_* / absmean_*   as tests/golden/swin_seed0.npz, for synth.images_f32(2, 0)
  rank_*                 64 images in one batch: embeddings, the reference's cosine_dist matrix (rank_cosdist_triu: its upper triangle
                         with the diagonal, row by row - the generator checks that the matrix is symmetric bit for bit), its row
                         arg-min off the diagonal and the top-2 gaps.  The image seed is the first of RANK_SEEDS whose smallest gap is above 2e-6 (the bar
                         the GPU rank test holds every row to); the float64 run of the same model is printed beside it.
"""
import argparse
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "swin_v2.npz")
RANK_SEEDS = (11, 5, 6, 7, 8, 9, 10, 12, 13)
RANK_BAR = 2e-6
BLOCKS = (("s1b0", "stage1.layers.0.0"), ("s4b1", "stage4.layers.0.1"))


class Mlp(nn.Module):
    """Stand-in for timm.models.layers.Mlp: Linear -> act -> Dropout -> Linear -> Dropout under timm's attribute names."""

    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.0):
        super().__init__()
        drops = drop if isinstance(drop, (tuple, list)) else (drop, drop)
        self.fc1 = nn.Linear(in_features, hidden_features or in_features)
        self.act = act_layer()
        self.drop1 = nn.Dropout(drops[0])
        self.fc2 = nn.Linear(hidden_features or in_features, out_features or in_features)
        self.drop2 = nn.Dropout(drops[1])

    def forward(self, x):
        return self.drop2(self.fc2(self.drop1(self.act(self.fc1(x)))))


def _stand_ins(reference):
    tl = types.ModuleType("timm.models.layers")
    tl.trunc_normal_ = torch.nn.init.trunc_normal_
    tl.Mlp = Mlp
    for n in ("timm", "timm.models"):
        sys.modules.setdefault(n, types.ModuleType(n))
    sys.modules["timm.models.layers"] = tl
    tv = types.ModuleType("torchvision")
    tv.models = types.ModuleType("torchvision.models")
    sys.modules.setdefault("torchvision", tv)
    sys.modules.setdefault("torchvision.models", tv.models)
    sys.path.insert(0, reference)
    sys.path.insert(0, os.path.join(reference, "reid"))


def _sample(t):
    t = t.detach()
    if t.dim() == 4:
        n, c, h, w = t.shape
        return t[:, :: max(1, c // 8), :: max(1, h // 8), :: max(1, w // 4)].contiguous().numpy()
    return t.numpy()


def _ranks(dist):
    d = np.array(dist, np.float64)
    np.fill_diagonal(d, np.inf)
    srt = np.sort(d, axis=1)
    return d.argmin(1).astype(np.int32), srt[:, 1] - srt[:, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference tree (holds reid/backbones/swin_transformer.py)")
    args = ap.parse_args()
    from reid_amd import synth
    _stand_ins(args.reference)
    from reid.backbones.swin_transformer import swin_t
    from reid.losses.utils import cosine_dist

    torch.manual_seed(0)
    sd_np = synth.swin_state_dict(0, version="v2")
    model = swin_t(num_classes=751, loss="triplet", version="v2")
    ref_sd = model.state_dict()
    assert list(ref_sd) == list(sd_np), [(a, b) for a, b in zip(ref_sd, sd_np) if a != b][:5]
    assert all(tuple(ref_sd[k].shape) == tuple(sd_np[k].shape) for k in ref_sd)
    v1_keys = list(swin_t(num_classes=751, loss="triplet").state_dict())
    print("state_dict entries: v1 %d, v2 %d" % (len(v1_keys), len(ref_sd)))
    res = model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd_np.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    model.eval()

    out = {"keys": np.array("\n".join(ref_sd).encode()), "shapes": np.array([list(ref_sd[k].shape) + [-1] * (4 - ref_sd[k].dim()) for k in ref_sd], np.int32)}
    idx = np.arange(49)
    dy = (idx // 7)[:, None] - (idx // 7)[None, :] + 6
    dx = (idx % 7)[:, None] - (idx % 7)[None, :] + 6
    for tag, pre in BLOCKS:
        attn = model.get_submodule(pre + ".attention_block.fn.fn")
        with torch.no_grad():
            table = attn._relative_positional_encodings()[0].numpy()                       # [heads][49][49]
            scale = torch.clamp(attn.logit_scale, max=float(np.log(1.0 / 0.01))).exp().numpy()
        t13 = np.zeros((table.shape[0], 13, 13), np.float32)
        t13[:, dy, dx] = table
        assert np.array_equal(t13[:, dy, dx], table), "the reference's table is not a function of the relative offset alone"
        out["bias13_" + tag], out["scale_" + tag] = t13, scale.astype(np.float32)
        print(tag, "heads", table.shape[0], "max |bias| %.3f" % np.abs(table).max(), "scales", np.round(scale, 2)[:6],
              "heads at the clamp:", int((scale >= 99.999).sum()))

    x = torch.from_numpy(synth.images_f32(2, 0))
    taps = {}
    hooks = [getattr(model, name).register_forward_hook(lambda m, i, o, name=name: taps.__setitem__(name, o.detach().clone()))
             for name in ("sfe", "stage1", "stage2", "stage3", "stage4", "norm", "avgpool")]
    with torch.no_grad():
        logits, emb = model(x)
    for h in hooks:
        h.remove()
    out.update({"seed": np.int64(0), "n": np.int64(2), "emb": emb.numpy(), "logits": logits.numpy()})
    for k, v in taps.items():
        if v.dim() == 4:
            out["tap_" + k] = _sample(v)
        else:
            out["tap_" + k] = v[:, :: max(1, v.shape[1] // 8)].contiguous().numpy() if v.dim() == 3 else v.numpy()
        out["mean_" + k] = np.float64(v.double().mean().item())
        out["absmean_" + k] = np.float64(v.double().abs().mean().item())
    with torch.no_grad():
        _, emb64 = model.double()(x.double())
    model.float()
    rng_e = float(emb.max() - emb.min())
    print("emb range %.3f, fp32 vs float64 of the reference itself: %.2e of range" % (rng_e, float((emb.double() - emb64).abs().max()) / rng_e))

    for seed in RANK_SEEDS:
        xr = torch.from_numpy(synth.images_f32(64, seed))
        with torch.no_grad():
            _, e = model(xr)
        dist = cosine_dist(e, e).numpy()
        arg, gap = _ranks(dist)
        print("rank seed %d: min gap %.2e median %.2e rows under the bar %d" % (seed, gap.min(), np.median(gap), int((gap <= RANK_BAR).sum())))
        if gap.min() > RANK_BAR:
            break
    else:
        raise SystemExit("no image seed leaves every row decided")
    with torch.no_grad():
        _, e64 = model.double()(xr.double())
        d64 = cosine_dist(e64, e64).numpy()
    model.float()
    print("rank set: fp32 vs float64 matrix %.2e, arg-mins moved %d" % (np.abs(dist - d64).max(), int((_ranks(d64)[0] != arg).sum())))
    assert np.array_equal(dist, dist.T), "the reference's cosine_dist matrix is not symmetric bit for bit"
    out.update({"rank_seed": np.int64(seed), "rank_emb": e.numpy(), "rank_cosdist_triu": dist.astype(np.float32)[np.triu_indices(64)], "rank_argmin": arg,
                "rank_gap": gap.astype(np.float32)})
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
