"""Generates tests/golden/anysize.npz from the REFERENCE's own SERse18_IBN at input sizes other than 256 x 128 (CPU only; run where the
reference tree is).

    python tools/gen_golden_anysize.py [--reference /path/to/reference]

The reference class is built with the stand-ins oracle/gen_golden.py uses (imported from there: the IBN-Net skeleton behind torch.hub.load,
the empty torchvision module) and the seeded weights of tests/golden/seres18_seed0.npz, synth.seres18_state_dict(0), loaded strict=True.
Nothing of the reference is written to the repository: the fixture holds seeds, sizes and numbers its classes produced.  Inputs are
regenerated from the seed: x = preprocess(synth.smooth_crops_u8(n, seed, h, w)), i.e. (v / 255 - 0.5) / 0.5 as NCHW float32.

Cases - the smallest at which each thing can go wrong (key prefix c<k>_):
    (64, 32),   n = 3   final maps 4 x 2: hw = 8, less than a wavefront
    (96, 72),   n = 3   maps 24 x 18, 12 x 9, 6 x 5, 6 x 5: odd widths, a stride-2 convolution on an odd side, no hw a multiple of 64
    (224, 268), n = 2   the evaluation script's VeRi shape, maps 56 x 67 down to 14 x 17
Per case: h, w, n, seed; the eleven stage taps (bn0, pooling0, the eight blocks, avgpooling) as gen_golden._sample takes them plus their
mean and mean absolute value over the whole tensor (tap_ / mean_ / absmean_); emb and logits of the eval-mode forward; desc_plain and
desc_tta, the evaluation script's descriptor cat(normalize(emb), normalize(logits)) of the plain view and
normalize((d(x) + d(hflip x)) / 2) (reid/image_reid_inference.py:112-123, :252-253).
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ((64, 32, 3, 11), (96, 72, 3, 12), (224, 268, 2, 13))     # (h, w, n, seed of the images)
WEIGHT_SEED = 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=None)
    args = ap.parse_args()
    from oracle import gen_golden
    if args.reference:
        gen_golden.REF = args.reference
    gen_golden._install_stubs()
    from reid.backbones.SERes18_IBN import seres18_ibn      # the reference's own class
    from reid_amd import synth
    import torch.nn.functional as F

    sd_np = synth.seres18_state_dict(WEIGHT_SEED)
    model = seres18_ibn(num_classes=751, loss="triplet")
    res = model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd_np.items()}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    model.eval()
    names = ["bn0", "pooling0"] + [b[0] for b in synth.SERES18_BLOCKS] + ["avgpooling"]
    out = {"n_cases": np.int64(len(CASES)), "weight_seed": np.int64(WEIGHT_SEED)}
    for k, (h, w, n, seed) in enumerate(CASES):
        crops = synth.smooth_crops_u8(n, seed, h, w)
        x = torch.from_numpy(crops).float().div(255.0).sub(0.5).div(0.5).permute(0, 3, 1, 2).contiguous()
        taps = {}
        hooks = [getattr(model, name).register_forward_hook(lambda m, i, o, name=name: taps.__setitem__(name, o.detach().clone()))
                 for name in names]
        with torch.no_grad():
            emb, logits = model(x)
        for hk in hooks:
            hk.remove()
        with torch.no_grad():
            emb2, logits2 = model(torch.flip(x, dims=[3]))
        d1 = torch.cat([F.normalize(emb, dim=1), F.normalize(logits, dim=1)], dim=1)
        d2 = torch.cat([F.normalize(emb2, dim=1), F.normalize(logits2, dim=1)], dim=1)
        p = "c%d_" % k
        out.update({p + "h": np.int64(h), p + "w": np.int64(w), p + "n": np.int64(n), p + "seed": np.int64(seed),
                    p + "emb": emb.numpy(), p + "logits": logits.numpy(), p + "desc_plain": d1.numpy(),
                    p + "desc_tta": F.normalize((d1 + d2) / 2, dim=1).numpy()})
        for name, v in taps.items():
            out[p + "tap_" + name] = gen_golden._sample(v)
            out[p + "shape_" + name] = np.asarray(v.shape, np.int64)
            out[p + "mean_" + name] = np.float64(v.double().mean().item())
            out[p + "absmean_" + name] = np.float64(v.double().abs().mean().item())
        print("case %d: %d x %d, n %d, last map %s, |emb| row0 %.4f" % (k, h, w, n, tuple(taps["basicBlock42"].shape[2:]), float(emb[0].norm())))
    path = os.path.join(ROOT, "tests", "golden", "anysize.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
