"""Writes tests/golden/pil_resize.npz: what Pillow and torch themselves compute for the evaluation script's transform
(transforms.Resize((H, W)) on an RGB PIL image -> ToTensor -> Normalize, reid/data_transforms.py:56-127), the ground truth of
tests/pil_resize_ref.py and through it of the *_images_u8 entry points.

    python tools/gen_golden_pil_resize.py          (needs PIL and torch; no GPU)

Contents
    n_small, src_<i>, u8_<i>, f32_<i>, out_<i>   small cases in full: a random uint8 source [h][w][3] of at most 64 px per side (stored), PIL's
                                      Image.resize((W, H), BILINEAR) of it, and torch's to(float32).div(255).sub_(mean).div_(std) of
                                      that in CHW with the ImageNet values; out_<i> = (H, W)
    custom_ms, f32_custom_0           case 0 normalised with another mean / std
    large_hw, large_out, large_salt, large_sha   the 13 x 3 large cases: source sizes, output sizes and the SHA-256 of PIL's output bytes.  The
                                      sources are tests/pil_resize_ref.formula_image(h, w, large_salt[i]): a stated integer
                                      formula with saturated first / last rows and columns (0 and 255), no RNG stream
    table                             the [3][256] ImageNet table from torch
    pillow, torch                     the versions that wrote the file
"""
import hashlib
import os
import sys

import numpy as np
import PIL
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pil_resize_ref as ref  # noqa: E402

# (source h, w) -> (H, W): both axes shrinking by a non-integer factor, growing, mixed, one axis only, identity, 1 x 1, an odd prime size
SMALL = (((64, 48), (16, 8)), ((37, 23), (24, 24)), ((5, 7), (32, 16)), ((64, 64), (32, 16)), ((1, 1), (16, 8)), ((20, 64), (24, 24)),
         ((16, 8), (16, 8)), ((33, 8), (16, 8)), ((61, 59), (24, 24)), ((3, 64), (32, 16)))
CUSTOM_MS = (0.5, 0.4, 0.3, 0.25, 0.2, 0.3)


def pil_resize(src, out_h, out_w):
    return np.asarray(Image.fromarray(src, "RGB").resize((out_w, out_h), Image.BILINEAR))


def torch_norm(u8, mean_std):
    t = torch.from_numpy(np.array(u8)).permute(2, 0, 1).to(torch.float32).div(255)     # ToTensor
    mean = torch.tensor(mean_std[:3], dtype=torch.float32)[:, None, None]
    std = torch.tensor(mean_std[3:], dtype=torch.float32)[:, None, None]
    return t.sub_(mean).div_(std).numpy()                                                           # Normalize


def main():
    rng = np.random.RandomState(20260)
    out = {"n_small": np.int64(len(SMALL)), "custom_ms": np.asarray(CUSTOM_MS, np.float32), "pillow": np.array(PIL.__version__),
           "torch": np.array(torch.__version__)}
    for i, ((h, w), (oh, ow)) in enumerate(SMALL):
        src = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        if i % 3 == 0:                       # hard edges: where truncation, the missing rounding between the passes and the order show
            src[rng.rand(h, w) < 0.3] = 255
            src[rng.rand(h, w) < 0.3] = 0
        u8 = pil_resize(src, oh, ow)
        out["src_%d" % i], out["u8_%d" % i], out["f32_%d" % i] = src, u8, torch_norm(u8, ref.IMAGENET_MEAN_STD)
        out["out_%d" % i] = np.asarray((oh, ow), np.int32)
    out["f32_custom_0"] = torch_norm(out["u8_0"], CUSTOM_MS)
    hw, osz, salt, sha = [], [], [], []
    for si, (h, w) in enumerate(ref.SOURCES):
        src = ref.formula_image(h, w, si)
        for oh, ow in ref.OUT_SIZES:
            hw.append((h, w))
            osz.append((oh, ow))
            salt.append(si)
            sha.append(hashlib.sha256(pil_resize(src, oh, ow).tobytes()).hexdigest())
    out["large_hw"], out["large_out"], out["large_sha"] = np.asarray(hw, np.int32), np.asarray(osz, np.int32), np.array(sha)
    out["large_salt"] = np.asarray(salt, np.int32)
    v = torch.arange(256, dtype=torch.uint8)
    ms = ref.IMAGENET_MEAN_STD
    out["table"] = torch.stack([v.to(torch.float32).div(255).sub_(ms[c]).div_(ms[3 + c]) for c in range(3)]).numpy()
    path = os.path.join(ROOT, "tests", "golden", "pil_resize.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes, %d small and %d large cases, Pillow %s, torch %s" % (path, os.path.getsize(path), len(SMALL), len(sha), PIL.__version__,
                                                                               torch.__version__))


if __name__ == "__main__":
    main()
