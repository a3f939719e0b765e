"""The random part of the evaluation script's ``strong_inference`` second view (reid/data_transforms.py:130-191).

``get_inference_transforms_flipped(..., strong_inference=True)`` is ``Resize -> RandomHorizontalFlip(p=1) -> Pad(10) ->
RandomCrop((H, W)) -> ToTensor -> Normalize``: everything but the crop offsets is fixed and runs on the device
(``Engine.descriptor_f32_nchw_shift`` / ``descriptor_images_u8_shift``).  This module draws the offsets.
"""
import numpy as np


def strong_inference_offsets(n, pad=10, generator=None):
    """int32 [n, 2] of (top, left) crop offsets into the padded image, each uniform on 0 .. 2 pad.

    Per image in order, ``top = torch.randint(0, 2 * pad + 1, (1,), generator=generator)`` and then ``left`` the same way: the order of
    torchvision's ``RandomCrop.get_params``, which draws ``i`` (top) from ``h - th + 1`` values and then ``j`` (left) from ``w - tw + 1``
    values, here both 2 pad + 1.  That order is cited from torchvision's source; torchvision is not a dependency of this package and the
    order has not been checked against an installed copy.  ``generator``: a ``torch.Generator`` (None: torch's global one).  Without
    torch the draws come from a numpy ``Generator`` (``generator``, or a fresh ``default_rng()``) - the same distribution, other numbers.

    The script draws inside DataLoader workers, so its own offsets are not reproducible from a seed either: the contract is the
    transform and the distribution, not the script's numbers.  ``pad = 0`` gives zeros (the plain mirror)."""
    n, pad = int(n), int(pad)
    if n < 0 or pad < 0:
        raise ValueError("strong_inference_offsets: n >= 0 and pad >= 0, got n = %d, pad = %d" % (n, pad))
    out = np.zeros((n, 2), np.int32)
    if pad == 0 or n == 0:
        return out
    if isinstance(generator, np.random.Generator):
        torch = None
    else:
        try:
            import torch
        except ImportError:
            torch = None
    if torch is None:
        rng = generator if isinstance(generator, np.random.Generator) else np.random.default_rng()
        for i in range(n):
            out[i, 0] = rng.integers(0, 2 * pad + 1)
            out[i, 1] = rng.integers(0, 2 * pad + 1)
        return out
    for i in range(n):
        out[i, 0] = int(torch.randint(0, 2 * pad + 1, (1,), generator=generator).item())
        out[i, 1] = int(torch.randint(0, 2 * pad + 1, (1,), generator=generator).item())
    return out
