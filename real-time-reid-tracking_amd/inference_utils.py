"""Host mirror of the evaluation script's post-processing on the HIP library.

* ``diminish_camera_bias(embeddings, cams, la=0.05)``   reid/inference_utils.py:5-15
* ``smooth_tracklets(embeddings, seqs, indices_valid)``   reid/inference_utils.py:18-27
* ``extract_descriptors(model_or_engine, images, flip=True)``: what ``inference_efficient`` + the averaging at
  reid/image_reid_inference.py:112-123,252-253 produce for one set of images - ``normalize((d(x) + d(hflip x)) / 2)`` with
  ``d = cat(normalize(emb), normalize(logits))``.  ``images`` is float32 [N,3,H,W] after the caller's transform
  (the script uses ImageNet mean/std, data_transforms.py:56-130).
"""
import numpy as np

from .engine import Engine, check_hw, get_engine, hw_f16_gate, hw_sib_f16_gate


def _np(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def diminish_camera_bias(embeddings, cams, la=0.05, device=0):
    """Returns the de-biased, row-normalised embeddings (same container type as the input; the reference works in place and
    returns its argument).  Camera ids without rows are skipped (the reference's torch.inverse would raise on them)."""
    out = get_engine(device).cam_debias(_np(embeddings), _np(cams), la)
    if hasattr(embeddings, "detach"):
        import torch
        res = torch.from_numpy(out).to(embeddings.dtype)
        embeddings.copy_(res)
        return embeddings
    return out


def smooth_tracklets(embeddings, seqs, indices_valid, device=0):
    """Same arguments as the reference: rows of one tracklet (equal ``seqs``) that are ``indices_valid`` move to
    0.1 * row + 0.9 * tracklet mean.  In place for torch tensors (the reference assigns into its argument) and returned."""
    out = get_engine(device).smooth_tracklets(_np(embeddings), _np(seqs), _np(indices_valid), keep=0.1)
    if hasattr(embeddings, "detach"):
        import torch
        embeddings.copy_(torch.from_numpy(out).to(embeddings.dtype))
        return embeddings
    return out


def extract_descriptors(images, flip=True, device=0, size=None, hw_precision=None, strong_offsets=None, pad=10, hw_f16=False, hw_sib_f16=False):
    """float [n,3,H,W] after the caller's transform ((256, 128), or sides in 32 .. 512 for seres18_ibn weights in exact fp32), or a list
    of uint8 [h,w,3] images of any sizes, which the device resizes as PIL does - to ``size`` = (H, W), default (256, 128); the script's
    VeRi geometry is (224, int(ratio * 224)) - and normalises with the ImageNet values (Engine.descriptor_images_u8).
    ``hw_precision``: the arithmetic of another size for this call (Engine.set_hw_precision: "f32" / "f16x3"), restored afterwards; None
    leaves the engine's setting alone.  ``hw_f16=True`` instead (both together are a ValueError naming them): another size runs
    seres18_ibn in fp16 storage with fp32 accumulation for this call (Engine.set_hw_f16), restored afterwards.  ``hw_sib_f16=True``
    (without ``hw_precision`` and ``hw_f16``: a ValueError naming them otherwise): the same for loaded cares18_ibn / emares18_ibn weights
    (Engine.set_hw_sib_f16), restored afterwards.
    ``strong_offsets``: int [n, 2] of (top, left) per image (data_transforms.strong_inference_offsets) - the second view becomes the
    script's strong_inference one, the mirror shifted by (top - pad, left - pad) over a black border (reid/data_transforms.py:130-191;
    Engine.descriptor_f32_nchw_shift / descriptor_images_u8_shift; needs ``flip``).  None is today's call and bits."""
    if size is not None:
        size = check_hw(size)
    if strong_offsets is not None:
        if not flip:
            raise ValueError("strong_offsets shift the mirrored view: flip must be on")
        strong_offsets, pad = Engine.check_shift(strong_offsets, len(images), pad)   # a bad value raises here, before any device call
    # no architecture to test here (the weights are whatever the engine holds); a bad value raises here, before any device call
    sib_f16 = hw_sib_f16_gate(hw_sib_f16, hw_precision, hw_f16, True, None, "another size")
    f16 = hw_f16_gate(hw_f16, hw_precision, True, None, "another size")
    if hw_precision is not None:
        Engine.hw_precision_value(hw_precision)
    if hw_precision is not None or f16 or sib_f16:      # the setting goes on for the rest of the call and off after it
        with Engine.hw_scope(get_engine(device), precision=hw_precision, f16=f16 or None, sib_f16=sib_f16 or None):
            return extract_descriptors(images, flip, device, size, strong_offsets=strong_offsets, pad=pad)
    if isinstance(images, (list, tuple)) and len(images) and all(getattr(im, "dtype", None) == np.uint8 for im in images):
        if strong_offsets is not None:
            return get_engine(device).descriptor_images_u8_shift(images, strong_offsets, pad=pad, size=size)
        return get_engine(device).descriptor_images_u8(images, flip_tta=flip, size=size)
    images = _np(images)
    if size is not None and tuple(images.shape[2:]) != size:
        raise ValueError("size %r is the resize target of uint8 images; these float images are %s" % (size, tuple(images.shape[2:])))
    if strong_offsets is not None:
        return get_engine(device).descriptor_f32_nchw_shift(images, strong_offsets, pad=pad)
    return get_engine(device).descriptor_f32_nchw(images, flip)
