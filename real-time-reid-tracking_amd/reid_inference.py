"""The evaluation script's chain on the device - counterpart of reid/image_reid_inference.py (SURVEY.md section 8c,
"Python harness row"), for the seres18 / cares18 / emares18 `.pt` path without side information (``arch="seres18"``, the default) and
for the script's ``--backbone swin_v1 | swin_v2`` (:145-152, :202-208; ``arch="swin"``), with ``--sie`` as ``use_side``.

Reference flow (reid/image_reid_inference.py):
  :78-135   inference_efficient   model(cat(img, flipped img)) -> cat(normalize(emb), normalize(logits)), the two halves apart
  :252-253  gallery  = normalize((plain + mirrored) / 2)          (:267-268 the same for the queries)
  :270-276  merged   = cat(gallery, query); diminish_camera_bias(merged, merged_cams)
  :284-286  dists    = compute_jaccard_distance(merged); dists[dists < 0] = 0
  :290-305  DBSCAN(eps, min_samples=min(10, num_gallery_cams + 1), metric="precomputed") -> pseudo labels
  :308-312  merged_seqs = merged_seqs * num_labels + pseudo; smooth_tracklets(merged, merged_seqs, pseudo != -1)
  :314-322  evaluate_all(query part, ..., gallery part, ...)

Here every link is one C-ABI call on device-resident data: the [ng + nq, 512 + num_class] descriptor matrix is written by
``reid_descriptor_f32_nchw_dev`` straight into its gallery / query row ranges, de-biased, re-ranked, smoothed and evaluated
in place (``reid_cam_debias_dev`` -> ``reid_rerank_jaccard_dev`` -> ``reid_smooth_tracklets_dev`` -> ``reid_rank_eval_dev``)
without a host round trip between links.  The one exception is the reference's own: DBSCAN is scikit-learn (or cuML) on the
host there (`dists.cpu().numpy()`, :297) and stays a host call here - clustering is outside the hot path -
so the Jaccard matrix is downloaded once for it; ``cluster_fn`` replaces it.  Images enter as float32 [n,3,256,128] after the
caller's transform, or as uint8 [h,w,3] arrays of any sizes as the dataset stores them: then the script's transform itself (PIL's
antialiased ``Resize``, ``ToTensor``, ``Normalize``, data_transforms.py:56-127) runs on the device, bit for bit
(``reid_descriptor_images_u8`` / ``reid_swin_descriptor_images_u8``).

With ``arch="swin"`` the descriptor link is ``reid_swin_descriptor_f32_nchw_dev``: images are float32 [n,3,h,w] with h, w multiples of
224 (the script resizes to 448x224, data_transforms.py:78-84), a row is [normalize(logits) | normalize(x_norm)] - the Swin returns
(logits, x_norm), swin_transformer.py:422-423 - and is num_class + 96 wide (``reid_swin_dims``); every later link takes that width as it
is.  ``use_side`` hands the cameras over as the view indices of both views (inference_efficient :117-120, model(img, cam.repeat(2))).

The two remaining links of the script's Market-1501 run are keywords of ``evaluate_reid``: ``strong_inference`` / ``strong_offsets`` make
the second view of the ResNet family the shifted mirror of get_inference_transforms_flipped(strong_inference=True)
(data_transforms.py:130-191, image_reid_inference.py:179-181; ``reid_descriptor_f32_nchw_shift_dev`` /
``reid_descriptor_images_u8_shift``), and ``attribute_dist`` adds the attribute distance (:276-289, tricks.py) to the device Jaccard
matrix before its one download (``reid_distmat_add_l2_dev``).
"""
import os

import numpy as np

from .engine import IMG_H, IMG_W, Engine, check_hw, get_engine, hw_f16_gate, hw_sib_f16_gate
from .parallel import DevArray


def dbscan_pseudo_labels(dists, eps=0.5, min_samples=5):
    """image_reid_inference.py:299-305 (the sklearn branch): DBSCAN on the precomputed distance matrix, on the host."""
    from sklearn.cluster import DBSCAN
    return DBSCAN(eps=eps, min_samples=min_samples, metric="precomputed", n_jobs=-1).fit_predict(dists)


ARCHS = ("seres18", "swin", "seres18_hw", "cares18_hw")
EMA_ARCH = "emares18_hw"
HW_ARCHS = ("seres18_hw", "cares18_hw", EMA_ARCH)
# "seres18_hw": the ResNet path at the images' own size - the script's --dataset veri runs the ResNet family at
# Resize((224, int(ratio * 224))), ratio the mean width / height of the dataset (data_transforms.py:121, image_reid_inference.py:169-180).
# Float images carry the size, uint8 images are resized to ``size`` (required); seres18_ibn weights, exact fp32 (reid_*_hw).  The default
# "seres18" stays fixed at 256 x 128, every architecture of the family and every precision mode.
# "cares18_hw": the same with cares18_ibn weights (the script's --backbone cares18): Engine.set_hw_siblings(True) for the call, restored after it.
# "emares18_hw": the same with emares18_ibn weights, accepted only together with the keyword hw_ema=True (_keyword_gates): Engine.set_hw_ema(True)
# for the call, restored after it.  Without the keyword the name is refused like any unknown one, so it is not in ARCHS.


def _keyword_gates(arch, hw_ema, hw_sib_f16, hw_f16, hw_precision):
    """The any-size keywords of one call against ``arch`` (ValueError, before any device call): arch="emares18_hw" and hw_ema=True come
    together or not at all; hw_sib_f16=True belongs to arch="cares18_hw" / "emares18_hw" and goes without hw_precision and hw_f16;
    hw_f16=True belongs to arch="seres18_hw" and replaces hw_precision.  Returns (hw_sib_f16, hw_f16) as bools."""
    on = bool(Engine.hw_ema_value(hw_ema))
    if arch == EMA_ARCH and not on:
        raise ValueError("arch must be one of %s, got %r (the keyword hw_ema=True enables arch=%r)" % (ARCHS, arch, EMA_ARCH))
    if on and arch != EMA_ARCH:
        raise ValueError("hw_ema belongs to arch=%r; arch=%r takes none" % (EMA_ARCH, arch))
    sib_f16 = hw_sib_f16_gate(hw_sib_f16, hw_precision, hw_f16, arch in ("cares18_hw", EMA_ARCH), "hw_sib_f16 belongs to arch='cares18_hw' / "
                              "'emares18_hw' (arch='seres18_hw': hw_f16); arch=%r takes none" % (arch,), "the call")
    f16 = hw_f16_gate(hw_f16, hw_precision, arch == "seres18_hw", "hw_f16 belongs to arch='seres18_hw' (the fp16-storage any-size forward "
                      "serves seres18_ibn only); arch=%r takes none" % (arch,), "arch='seres18_hw'")
    return sib_f16, f16


def _check_hw_precision(arch, hw_precision):
    """The keyword hw_precision belongs to the *_hw archs and takes Engine.set_hw_precision's values (ValueError, before any device call)."""
    if hw_precision is not None:
        if arch not in HW_ARCHS:
            raise ValueError("hw_precision is the arithmetic of arch='seres18_hw' / 'cares18_hw' / 'emares18_hw'; arch=%r takes none" % (arch,))
        Engine.hw_precision_value(hw_precision)


def _descriptor_width(engine, arch):
    """Width of a descriptor row of ``arch`` on this engine; ValueError for an unknown arch or weights without a classifier."""
    if arch not in ARCHS and arch != EMA_ARCH:              # "emares18_hw" has passed _keyword_gates where this is reached
        raise ValueError("arch must be one of %s, got %r" % (ARCHS, arch))
    if arch == "swin":
        nc, dim = getattr(engine, "swin_num_class", 0), getattr(engine, "swin_dim", 0)
        if nc <= 0 or dim <= 0:
            raise ValueError("arch='swin' needs Swin weights with a classifier on the engine (Engine.load_swin)")
        return dim + nc
    return engine.embed_dim + engine.num_class


def _check_images(images, arch):
    images = np.asarray(images)
    if arch == "swin":
        if images.ndim != 4 or images.shape[1] != 3 or images.shape[2] <= 0 or images.shape[3] <= 0 or images.shape[2] % 224 or \
                images.shape[3] % 224:
            raise ValueError("images must be float32 [n,3,h,w] with h, w multiples of 224, got %s" % (images.shape,))
    elif arch in HW_ARCHS:
        if images.ndim != 4 or images.shape[1] != 3:
            raise ValueError("images must be float32 [n,3,h,w], got %s" % (images.shape,))
        check_hw(images.shape[2:])
    elif images.ndim != 4 or images.shape[1:] != (3, IMG_H, IMG_W):
        raise ValueError("images must be float32 [n,3,%d,%d], got %s" % (IMG_H, IMG_W, images.shape))
    return images


def is_u8_images(images):
    """True for images handed over as the dataset stores them: a list / tuple of uint8 [h,w,3] arrays of any sizes, or one uint8
    [n,h,w,3] array.  Everything else is the float path's business."""
    if isinstance(images, np.ndarray):
        return images.dtype == np.uint8
    if isinstance(images, (list, tuple)):
        return len(images) > 0 and all(getattr(im, "dtype", None) == np.uint8 for im in images)
    return False


def _check_u8_images(images, arch, size):
    """uint8 HWC images of any sizes and the (H, W) they are resized to -> (list of arrays, (H, W)); ValueError before any device call."""
    if arch == "swin":
        h, w, _ = Engine._swin_crop_args((448, 224) if size is None else size, None)
    elif arch in HW_ARCHS:
        if size is None:
            raise ValueError("arch='%s' resizes uint8 images to size=(H, W), which must be given" % arch)
        h, w = check_hw(size)
    else:
        if size is not None and tuple(int(v) for v in size) != (IMG_H, IMG_W):
            raise ValueError("arch=%r resizes to (%d, %d) only, got size %r" % (arch, IMG_H, IMG_W, size))
        h, w = IMG_H, IMG_W
    out = []
    for i, im in enumerate(images):
        im = np.asarray(im)
        if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3 or im.shape[0] < 1 or im.shape[1] < 1:
            raise ValueError("image %d must be uint8 [h,w,3], got %s %s" % (i, im.dtype, im.shape))
        if max(im.shape[:2]) > Engine.PIL_MAX_SIDE:
            raise ValueError("image %d is %d x %d, a source side may be %d at most" % (i, im.shape[0], im.shape[1], Engine.PIL_MAX_SIDE))
        out.append(im)
    return out, (h, w)


def _inference_u8(engine, images, d_out, flip, bs, arch, view_index, size, width, strong_offsets=None, pad=10):
    """The uint8 path of inference_efficient: batches of ``bs`` images through the *_images_u8 entries, whose rows (about 5 KB per
    image) are copied into the device matrix."""
    n = len(images)
    for i in range(0, n, bs):
        part = images[i:i + bs]
        if arch == "swin":
            if view_index is not None:
                engine.set_side_index(view_index[i:i + bs])
            rows = engine.swin_descriptor_images_u8(part, size=size, flip_tta=flip)
        elif strong_offsets is not None:
            rows = engine.descriptor_images_u8_shift(part, strong_offsets[i:i + bs], pad=pad, size=size if arch in HW_ARCHS else None)
        elif arch in HW_ARCHS:
            rows = engine.descriptor_images_u8(part, flip_tta=flip, size=size)
        else:
            rows = engine.descriptor_images_u8(part, flip_tta=flip)
        engine.h2d(d_out + i * width * 4, rows)
    engine.sync()
    return n


def _check_strong(arch, flip, strong_offsets, n, pad):
    """The strong_inference keywords, checked before any device call: the ResNet family only (the script gives the Swin the plain
    mirror), with the mirrored view on, pad in 0 .. 32 and every (top, left) in [0, 2 pad] -> (int32 [n, 2], pad)."""
    if arch == "swin":
        raise ValueError("strong_inference / strong_offsets are the ResNet family's second view; the script gives arch='swin' the plain mirror")
    if not flip:
        raise ValueError("strong_inference / strong_offsets shift the mirrored view: flip must be on")
    return Engine.check_shift(strong_offsets, n, pad)


def inference_efficient(engine, images, d_out, flip=True, bs=1024, arch="seres18", view_index=None, size=None, hw_precision=None,
                        strong_offsets=None, pad=10, hw_ema=False, hw_f16=False, hw_sib_f16=False):
    """Descriptors of ``images`` (float32 [n,3,256,128], host) into the device rows ``d_out`` (pointer to [n, 512 + num_class]
    fp32): upload in batches of ``bs`` images, one ``reid_descriptor_f32_nchw_dev`` per batch.  Unlike the reference function
    (:78-135) the plain / mirrored halves are averaged and renormalised here already (:252-253).

    ``arch="swin"``: images float32 [n,3,h,w], h, w multiples of 224, rows [n, num_class + 96] through
    ``reid_swin_descriptor_f32_nchw_dev``; ``view_index`` (one per image; ``arch="swin"`` only) is the side index of both views.

    ``images`` may instead be a sequence of uint8 [h,w,3] arrays of any sizes (or one uint8 [n,h,w,3] array): the script's transform -
    PIL's antialiased Resize, ToTensor, Normalize with the ImageNet values - then runs on the device (``reid_descriptor_images_u8``,
    to 256x128; ``reid_swin_descriptor_images_u8`` to ``size`` = (H, W), default (448, 224)), with rows bit-identical to the float path
    on the same images preprocessed with PIL on the host.  ``size`` is for uint8 images only.

    ``arch="seres18_hw"``: the ResNet path at another input size - float32 [n,3,h,w] with sides in 32 .. 512, or uint8 images resized to
    ``size`` = (H, W) (required), e.g. the script's VeRi geometry ``size=(224, int(ratio * 224))``; seres18_ibn weights with the context in
    exact fp32 (``reid_descriptor_f32_nchw_hw_dev`` / ``reid_descriptor_images_u8_hw``), or - ``hw_precision`` "f32" / "f16x3"
    (``Engine.set_hw_precision``) - in the arithmetic named, whatever the context's mode: set for this call and restored after it; None
    leaves the engine's setting alone.  ``arch="cares18_hw"``: the same entries on cares18_ibn weights (the script's --backbone cares18 with
    --dataset veri), ``Engine.set_hw_siblings(True)`` for this call and restored after it.  ``arch="emares18_hw"`` with ``hw_ema=True`` (the
    name alone is refused like an unknown one): the same entries on emares18_ibn weights, ``Engine.set_hw_ema(True)`` for this call and
    restored after it.

    ``strong_offsets``: int [n, 2] of (top, left) per image with ``pad`` (data_transforms.strong_inference_offsets): the second view is the
    script's strong_inference one - the mirror shifted by (top - pad, left - pad) over a black border, black being (0 - mean) / std of the
    ImageNet values (``reid_descriptor_f32_nchw_shift_dev`` / ``reid_descriptor_images_u8_shift``).  ``arch="swin"`` takes none: the
    script gives the Swin the plain mirror.  None is today's call and bits.

    ``hw_f16=True`` (``arch="seres18_hw"`` only, and instead of ``hw_precision``: both together are a ValueError): the any-size forward runs
    in fp16 storage with fp32 accumulation - ``Engine.set_hw_f16(True)`` for this call and restored after it.  ``hw_sib_f16=True``
    (``arch="cares18_hw"`` / ``"emares18_hw"`` only - the latter still with ``hw_ema=True`` -, without ``hw_precision`` and ``hw_f16``): the
    same for the siblings, ``Engine.set_hw_sib_f16(True)`` for this call and restored after it."""
    sib_f16, f16 = _keyword_gates(arch, hw_ema, hw_sib_f16, hw_f16, hw_precision)
    _check_hw_precision(arch, hw_precision)
    if strong_offsets is not None:
        strong_offsets, pad = _check_strong(arch, flip, strong_offsets, len(images), pad)
    width = _descriptor_width(engine, arch)
    u8 = is_u8_images(images)
    if u8:
        images, size = _check_u8_images(images, arch, size)
        n = len(images)
    else:
        if size is not None:
            raise ValueError("size is the resize target of uint8 images; float images carry their own")
        images = _check_images(images, arch)
        n = images.shape[0]
    if int(bs) < 1:
        raise ValueError("bs must be at least 1, got %r" % (bs,))
    if view_index is not None:
        if arch != "swin":
            raise ValueError("view_index is the Swin's side information; arch=%r takes none here" % (arch,))
        view_index = np.asarray(view_index).reshape(-1)
        if view_index.shape[0] != n or (n and (view_index.min() < 0 or view_index.max() >= 2 ** 31)):
            raise ValueError("view_index must hold one non-negative index per image (%d), got %d" % (n, view_index.shape[0]))
        view_index = view_index.astype(np.int32)
    if hw_precision is not None or f16 or arch in ("cares18_hw", EMA_ARCH):   # every argument is checked: the settings go on for the device work and off after it
        with Engine.hw_scope(engine, precision=hw_precision, siblings=True if arch == "cares18_hw" else None, ema=True if arch == EMA_ARCH else None,
                             f16=f16 or None, sib_f16=sib_f16 or None):
            return inference_efficient(engine, images, d_out, flip, bs, "seres18_hw", view_index, size if u8 else None,
                                       strong_offsets=strong_offsets, pad=pad)
    if u8:
        return _inference_u8(engine, images, d_out, flip, int(bs), arch, view_index, size, width, strong_offsets, pad)
    fill = None
    if strong_offsets is not None:
        fill = Engine.normalised_zero_fill()
    stage = DevArray(engine, (min(bs, max(n, 1)),) + images.shape[1:], np.float32)
    try:
        for i in range(0, n, bs):
            part = np.ascontiguousarray(images[i:i + bs], np.float32)
            engine.h2d(stage.ptr, part)
            if arch == "swin":
                if view_index is not None:
                    engine.set_side_index(view_index[i:i + bs])
                engine.swin_descriptor_dev(stage.ptr, part.shape[0], part.shape[2], part.shape[3], flip, d_out + i * width * 4)
            elif strong_offsets is not None:
                engine.descriptor_shift_dev(stage.ptr, part.shape[0], part.shape[2:], strong_offsets[i:i + bs], pad, fill, d_out + i * width * 4)
            elif arch in HW_ARCHS:
                engine.descriptor_dev(stage.ptr, part.shape[0], flip, d_out + i * width * 4, size=part.shape[2:])
            else:
                engine.descriptor_dev(stage.ptr, part.shape[0], flip, d_out + i * width * 4)
        engine.sync()
    finally:
        stage.free()
    return n


def evaluate_reid(gallery_images, gallery_labels, gallery_cams, gallery_seqs, query_images, query_labels, query_cams,
                  query_seqs, num_gallery_cams=None, eps=0.5, la=0.05, k1=20, k2=6, flip=True, cluster_fn=None, taps=None,
                  verbose=True, device=0, engine=None, arch="seres18", use_side=False, size=None, hw_precision=None,
                  strong_inference=False, strong_offsets=None, attribute_dist=None, pad=10, hw_ema=False, hw_f16=False, hw_sib_f16=False):
    """(CMC float32 [ng], mAP float) of the script's chain for one gallery / query pair; weights must be loaded on the engine
    (``Engine.load_seres18`` / ``build_model``).  ``taps`` (a dict) receives host copies of the intermediates the
    reference-generated fixture holds: "desc", "debiased", "jaccard", "pseudo_labels", "smoothed".
    ``cluster_fn(dists float32 [N,N]) -> int labels [N]`` (-1 = noise) replaces the DBSCAN call.
    ``arch="swin"``: the chain on the loaded Swin weights (``Engine.load_swin``), images float32 [n,3,h,w] with h, w multiples of 224;
    ``use_side`` (the script's --sie, ``arch="swin"`` only) passes each image's camera as the view index of both its views.
    Gallery and query images may each be a sequence of uint8 [h,w,3] arrays of any sizes instead (see ``inference_efficient``); ``size``
    = (H, W) is what a Swin resizes them to (default (448, 224); the ResNet family is fixed at 256x128 unless ``arch="seres18_hw"``, which
    runs seres18_ibn weights in exact fp32 at the float images' own size or at ``size``: VeRi is ``size=(224, int(ratio * 224))``;
    ``hw_precision`` "f32" / "f16x3" names that forward's arithmetic for this call - ``Engine.set_hw_precision``, restored afterwards - and
    None leaves the engine's setting alone; ``arch="cares18_hw"`` is the same for cares18_ibn weights, with ``Engine.set_hw_siblings(True)``
    for the call, and ``arch="emares18_hw"`` together with ``hw_ema=True`` for emares18_ibn weights, with ``Engine.set_hw_ema(True)`` for the
    call; without that keyword the name is refused).
    ``strong_inference`` / ``strong_offsets``: the script's second view for the ResNet family (--backbone seres18 / cares18,
    image_reid_inference.py:179-181) - the mirror shifted by up to +-``pad`` pixels on each axis over a black border.
    ``strong_offsets`` is int [ng + nq, 2] of (top, left) per image, gallery first; ``strong_inference=True`` without offsets draws them
    (data_transforms.strong_inference_offsets, torch's global generator).  Either with ``arch="swin"`` is a ValueError: the script gives
    the Swin the plain mirror.  ``attribute_dist``: the Market-1501 term (:276-289) - an [N, 30] array of already looked-up attribute rows
    (gallery first), or a ``(labels, mat_path)`` pair for tricks.attribute_rows; the rows are normalised on the host, uploaded and
    euclidean_dist(rows, rows) is added to the device Jaccard matrix (``reid_distmat_add_l2_dev``) before its download.
    ``taps["jaccard"]`` stays the matrix before the add; ``taps["dists"]`` is the one handed to DBSCAN / ``cluster_fn``.  With these
    keywords left out the call and its bits are what they were.  ``hw_f16=True`` (``arch="seres18_hw"`` only, instead of ``hw_precision``):
    the descriptors come from the fp16-storage any-size forward, ``Engine.set_hw_f16(True)`` for the call.  ``hw_sib_f16=True``
    (``arch="cares18_hw"`` / ``"emares18_hw"`` only, without ``hw_precision`` and ``hw_f16``): the same for the siblings,
    ``Engine.set_hw_sib_f16(True)`` for the call."""
    _keyword_gates(arch, hw_ema, hw_sib_f16, hw_f16, hw_precision)
    if strong_inference or strong_offsets is not None:
        n_all = len(gallery_labels) + len(query_labels)
        if strong_offsets is None:
            from .data_transforms import strong_inference_offsets
            _check_strong(arch, flip, np.zeros((n_all, 2), np.int32), n_all, pad)     # arch, flip and pad, before anything is drawn
            strong_offsets = strong_inference_offsets(n_all, pad)
        strong_offsets, pad = _check_strong(arch, flip, strong_offsets, n_all, pad)
    attr_rows = None
    if attribute_dist is not None:
        from . import tricks
        if isinstance(attribute_dist, tuple) and len(attribute_dist) == 2 and isinstance(attribute_dist[1], (str, os.PathLike)):
            attr_rows = tricks.attribute_rows(attribute_dist[0], attribute_dist[1])
        else:
            attr_rows = np.asarray(attribute_dist, np.float32)
        if attr_rows.ndim != 2 or attr_rows.shape[0] != len(gallery_labels) + len(query_labels) or not 1 <= attr_rows.shape[1] <= 32:
            raise ValueError("attribute_dist must give one row of 1 .. 32 attributes per image (%d, gallery first), got %s"
                             % (len(gallery_labels) + len(query_labels), attr_rows.shape))
        attr_rows = tricks.normalize_rows(attr_rows)
    _check_hw_precision(arch, hw_precision)
    if arch not in ARCHS and arch != EMA_ARCH:
        raise ValueError("arch must be one of %s, got %r" % (ARCHS, arch))
    if use_side and arch != "swin":
        raise ValueError("use_side is the Swin's side information (--sie); arch=%r takes none here" % (arch,))
    eng = engine or get_engine(device)
    gl, gc, gs = (np.ascontiguousarray(a, np.int64).reshape(-1) for a in (gallery_labels, gallery_cams, gallery_seqs))
    ql, qc, qs = (np.ascontiguousarray(a, np.int64).reshape(-1) for a in (query_labels, query_cams, query_seqs))
    ng, nq = len(gl), len(ql)
    if len(gallery_images) != ng or len(query_images) != nq or ng < 1 or nq < 1:
        raise ValueError("images and labels disagree: %d/%d gallery, %d/%d query" % (len(gallery_images), ng, len(query_images), nq))
    u8 = [is_u8_images(gallery_images), is_u8_images(query_images)]
    if size is not None and not any(u8):
        raise ValueError("size is the resize target of uint8 images; float images carry their own")
    gallery_images, query_images = (_check_u8_images(im, arch, size)[0] if is_u8 else _check_images(im, arch)
                                    for im, is_u8 in zip((gallery_images, query_images), u8))
    n, width = ng + nq, _descriptor_width(eng, arch)
    merged = DevArray(eng, (n, width), np.float32)
    dists = DevArray(eng, (n, n), np.float32)
    try:
        strong = {} if strong_offsets is None else {"pad": pad}
        inference_efficient(eng, gallery_images, merged.ptr, flip, arch=arch, view_index=gc if use_side else None, size=size if u8[0] else None,
                            hw_precision=hw_precision, hw_ema=hw_ema, hw_f16=hw_f16, hw_sib_f16=hw_sib_f16, **(strong and dict(strong, strong_offsets=strong_offsets[:ng])))
        inference_efficient(eng, query_images, merged.row_ptr(ng), flip, arch=arch, view_index=qc if use_side else None,
                            size=size if u8[1] else None, hw_precision=hw_precision, hw_ema=hw_ema, hw_f16=hw_f16, hw_sib_f16=hw_sib_f16,
                            **(strong and dict(strong, strong_offsets=strong_offsets[ng:])))
        if taps is not None:
            taps["desc"] = merged.numpy()
        merged_cams = np.concatenate([gc, qc]).astype(np.int32)
        merged_seqs = np.concatenate([gs, qs])
        eng.cam_debias_dev(merged.ptr, merged_cams, n, width, la)
        if taps is not None:
            taps["debiased"] = merged.numpy()
        eng.rerank_jaccard_dev(merged.ptr, n, width, k1, k2, dists.ptr)     # negatives already clamped (faiss_utils.py:239-240)
        if attr_rows is not None:                                           # dists += attribute_dist (:288-289), on the device
            if taps is not None:
                taps["jaccard"] = dists.numpy()
            d_attr = DevArray(eng, attr_rows.shape, np.float32)
            try:
                eng.h2d(d_attr.ptr, attr_rows)
                eng.distmat_add_l2_dev(d_attr.ptr, n, attr_rows.shape[1], dists.ptr)
                eng.sync()
            finally:
                d_attr.free()
        host_dists = dists.numpy()                                          # the reference's dists.cpu().numpy() (:297)
        if taps is not None:
            if attr_rows is None:
                taps["jaccard"] = host_dists
            taps["dists"] = host_dists
        cams = int(num_gallery_cams) if num_gallery_cams is not None else int(gc.max()) + 1
        cluster = cluster_fn or (lambda dd: dbscan_pseudo_labels(dd, eps, min(10, cams + 1)))
        pseudo = np.asarray(cluster(host_dists)).astype(np.int64).reshape(-1)
        if pseudo.shape[0] != n:
            raise ValueError("cluster_fn returned %d labels for %d rows" % (pseudo.shape[0], n))
        num_labels = int(pseudo.max()) + 1
        if taps is not None:
            taps["pseudo_labels"] = pseudo.copy()
        seqs = (merged_seqs * num_labels + pseudo).astype(np.int32)
        eng.smooth_tracklets_dev(merged.ptr, seqs, pseudo != -1, n, width, keep=0.1)
        if taps is not None:
            taps["smoothed"] = merged.numpy()
        cmc_sum, ap, valid = eng.rank_eval_dev(merged.row_ptr(ng), ql, qc, nq, merged.ptr, gl, gc, ng, width)
    finally:
        eng.sync()
        merged.free()
        dists.free()
    total = 0.0
    for i in range(nq):              # python-float accumulation in query order, as the reference does (evaluate.py:41-50)
        if valid[i]:
            total += float(ap[i])
    cmc = cmc_sum.astype(np.float32) / nq
    mean_ap = total / nq
    if verbose:
        print('Rank@1:%f Rank@5:%f Rank@10:%f mAP:%f' % (cmc[0], cmc[min(4, ng - 1)], cmc[min(9, ng - 1)], mean_ap))
    return cmc, mean_ap
