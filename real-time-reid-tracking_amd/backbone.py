"""Backbone objects handed out by ``build_model`` - what the tracker calls as ``model(im_batch)``.

They hold the checkpoint as a plain numpy ``state_dict`` (same keys as the reference's module,
reid/backbones/SERes18_IBN.py:186-248) and a handle to the HIP engine; there is no torch graph and no CPU
forward.  They tolerate the calls the external loader makes on an ``nn.Module``: ``.to(device)``, ``.half()``,
``.eval()``, ``state_dict()`` / ``load_state_dict()``, ``warmup()``.
"""
from collections import OrderedDict

import numpy as np

from . import precision as _precision
from . import synth, weights
from .engine import IMG_H, IMG_W, Engine, check_hw, get_engine, hw_f16_gate, hw_sib_f16_gate


def _device_index(device):
    if device is None:
        return 0
    if isinstance(device, int):
        return device
    s = str(device)
    if s in ("cuda", "gpu", "hip"):
        return 0
    if s.startswith("cuda:"):
        return int(s.split(":")[1])
    if s == "cpu":
        raise RuntimeError("this backbone runs only on an MI355X through libreid_hip.so; there is no CPU path")
    return int(s)


def _copy_matching(dst, src, strict, resizable=()):
    """Copies checkpoint tensors into the held state_dict.  A shape mismatch raises when ``strict`` (as torch does:
    "size mismatch for ..."); otherwise the tensor is skipped with a warning naming it - except the classifier, whose row
    count (num_classes of the training set) is taken from the checkpoint.  Returns the skipped keys."""
    bad = []
    for k, v in src.items():
        if k not in dst:
            continue
        v = np.asarray(v)
        if tuple(dst[k].shape) == tuple(v.shape):
            dst[k] = v.astype(dst[k].dtype)
        elif k in resizable and v.ndim == dst[k].ndim and v.shape[1:] == dst[k].shape[1:]:
            dst[k] = v.astype(dst[k].dtype)             # a checkpoint trained with another number of identities
        else:
            bad.append("%s: checkpoint %s vs model %s" % (k, tuple(v.shape), tuple(dst[k].shape)))
    if bad:
        if strict:
            raise RuntimeError("Error(s) in loading state_dict: size mismatch for " + "; ".join(bad[:5]))
        import warnings
        warnings.warn("load_state_dict(strict=False): skipped tensors with another shape (seeded values kept): " + "; ".join(bad))
    return [b.split(":")[0] for b in bad]


def _torch_cuda_forward(x, embed_dev, engine, out_dims):
    """CUDA tensor in -> CUDA tensors out, no host round trip: the device entry point runs on ``x.data_ptr()`` on torch's
    current stream of that device (the yolov8_tracking multibackend hands the model CUDA batches every frame)."""
    import torch
    xf = x.detach()
    if xf.dtype != torch.float32 or not xf.is_contiguous():
        xf = xf.float().contiguous()
    with torch.cuda.device(xf.device), engine.on_torch_stream():
        outs = [torch.empty((xf.shape[0], d), dtype=torch.float32, device=xf.device) for d in out_dims]
        embed_dev(xf, outs)
    return outs


def _index_array(index, n):
    """cam / view_index argument (sequence, numpy array or torch tensor, one entry per image) -> int32[n]."""
    a = index.detach().cpu().numpy() if hasattr(index, "detach") else np.asarray(index)
    a = a.reshape(-1).astype(np.int64)
    if a.shape[0] != n:
        raise ValueError("expected one index per image (%d), got %d" % (n, a.shape[0]))
    return a.astype(np.int32)


class SERes18IBN:
    """ResNet18-IBN-a + SE + GeM + BNNeck ("ResNet18-SE"), eval mode only.

    ``model(x)`` -> embedding [N,512] = BNNeck output; ``model(x, return_logits=True)`` ->
    (embedding, logits[N,num_classes]) like the reference's eval-mode tuple (SERes18_IBN.py:274-275).
    ``x``: float32/float16 [N,3,256,128] NCHW, normalised - numpy array or torch tensor; the result has the
    type (and, for torch, the device) of the input.  Inputs [N,3,H,W] of another size (sides 32 .. 512) run the any-size forward in exact
    fp32, with ``hw_precision="f16x3"`` in the fp32-class arithmetic, or with ``hw_f16=True`` in fp16 storage with fp32 accumulation
    (libreid_hip_anysize_f16.so); the engine's settings come back after the call.
    """

    embed_dim = 512
    arch = "seres18_ibn"

    def __init__(self, num_classes=751, loss="triplet", pretrained=False, use_gpu=True, seed=0, num_cams=6, cam_factor=-1.0,
                 precision=None, hw_precision=None, hw_siblings=False, hw_ema=False, hw_f16=False, hw_sib_f16=False, **_):
        if loss not in ("triplet", "softmax"):
            raise NotImplementedError                      # seres18_ibn(), SERes18_IBN.py:279-285
        self._mode = _precision.resolve(precision)         # "f16x3" unless the argument or $REID_PRECISION says otherwise (precision.py)
        # inputs of another size (seres18_ibn only): None = exact fp32 for that call, "f16x3" = the fp32-class arithmetic for that call
        hw = Engine.hw_precision_value(hw_precision)
        # cares18_ibn only: True = inputs of another size run too (Engine.set_hw_siblings around such a call)
        self._hw_siblings = bool(Engine.hw_siblings_value(hw_siblings))
        if self._hw_siblings and self.arch != "cares18_ibn":
            raise ValueError("%s has no hw_siblings argument (cares18_ibn only)" % self.arch)
        # emares18_ibn only: True = inputs of another size run too (Engine.set_hw_ema around such a call)
        self._hw_ema = bool(Engine.hw_ema_value(hw_ema))
        if self._hw_ema and self.arch != "emares18_ibn":
            raise ValueError("%s has no hw_ema argument (emares18_ibn only)" % self.arch)
        # seres18_ibn only: True = inputs of another size run in fp16 storage with fp32 accumulation (Engine.set_hw_f16 around such a call)
        self._hw_f16 = hw_f16_gate(hw_f16, hw_precision, self.arch == "seres18_ibn", "%s has no hw_f16 argument (seres18_ibn only)" % self.arch,
                                   "inputs of another size")
        # cares18_ibn / emares18_ibn only: True = inputs of another size run in fp16 storage with fp32 accumulation (Engine.set_hw_sib_f16
        # around such a call); the keyword alone is enough, hw_siblings / hw_ema need not be given
        self._hw_sib_f16 = hw_sib_f16_gate(hw_sib_f16, hw_precision, hw_f16, self.arch != "seres18_ibn",
                                           "seres18_ibn has no hw_sib_f16 argument (cares18_ibn and emares18_ibn only; seres18_ibn: hw_f16)",
                                           "inputs of another size")
        self._hw_call = _HwClassCall(self) if hw == 2 else None
        self.num_classes = num_classes
        self.num_cams, self.cam_factor = num_cams, float(cam_factor)   # SERes18_IBN.py:193,198: cam_bias [num_cams,512] and its factor
        self.is_reid = loss == "softmax"
        self.training = False
        self._device = 0
        # held with SERse18_IBN's named keys; state_dict() hands out the reference's own key layout (positional for the siblings'
        # downsample blocks), load_state_dict() accepts both
        self._sd = weights.normalize_state_dict(synth.seres18_state_dict(seed, num_class=num_classes, num_cams=num_cams, gem_p=3.0,
                                                                         arch=self.arch))
        self._dirty = True
        if pretrained:
            import warnings
            warnings.warn("ImageNet-pretrained IBN-Net weights need torch.hub/network access (SERes18_IBN.py:201); "
                          "keeping the seeded random initialisation")

    # ---- nn.Module-like surface
    def to(self, device=None, *a, **k):
        idx = _device_index(device)
        if idx != self._device:
            self._device, self._dirty = idx, True
        return self

    def cuda(self, device=None):
        return self.to(0 if device is None else device)

    def half(self):
        return self            # fp16 inputs are widened on entry; arithmetic stays fp32

    def float(self):
        return self

    def eval(self):
        self.training = False
        return self

    def train(self, mode=True):
        if mode:
            raise NotImplementedError("inference engine: eval mode only")
        return self

    def parameters(self):
        return iter(())

    def _ref_key(self, k):
        ds = ("basicBlock21", "basicBlock31", "basicBlock41")
        return synth.sibling_key(k) if getattr(self, "arch", "seres18_ibn") != "seres18_ibn" and k.startswith(ds) else k

    def state_dict(self):
        try:
            import torch
            return OrderedDict((self._ref_key(k), torch.from_numpy(np.array(v))) for k, v in self._sd.items())
        except ImportError:
            return OrderedDict((self._ref_key(k), np.array(v)) for k, v in self._sd.items())

    def load_state_dict(self, state_dict, strict=True):
        sd = weights.normalize_state_dict(state_dict)
        missing = [k for k in self._sd if k not in sd]
        unexpected = [k for k in sd if k not in self._sd]
        if strict and (missing or unexpected):
            raise RuntimeError("Error(s) in loading state_dict: missing %s unexpected %s" % (missing[:5], unexpected[:5]))
        mismatched = _copy_matching(self._sd, sd, strict, resizable=("classifier.0.weight",))
        if "classifier.0.weight" in self._sd:
            self.num_classes = self._sd["classifier.0.weight"].shape[0]
        self._dirty = True
        return missing, unexpected + mismatched

    # ---- engine
    @property
    def precision(self):
        """The arithmetic this model runs in now ("f16x3", "f32" or "f16"; "f32" after a fall back, precision.py)."""
        return _precision.LABEL[self._mode]

    def _needs_bind(self, eng):
        return self._dirty or getattr(eng, "_owner", None) is not self

    def _do_bind(self, eng):
        blob, manifest, _ = weights.pack_seres18(self._sd, cam_factor=getattr(self, "cam_factor", -1.0))
        eng.load_seres18(blob, manifest)
        eng._owner = self
        self._dirty = False

    def _run(self, fn):
        """fn(engine) with this model's weights bound and the context in this model's arithmetic (precision.run)."""
        return _precision.run(self, get_engine(self._device), self.arch, fn)

    def warmup(self, imgsz=(1, 3, IMG_H, IMG_W)):
        """One dummy batch: allocates workspaces and loads code objects (track_yolov5.py:169-171)."""
        self(np.zeros(imgsz, np.float32))
        return self

    def __call__(self, x, cam=None, return_logits=False):
        """``cam``: camera index per image (int array / tensor) - adds cam_factor * cam_bias[cam] to the embedding before the
        classifier, as SERse18_IBN.forward(x, cam) does (SERes18_IBN.py:269-271); the extractor path never passes it."""
        try:
            return self._forward(x, cam, return_logits)
        finally:
            if cam is not None:
                get_engine(self._device).set_side_index(None)     # nothing pending after a failed call

    def _forward(self, x, cam, return_logits):
        is_torch = hasattr(x, "detach")
        if not is_torch:
            x = np.asarray(x, np.float32)
        if x.ndim != 4 or x.shape[1] != 3:
            raise ValueError("expected [N,3,H,W] input, got %s" % (tuple(x.shape),))
        size = check_hw(tuple(x.shape[2:]))
        any_size = size != (IMG_H, IMG_W)
        if any_size and self.arch != "seres18_ibn" and not (self._hw_siblings or self._hw_ema or self._hw_sib_f16):
            raise ValueError("%s runs at [N,3,%d,%d] only (other sizes: seres18_ibn), got %s" % (self.arch, IMG_H, IMG_W, tuple(x.shape)))
        # another size runs the any-size forward: this CALL runs in exact fp32 (mode 0) or, with hw_precision="f16x3", in the fp32-class
        # arithmetic (reid_ctx_set_hw_precision 2 around the call); the model keeps its own mode and the engine gets its settings back
        if not any_size:
            run = self._run
        else:
            call = self._hw_call or _ExactCall(self)

            def run(fn):       # the model's keywords go on inside what `call` sets up, for this call, and off after it
                def scoped(e):
                    with Engine.hw_scope(e, siblings=self._hw_siblings or None, ema=self._hw_ema or None, f16=self._hw_f16 or None,
                                    sib_f16=self._hw_sib_f16 or None):
                        return fn(e)
                return call.run(scoped)
        if is_torch and x.is_cuda:
            if x.device.index != self._device:
                self.to(x.device.index)


            def on_device(eng):
                if cam is not None:
                    eng.set_side_index(_index_array(cam, x.shape[0]))
                return _torch_cuda_forward(
                    x, lambda xf, o: eng.embed_f32_nchw_dev(xf.data_ptr(), xf.shape[0], o[0].data_ptr(), o[1].data_ptr(),
                                                            size=size if any_size else None), eng,
                    (self.embed_dim, self.num_classes))
            emb, logits = run(on_device)
        else:
            x_np = x.detach().float().cpu().numpy() if is_torch else np.asarray(x, np.float32)

            def on_host(eng):
                if cam is not None:
                    eng.set_side_index(_index_array(cam, x_np.shape[0]))
                return eng.embed_f32_nchw(x_np, logits=True)
            emb, logits = run(on_host)
            if is_torch:
                import torch
                emb, logits = torch.from_numpy(emb), torch.from_numpy(logits)
        if self.is_reid:
            return logits                                   # SERes18_IBN.py:272-273
        return (emb, logits) if return_logits else emb

    forward = __call__

    def embed_crops(self, crops):
        """uint8 HxWx3 crops of any size -> float32[N,512]; resize + normalise on the device."""
        crops = list(crops)
        return self._run(lambda eng: eng.embed_ragged_u8(crops))


class _ExactCall(object):
    """precision.run owner for ONE call in exact fp32 with another object's weights (an input size other than 256 x 128)."""
    _mode = _precision.EXACT

    def __init__(self, owner):
        self._owner = owner

    def _needs_bind(self, eng):
        return self._owner._needs_bind(eng)

    def _do_bind(self, eng):
        self._owner._do_bind(eng)

    def run(self, fn):
        return _precision.run(self, get_engine(self._owner._device), self._owner.arch, fn)


class _HwClassCall(_ExactCall):
    """precision.run owner for the calls of a model at another input size in the fp32-class arithmetic (hw_precision="f16x3"): the context
    in mode 2 and reid_ctx_set_hw_precision 2 around the call, both restored after it.  A checkpoint outside the split range (refused at
    the switch, or through the fault word while running) makes THIS owner exact fp32 for the rest of the model's life, with the one log
    line of precision.fallback_to_exact - the model's own mode at 256 x 128 is not touched."""

    def __init__(self, owner):
        _ExactCall.__init__(self, owner)
        self._mode = _precision.F32_CLASS

    def run(self, fn):
        def scoped(e):
            with e.hw_precision_scope(2 if self._mode == _precision.F32_CLASS else None):
                return fn(e)
        return _ExactCall.run(self, scoped)


def seres18_ibn(num_classes=751, loss="triplet", pretrained=False, use_gpu=True, **kwargs):
    """Factory with the registry's calling convention (models/__init__.py:116-121)."""
    return SERes18IBN(num_classes=num_classes, loss=loss, pretrained=pretrained, use_gpu=use_gpu, **kwargs)


class CARes18IBN(SERes18IBN):
    """CARes18_IBN (reid/backbones/CARes18.py:185-281): the same IBN-Net skeleton, every block ends in
    relu(TripletAttention(y) + shortcut) (:148-157; triplet_attention.py:69-101).  All three arithmetic modes; precision="f16"
    (fp16 storage) runs the tails of libreid_hip_siblings_f16.so, which must lie beside libreid_hip.so.  ``hw_siblings=True``: inputs
    [N,3,H,W] of another size (sides 32 .. 512) run too, in exact fp32 or - ``hw_precision="f16x3"`` - fp32-class, as seres18_ibn's do,
    with the TripletAttention tail of libreid_hip_anysize_ca.so."""
    arch = "cares18_ibn"


class EMARes18IBN(SERes18IBN):
    """EMARes18_IBN (reid/backbones/EMA_Res18.py:118-181): every block ends in relu(EMA(y) + shortcut) (:79-86), EMA with 32
    channel groups (:10-38).  All three arithmetic modes; precision="f16" (fp16 storage) runs the tails of
    libreid_hip_siblings_f16.so, which must lie beside libreid_hip.so.  ``hw_ema=True``: inputs [N,3,H,W] of another size (sides 32 ..
    512) run too, in exact fp32 or - ``hw_precision="f16x3"`` - fp32-class, as seres18_ibn's do, with the EMA tail of
    libreid_hip_anysize_ema.so."""
    arch = "emares18_ibn"


def cares18_ibn(num_classes=751, loss="triplet", pretrained=False, use_gpu=True, **kwargs):
    """Same name as the reference's factory (CARes18.py:270-281)."""
    return CARes18IBN(num_classes=num_classes, loss=loss, pretrained=pretrained, use_gpu=use_gpu, **kwargs)


def emares18_ibn(num_classes=751, loss="triplet", pretrained=False, use_gpu=True, **kwargs):
    """Same name as the reference's factory (EMA_Res18.py:184-195)."""
    return EMARes18IBN(num_classes=num_classes, loss=loss, pretrained=pretrained, use_gpu=use_gpu, **kwargs)


class SwinT:
    """The reference's custom Swin-T (reid/backbones/swin_transformer.py:339-427, swin_t :508-513): conv stem,
    4 stages of (W-MSA, SW-MSA) blocks, top-down ConvTranspose fusion, LN -> GeM_1D -> BatchNorm1d(96).  ``version="v1"`` (default):
    pre-norm blocks, scaled dot-product attention with a 13x13 relative-position table; ``version="v2"``: post-norm blocks, cosine
    attention with a learned scale per head and a position bias from meta_mlp (:140-149,205-209,238-246) - the reference's
    ``--backbone swin_v2``.  The state_dict speaks the reference's keys of that version.

    ``model(x)`` -> embedding [N,96] (x_norm); ``model(x, return_logits=True)`` -> (logits, embedding), the order of the
    reference's eval-mode tuple (:422-423).  ``x``: float [N,3,H,W] with H, W multiples of 224 - the
    reference itself rejects 128x256.  Unlike the reference (Q14) N = 1 works.
    """

    embed_dim = 96

    arch = "swin_transformer"
    _arch = "swin"            # precision.run: which of the shared engine's two weight sets this object owns

    def __init__(self, num_classes=751, loss="softmax", pretrained=False, use_gpu=True, seed=0, camera=0, sequence=0, side_info=True,
                 side_info_coeff=1.5, precision=None, version="v1", hw_sib_f16=False, **_):
        if Engine.hw_sib_f16_value(hw_sib_f16):
            raise ValueError("swin_transformer has no hw_sib_f16 argument (cares18_ibn and emares18_ibn only)")
        if version not in synth.SWIN_VERSIONS:
            raise ValueError("swin_t: version must be 'v1' or 'v2', got %r" % (version,))
        self.version = version
        self._mode = _precision.resolve(precision)
        self.num_classes = num_classes
        self.loss = loss
        self.training = False
        self._device = 0
        # ShadowFeatureExtraction's side-information table (swin_transformer.py:285-293): camera * sequence, camera or sequence rows
        self.views = camera * sequence if camera * sequence > 0 else camera if camera > 0 else max(sequence, 0)
        self.side_info, self.side_info_coeff = bool(side_info), float(side_info_coeff)
        self._sd = synth.swin_state_dict(seed, num_class=num_classes, views=self.views, version=version)
        self._dirty = True
        if pretrained:
            import warnings
            warnings.warn("no pretrained Swin weights are reachable offline (pretrained_urls is empty in the reference, "
                          "swin_transformer.py:19); keeping the seeded random initialisation")

    to = SERes18IBN.to
    cuda = SERes18IBN.cuda
    half = SERes18IBN.half
    float = SERes18IBN.float
    eval = SERes18IBN.eval
    train = SERes18IBN.train
    parameters = SERes18IBN.parameters
    state_dict = SERes18IBN.state_dict
    _ref_key = SERes18IBN._ref_key

    def load_state_dict(self, state_dict, strict=True):
        sd = weights.normalize_state_dict(state_dict)
        missing = [k for k in self._sd if k not in sd]
        unexpected = [k for k in sd if k not in self._sd]
        if strict and (missing or unexpected):
            raise RuntimeError("Error(s) in loading state_dict: missing %s unexpected %s" % (missing[:5], unexpected[:5]))
        mismatched = _copy_matching(self._sd, sd, strict, resizable=("classifier.weight", "classifier.0.weight"))
        for k in ("classifier.weight", "classifier.0.weight"):
            if k in self._sd:
                self.num_classes = self._sd[k].shape[0]
        self._dirty = True
        return missing, unexpected + mismatched

    precision = SERes18IBN.precision
    _run = SERes18IBN._run

    def _needs_bind(self, eng):
        return self._dirty or getattr(eng, "_swin_owner", None) is not self

    def _do_bind(self, eng):
        blob, manifest, _ = weights.pack_swin(self._sd, side_info_coeff=getattr(self, "side_info_coeff", 1.5))
        eng.load_swin(blob, manifest)
        eng._swin_owner = self
        self._dirty = False

    def warmup(self, imgsz=(1, 3, 224, 224)):
        self(np.zeros(imgsz, np.float32))
        return self

    def __call__(self, x, view_index=None, return_logits=False):
        """``view_index``: view (camera / sequence) index per image - adds side_info_coeff * side_info_embedding[view] to the SFE
        output when the model was built with side_info and camera / sequence > 0 (swin_transformer.py:301-302, which ignores
        the argument otherwise - so does this)."""
        if view_index is not None and not (self.side_info and self.views > 0):
            if self.side_info:      # the reference would index a parameter that does not exist (AttributeError)
                raise AttributeError("SwinTransformer was built without camera / sequence: no side_info_embedding")
            view_index = None
        try:
            return self._forward(x, view_index, return_logits)
        finally:
            if view_index is not None:
                get_engine(self._device).set_side_index(None)

    def _forward(self, x, view_index, return_logits):
        is_torch = hasattr(x, "detach")
        if is_torch and x.is_cuda:
            if x.ndim != 4 or x.shape[1] != 3 or x.shape[2] % 224 or x.shape[3] % 224:
                raise ValueError("expected float[n,3,224k,224m], got %s" % (tuple(x.shape),))
            if x.device.index != self._device:
                self.to(x.device.index)


            def on_device(eng):
                if view_index is not None:
                    eng.set_side_index(_index_array(view_index, x.shape[0]))
                return _torch_cuda_forward(
                    x, lambda xf, o: eng.swin_embed_dev(xf.data_ptr(), xf.shape[0], xf.shape[2], xf.shape[3], o[0].data_ptr(), o[1].data_ptr()),
                    eng, (self.embed_dim, self.num_classes))
            emb, logits = self._run(on_device)
        else:
            x_np = x.detach().float().cpu().numpy() if is_torch else np.asarray(x, np.float32)

            def on_host(eng):
                if view_index is not None:
                    eng.set_side_index(_index_array(view_index, x_np.shape[0]))
                return eng.swin_embed_f32_nchw(x_np, logits=True)
            emb, logits = self._run(on_host)
            if is_torch:
                import torch
                emb, logits = torch.from_numpy(emb), torch.from_numpy(logits)
        return (logits, emb) if return_logits else emb

    forward = __call__

    def descriptor(self, x, view_index=None, flip_tta=True):
        """The evaluation script's retrieval descriptor (reid/image_reid_inference.py:112-123,252-253 with --backbone swin_*):
        float [N,3,H,W] (numpy or CPU / CUDA torch tensor, H, W multiples of 224) -> numpy float32 [N, num_classes + 96] =
        [normalize(logits) | normalize(x_norm)], averaged with the mirrored image's and renormalised when ``flip_tta``.
        ``view_index`` (the script's --sie: the camera index) serves the plain and the mirrored view of an image alike."""
        x_np = x.detach().float().cpu().numpy() if hasattr(x, "detach") else np.asarray(x, np.float32)
        if x_np.ndim != 4 or x_np.shape[1] != 3 or x_np.shape[2] <= 0 or x_np.shape[3] <= 0 or x_np.shape[2] % 224 or x_np.shape[3] % 224:
            raise ValueError("expected float[n,3,224k,224m], got %s" % (tuple(x_np.shape),))
        if view_index is not None and not (self.side_info and self.views > 0):
            if self.side_info:
                raise AttributeError("SwinTransformer was built without camera / sequence: no side_info_embedding")
            view_index = None
        idx = None
        if view_index is not None:
            idx = _index_array(view_index, x_np.shape[0])
            if idx.size and (idx.min() < 0 or idx.max() >= self.views):
                raise ValueError("view_index must lie in [0, %d), got %d .. %d" % (self.views, idx.min(), idx.max()))

        def run(eng):
            if idx is not None:
                eng.set_side_index(idx)
            return eng.swin_descriptor_f32_nchw(x_np, flip_tta=flip_tta)
        try:
            return self._run(run)
        finally:
            if idx is not None:
                get_engine(self._device).set_side_index(None)

    def descriptor_images(self, images, size=(448, 224), view_index=None, flip_tta=True):
        """descriptor() from uint8 HxWx3 images of any sizes as the dataset stores them: the evaluation script's transform - PIL's
        antialiased Resize to ``size`` = (H, W) (multiples of 224), ToTensor, ImageNet Normalize (reid/data_transforms.py:56-127) -
        runs on the device, and the rows are bit-identical to descriptor() on the images preprocessed with PIL on the host."""
        images = list(images)
        Engine._swin_crop_args(size, None)                  # a bad size raises here, before anything is bound or launched
        for i, im in enumerate(images):
            if getattr(im, "dtype", None) != np.uint8 or np.ndim(im) != 3 or np.shape(im)[2] != 3 or min(np.shape(im)[:2]) < 1:
                raise ValueError("image %d must be uint8 [h,w,3], got %s %s" % (i, getattr(im, "dtype", type(im)), np.shape(im)))
        if view_index is not None and not (self.side_info and self.views > 0):
            if self.side_info:
                raise AttributeError("SwinTransformer was built without camera / sequence: no side_info_embedding")
            view_index = None
        idx = None
        if view_index is not None:
            idx = _index_array(view_index, len(images))
            if idx.size and (idx.min() < 0 or idx.max() >= self.views):
                raise ValueError("view_index must lie in [0, %d), got %d .. %d" % (self.views, idx.min(), idx.max()))

        def run(eng):
            if idx is not None:
                eng.set_side_index(idx)
            return eng.swin_descriptor_images_u8(images, size=size, flip_tta=flip_tta)
        try:
            return self._run(run)
        finally:
            if idx is not None:
                get_engine(self._device).set_side_index(None)

    def embed_crops(self, crops, size=(224, 224)):
        """uint8 HxWx3 crops of any size -> float32[N,96]: bilinear resize to ``size`` = (H, W) (multiples of 224), ImageNet
        normalisation (reid/data_transforms.py:64) and the stem's first convolution in one kernel on the device."""
        crops = list(crops)
        Engine._swin_crop_args(size, None)                  # a bad size raises here, before anything is bound or launched
        return self._run(lambda eng: eng.swin_embed_ragged_u8(crops, size=size))

    def embed_frame(self, frame, boxes_xyxy, size=(224, 224)):
        """Windows frame[y1:y2, x1:x2] of one uint8 frame (int boxes [N,4] as x1,y1,x2,y2) -> float32[N,96]; the frame is uploaded once."""
        Engine._swin_crop_args(size, None)
        return self._run(lambda eng: eng.swin_embed_frame_u8(frame, boxes_xyxy, size=size))


def swin_t(num_classes=751, loss="softmax", pretrained=False, use_gpu=True, **kwargs):
    """Registry constructor, same name as the reference's (swin_transformer.py:508)."""
    return SwinT(num_classes=num_classes, loss=loss, pretrained=pretrained, use_gpu=use_gpu, **kwargs)
