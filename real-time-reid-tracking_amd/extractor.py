"""DeepSORT appearance extractor - mirror of modification_deepsort/feature_extractor.py:14-53.

    extractor = Extractor(model_path, use_cuda=True)
    features  = extractor(im_crops)        # list of HxWx3 uint8 -> np.ndarray float32 [N, 512]

A checkpoint of the reference's other tracker ReID model, swin_transformer (modification_tracking/models/__init__.py:80,
reid_model_factory.py:9), is recognised from its keys: the same object then resizes to 224x224 (``size=`` overrides; multiples of 224),
normalises with ImageNet's mean / std (reid/data_transforms.py:64) and returns float32 [N, 96].

What the reference does per call (feature_extractor.py:31-53): a Python loop of cv2.resize + ToTensor + Normalize
per crop, torch.cat, H2D copy, backbone forward, D2H copy.  Here the crops are packed once, copied once, and the
resize / normalise / backbone all run as HIP kernels; the return value is a fresh C-contiguous host array.

Deviations, all forced by defects of the reference file itself:
  Q1  it imports a class that no longer exists (SEDense18_IBN); this binds to the current SERse18_IBN layout.
  Q2  it never calls .eval(); the only well-defined semantics, used here, is eval mode (running-stat BN).
  Q3  embedding = BNNeck output (512-d), the first element of the eval-mode tuple (SERes18_IBN.py:274-275).
"""
import logging

import numpy as np

from . import precision as _precision
from . import weights


def pack_checkpoint(state_dict):
    """state_dict -> (arch, blob, manifest, info): arch "swin" for a swin_t checkpoint (v1 or v2: the ShadowFeatureExtraction stem and
    the stage keys, weights.is_swin_state_dict), packed with weights.pack_swin; "seres18" for everything else, packed with
    weights.pack_seres18 as before (strict=False semantics, feature_extractor.py:19).  No engine, no device."""
    if weights.is_swin_state_dict(state_dict):
        return ("swin",) + tuple(weights.pack_swin(state_dict))
    return ("seres18",) + tuple(weights.pack_seres18(state_dict))


class Extractor(object):
    def __init__(self, model_path, use_cuda=True, device=0, precision=None, size=None, hw_siblings=False, hw_ema=False, hw_f16=False, hw_sib_f16=False):
        """``Extractor(model_path, use_cuda=True)`` as feature_extractor.py:15-29.  ``precision`` (keyword, not in the reference):
        "f16x3" (default; $REID_PRECISION overrides the default) / "f32" / "f16" - see precision.py; a checkpoint the fp32-class
        arithmetic cannot represent runs in exact fp32, with one log line.  ``size`` (keyword, (W, H) like ``self.size``): the size
        crops are resized to - a Swin checkpoint takes multiples of 224 (default (224, 224)); the ResNet family (128, 256), and a
        seres18_ibn checkpoint any (W, H) with sides in 32 .. 512 (DeepSORT's own (64, 128), feature_extractor.py:23) when its
        arithmetic is asked for by name: ``precision="f32"`` (exact fp32) or ``precision="f16x3"`` (fp32-class, the any-size forward's
        reid_ctx_set_hw_precision 2 around every call) must be given - $REID_PRECISION is a default, not a name, and nothing is demoted
        behind the caller's back - and the object's log line names size and arithmetic.  ``hw_siblings=True`` (keyword) lets a cares18_ibn
        checkpoint take such a size too, under the same rule: Engine.set_hw_siblings(True) around every call (the TripletAttention tail
        of libreid_hip_anysize_ca.so); ``hw_ema=True`` (keyword) does the same for an emares18_ibn checkpoint: Engine.set_hw_ema(True)
        around every call (the EMA tail of libreid_hip_anysize_ema.so); without it emares18_ibn has no other size.  ``hw_f16=True``
        (keyword, seres18_ibn checkpoints only): at such a size the crops run in fp16 storage with fp32 accumulation -
        Engine.set_hw_f16(True) around every call (libreid_hip_anysize_f16.so); it names the arithmetic itself, so ``precision`` need not
        be given, and whatever ``precision`` is applies at (128, 256) only.  ``hw_sib_f16=True`` (keyword, cares18_ibn / emares18_ibn
        checkpoints only, without ``hw_f16``): the same for the siblings - Engine.set_hw_sib_f16(True) around every call
        (libreid_hip_anysize_sib_f16.so); the keyword alone is enough, ``hw_siblings`` / ``hw_ema`` and ``precision`` need not be given."""
        if not use_cuda:
            raise RuntimeError("Extractor: the MI355X engine has no CPU path (use_cuda=False is not supported)")
        self.device = "cuda"
        self._mode = _precision.resolve(precision)
        from .engine import Engine as _Engine
        self._hw_siblings = bool(_Engine.hw_siblings_value(hw_siblings))      # a bad value raises here, before any device call
        self._hw_ema = bool(_Engine.hw_ema_value(hw_ema))
        self._hw_f16 = bool(_Engine.hw_f16_value(hw_f16))
        self._hw_sib_f16 = bool(_Engine.hw_sib_f16_value(hw_sib_f16))
        if self._hw_sib_f16 and self._hw_f16:
            raise ValueError("Extractor: hw_sib_f16 and hw_f16 name the fp16-storage arithmetic of different checkpoints: give one of them, "
                             "got hw_sib_f16=%r and hw_f16=%r" % (hw_sib_f16, hw_f16))
        if isinstance(model_path, dict):
            state_dict = model_path            # already-loaded state_dict (tests, benchmarks)
        else:
            # PyTorch only reads the checkpoint (feature_extractor.py:18) - and it is imported BEFORE the engine: torch bundles its
            # own HIP runtime, and the process must hold ONE (libreid_hip.so binds to whichever is loaded first; the other order
            # loads two and aborts in the exit handlers - DESIGN.md section 6, the rule parallel.RcclComm.from_env enforces)
            import torch
            state_dict = torch.load(model_path, map_location="cpu")   # {"state_dict": ...} / "module." prefixes: weights.pack_seres18
        from .engine import Engine, get_engine, hw_f16_gate, hw_sib_f16_gate
        self._arch, blob, manifest, self.info = pack_checkpoint(state_dict)
        if self._hw_ema and self.info.get("arch") != "emares18_ibn":
            raise ValueError("Extractor: hw_ema belongs to emares18_ibn checkpoints, got %s" % (self.info.get("arch"),))
        got = "swin" if self._arch == "swin" else self.info.get("arch")       # no hw_precision here: `precision` names that arithmetic
        hw_f16_gate(hw_f16, None, got == "seres18_ibn", "Extractor: hw_f16 belongs to seres18_ibn checkpoints (the fp16-storage any-size "
                    "forward serves them only), got %s" % (got,), None)
        hw_sib_f16_gate(hw_sib_f16, None, False, got in ("cares18_ibn", "emares18_ibn"), "Extractor: hw_sib_f16 belongs to cares18_ibn / "
                        "emares18_ibn checkpoints (seres18_ibn: hw_f16), got %s" % (got,), None)
        if self._arch == "swin":
            self.size = tuple(int(v) for v in (size or (224, 224)))           # (W, H)
            Engine._swin_crop_args(self.size[::-1], None)
        else:
            self.size = (128, 256)             # (W, H), feature_extractor.py:24
            if size is not None and tuple(size) != self.size:
                from .engine import check_hw
                h, w = check_hw(tuple(size)[::-1])
                sized = ("seres18_ibn", "cares18_ibn") if self._hw_siblings else ("seres18_ibn",)
                if self._hw_ema:
                    sized = sized + ("emares18_ibn",)
                if self._hw_f16 or self._hw_sib_f16:
                    pass                       # the architecture was checked above, and the keyword names the arithmetic of this size itself
                elif self.info.get("arch") not in sized or precision is None or self._mode == _precision.F16:
                    raise ValueError("Extractor: at a size other than (W, H) = (128, 256) the ResNet18-IBN family runs seres18_ibn "
                                     "checkpoints in exact fp32 (precision=\"f32\") or fp32-class (precision=\"f16x3\"), asked for by "
                                     "name; got size %r, %s, precision %s"
                                     % (size, self.info.get("arch"), "None" if precision is None else _precision.LABEL[self._mode]))
                self.size = (w, h)
        self.net = get_engine(device)          # a bad size was refused above, before any device call
        setattr(self.net, "_swin_owner" if self._arch == "swin" else "_owner", None)
        self._packed = (blob, manifest)
        _precision.run(self, self.net, "Extractor", lambda eng: None)      # load now; a checkpoint mode 2 refuses falls back here
        logger = logging.getLogger("root.tracker")
        where = model_path if not isinstance(model_path, dict) else "<state_dict>"
        if self._arch != "swin" and self.size != (128, 256):
            logger.info("Loading weights from {}... Done! (size (W, H) = {}: {})".format(
                where, self.size, "fp16 storage" if self._hw_f16 or self._hw_sib_f16 else
                "fp32-class f16x3" if self._mode == _precision.F32_CLASS else "exact fp32"))
        else:
            logger.info("Loading weights from {}... Done!".format(where))

    @property
    def precision(self):
        """The arithmetic this extractor runs in now ("f16x3", "f32" or "f16"; "f32" after a fall back)."""
        return _precision.LABEL[self._mode]

    def _preprocess(self, im_crops):
        """Host-visible equivalent of feature_extractor.py:31-46 is fused into the device path; this only
        validates the crops the way the reference's torch.cat would fail on an empty list."""
        if len(im_crops) == 0:
            raise RuntimeError("Extractor: expected a non-empty list of crops")   # torch.cat([]) raises, :44
        return [np.asarray(im) for im in im_crops]

    def _needs_bind(self, eng):                                # another model of this family was loaded on this device meanwhile
        return getattr(eng, "_swin_owner" if self._arch == "swin" else "_owner", None) is not self

    def _do_bind(self, eng):
        if self._arch == "swin":
            eng.load_swin(*self._packed)
            eng._swin_owner = self
        else:
            eng.load_seres18(*self._packed)
            eng._owner = self

    def _run(self, fn):
        if self._arch != "swin" and self.size != (128, 256):
            # another size: the fp32-class arithmetic is the any-size forward's own setting, put on for the call and taken off after it; after
            # a fall back (precision.run) the object is exact fp32 and the setting stays as the engine has it
            from .engine import Engine

            def scoped(eng):
                sib = True if self._hw_siblings and self.info.get("arch") == "cares18_ibn" else None
                ema = True if self._hw_ema and self.info.get("arch") == "emares18_ibn" else None
                x3 = 2 if self._mode == _precision.F32_CLASS and not self._hw_f16 and not self._hw_sib_f16 else None
                with Engine.hw_scope(eng, precision=x3, siblings=sib, ema=ema, f16=self._hw_f16 or None, sib_f16=self._hw_sib_f16 or None):
                    return fn(eng)
            return _precision.run(self, self.net, "Extractor", scoped)
        return _precision.run(self, self.net, "Extractor", fn)

    def __call__(self, im_crops):
        """feature_extractor.py:48-53: host crops in, host features out (the upload of one pass of crops, its download and the
        kernels of its neighbours overlap inside the library).  A stacked ``uint8[n,256,128,3]`` array - crops already at the
        extractor's size, for which the reference's cv2.resize is the identity - goes to the fixed-size entry point as it is (Swin:
        to the crops entry point in place, without a packing copy).  A Swin checkpoint returns float32 [N, 96]."""
        size_hw = (self.size[1], self.size[0])
        if isinstance(im_crops, np.ndarray) and im_crops.dtype == np.uint8 and im_crops.ndim == 4 \
                and im_crops.shape[1:] == size_hw + (3,) and im_crops.shape[0] > 0:
            if self._arch == "swin":
                stacked = np.ascontiguousarray(im_crops)
                return self._run(lambda eng: eng.swin_embed_ragged_u8(list(stacked), size=size_hw))
            if size_hw != (256, 128):
                stacked = np.ascontiguousarray(im_crops)
                return self._run(lambda eng: eng.embed_ragged_u8(list(stacked), size=size_hw))
            return self._run(lambda eng: eng.embed_u8(im_crops))
        crops = self._preprocess(im_crops)
        if self._arch == "swin":
            return self._run(lambda eng: eng.swin_embed_ragged_u8(crops, size=size_hw))
        if size_hw != (256, 128):
            return self._run(lambda eng: eng.embed_ragged_u8(crops, size=size_hw))
        return self._run(lambda eng: eng.embed_ragged_u8(crops))

    def from_frame(self, bbox_xywh, ori_img):
        """DeepSort._get_features(bbox_xywh, ori_img) ([external] deep_sort.py) in one call: centre-format boxes are
        converted and clipped like DeepSort._xywh_to_xyxy (x1 = max(int(x - w/2), 0), x2 = min(int(x + w/2), W - 1), ...),
        the frame goes to the device once and the windows are cut and resized there.  Returns float32 [N, 512] ([N, 96] for Swin)
        (an empty array when there is no box, as the reference's `np.array([])` branch)."""
        ori_img = np.asarray(ori_img)
        boxes = np.asarray(bbox_xywh, dtype=np.float64).reshape(-1, 4)
        if boxes.shape[0] == 0:
            return np.array([])
        height, width = ori_img.shape[:2]
        xyxy = np.empty((boxes.shape[0], 4), np.int32)
        for i, (x, y, w, h) in enumerate(boxes):
            xyxy[i] = (max(int(x - w / 2), 0), max(int(y - h / 2), 0), min(int(x + w / 2), width - 1), min(int(y + h / 2), height - 1))
        if self._arch == "swin":
            return self._run(lambda eng: eng.swin_embed_frame_u8(ori_img, xyxy, size=(self.size[1], self.size[0])))
        if self.size != (128, 256):      # the frame entry is 256 x 128; the same windows, cut on the host, through the ragged entry
            crops = [ori_img[y1:y2, x1:x2] for x1, y1, x2, y2 in xyxy]
            return self._run(lambda eng: eng.embed_ragged_u8(crops, size=(self.size[1], self.size[0])))
        return self._run(lambda eng: eng.embed_frame_u8(ori_img, xyxy))
