"""Thin numpy-facing wrapper over one libreid_hip context (one per process and device).

Nothing here computes: every method marshals numpy arrays (or raw device
pointers) into the C ABI and returns what the HIP kernels produced.
"""
import collections
import contextlib
import ctypes as C

import numpy as np

from . import _ffi
from ._ffi import check

_ENGINES = {}

IMG_H, IMG_W = 256, 128   # Extractor.size = (128, 256) as (W, H), feature_extractor.py:24
SIZE_MIN, SIZE_MAX = 32, 512   # input sides of the any-size forward (reid_*_hw, include/reid_hip.h)
HW_PRECISION_NAMES = {"f32": 0, "fp32": 0, "exact": 0, "f16x3": 2, "fp32-class": 2}   # Engine.set_hw_precision
DISTMAT_PRECISION_NAMES = {"f32": 0, "f16x3": 2}   # Engine.distmat(precision=): the exact entry, reid_distmat_x3
SELECT_X3_KMAX = 24                                # Engine.knn(precision="f16x3"): reid_knn_x3's largest k


def check_hw(size):
    """(H, W) of a ResNet18-IBN-SE input, each side an integer in [32, 512]; ValueError otherwise, before any device call."""
    try:
        h, w = size
        if int(h) != h or int(w) != w:
            raise TypeError
        h, w = int(h), int(w)
    except (TypeError, ValueError):
        raise ValueError("size must be (H, W) integers, got %r" % (size,))
    if not (SIZE_MIN <= h <= SIZE_MAX and SIZE_MIN <= w <= SIZE_MAX):
        raise ValueError("input size (H, W) = (%d, %d): each side must be in [%d, %d]" % (h, w, SIZE_MIN, SIZE_MAX))
    return h, w


def any_pass_size(chunk, h, w):
    """Images per pass of the any-size forward: the context's chunk scaled by 256 * 128 / (h * w), clamped to 1 .. 4096 (se_any_pass)."""
    return max(1, min(4096, int(chunk) * IMG_H * IMG_W // (int(h) * int(w))))


def stage_shapes(h, w):
    """[(Ho, Wo, C)] of the ten activation taps of reid_debug_stage for an h x w input (stem, pool, eight blocks)."""
    h1, w1 = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    hh, ww = (h1 - 1) // 2 + 1, (w1 - 1) // 2 + 1
    out = [(h1, w1, 64), (hh, ww, 64)]
    for c, stride in ((64, 1), (64, 1), (128, 2), (128, 1), (256, 2), (256, 1), (512, 1), (512, 1)):
        hh, ww = (hh - 1) // stride + 1, (ww - 1) // stride + 1
        out.append((hh, ww, c))
    return out


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _f16(a):
    return np.ascontiguousarray(a, dtype=np.float16)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _hw_precision_c(v):
    if v is None:
        return -1
    if isinstance(v, str):
        return HW_PRECISION_NAMES.get(v.strip().lower())
    if not isinstance(v, bool) and isinstance(v, (int, np.integer)) and int(v) in (-1, 0, 2):
        return int(v)
    return None


def _hw_flag_c(v):
    if isinstance(v, (bool, np.bool_)) or (isinstance(v, (int, np.integer)) and int(v) in (0, 1)):
        return int(v)
    return None


# The settings of the any-size forward, each stated once: name, C setter, the library's default as the property reports it (an int keeps
# the C value, a bool its truth), value -> C value (None: refused), the ValueError text, the exceptions a restoring scope lets pass, and
# the docstrings of set_hw_X and - where they are not the flag form's - of hw_X_value and hw_X.  Engine.hw_X_value, set_hw_X, hw_X and
# hw_X_scope are built from a row; Engine.hw_scope enters the scopes in this order.
HwSetting = collections.namedtuple("HwSetting", "name setter default c_value error restore_may_fail set_doc value_doc get_doc")
HW_SETTINGS = (
    HwSetting("hw_precision", "reid_ctx_set_hw_precision", -1, _hw_precision_c,
              "hw_precision must be None / -1 (other input sizes need mode 0), \"f32\" / 0 or \"f16x3\" / 2, got %r",
              (_ffi.ReidHipError,),      # `prev` was 2 and the weights bound meanwhile cannot be split: stay
              """The arithmetic of the any-size forward of seres18_ibn (reid_ctx_set_hw_precision): None / -1 = another size needs the context
        in mode 0 (default), "f32" / 0 = other sizes run exact fp32 whatever the mode, "f16x3" / 2 = they run fp32-class whatever the mode
        (libreid_hip_anysize_x3.so).  256 x 128 is not affected.""",
              """None / -1 -> -1, "f32" / 0 -> 0, "f16x3" / 2 -> 2 (the values of reid_ctx_set_hw_precision); ValueError otherwise, before any
        device call - the fp16-storage arithmetic of the any-size forward is a setting of its own (set_hw_f16), every other value has none.""",
              "-1, 0 or 2: what set_hw_precision set last (the library's default is -1)."),
    HwSetting("hw_siblings", "reid_ctx_set_hw_siblings", False, _hw_flag_c,
              "hw_siblings must be False / 0 (other input sizes run seres18_ibn only) or True / 1 (cares18_ibn too), got %r", (),
              """CARes18-IBN at input sizes other than 256 x 128 (reid_ctx_set_hw_siblings): False (default) = the reid_*_hw entries refuse a
        loaded cares18_ibn at another size, True = it runs there with the TripletAttention tail of libreid_hip_anysize_ca.so, under the
        size, precision and pass-size rules of seres18_ibn.  emares18_ibn stays refused; 256 x 128 is not affected.""", None, None),
    HwSetting("hw_ema", "reid_ctx_set_hw_ema", False, _hw_flag_c,
              "hw_ema must be False / 0 (other input sizes refuse emares18_ibn) or True / 1 (they run it), got %r", (),
              """EMARes18-IBN at input sizes other than 256 x 128 (reid_ctx_set_hw_ema): False (default) = the reid_*_hw entries refuse a
        loaded emares18_ibn at another size, True = it runs there with the EMA tail of libreid_hip_anysize_ema.so, under the size,
        precision and pass-size rules of seres18_ibn and whatever set_hw_siblings is.  cares18_ibn still needs set_hw_siblings; 256 x 128 is
        not affected.""", None, None),
    HwSetting("hw_f16", "reid_ctx_set_hw_f16", False, _hw_flag_c,
              "hw_f16 must be False / 0 (other input sizes run in the arithmetic hw_precision names) or True / 1 (they run "
              "seres18_ibn in fp16 storage), got %r", (),
              """seres18_ibn at input sizes other than 256 x 128 in fp16 storage with fp32 accumulation (reid_ctx_set_hw_f16): False (default) =
        set_hw_precision and the mode decide, True = such inputs run through libreid_hip_anysize_f16.so whatever the mode and
        hw_precision, which keeps its value.  cares18_ibn / emares18_ibn are refused there; 256 x 128 is not affected.""", None, None),
    HwSetting("hw_sib_f16", "reid_ctx_set_hw_sib_f16", False, _hw_flag_c,
              "hw_sib_f16 must be False / 0 (other input sizes run cares18_ibn / emares18_ibn as hw_siblings, hw_ema and "
              "hw_precision say) or True / 1 (they run them in fp16 storage), got %r", (),
              """cares18_ibn / emares18_ibn at input sizes other than 256 x 128 in fp16 storage with fp32 accumulation
        (reid_ctx_set_hw_sib_f16): False (default) = set_hw_siblings, set_hw_ema, set_hw_precision and the mode decide (and set_hw_f16
        refuses them), True = such inputs run through libreid_hip_anysize_f16.so with the block tails of libreid_hip_anysize_sib_f16.so
        whatever those settings are; they keep their values.  seres18_ibn and 256 x 128 are not affected.""", None, None),
)


class _HwSettings:
    """Engine's share of the any-size settings: hw_X_value, set_hw_X, hw_X and hw_X_scope per row of HW_SETTINGS (_hw_members, below
    the class), and hw_scope over all of them.  The scopes go through ``self.hw_X`` and ``self.set_hw_X`` only, so they serve any object
    that has those two (the host tests' stand-ins)."""

    @contextlib.contextmanager
    def hw_scope(self, precision=None, siblings=None, ema=None, f16=None, sib_f16=None):
        """Context manager over the five single scopes, entered in the order of HW_SETTINGS - precision, siblings, ema, f16, sib_f16 - and
        left in reverse: a value of None leaves that setting alone, every other one is set inside and what it was before comes back
        outside (hw_X_scope).  The package calls it as ``Engine.hw_scope(eng, ...)``, which asks of ``eng`` only the attribute and the
        setter of each setting that is not None."""
        with contextlib.ExitStack() as stack:
            for s, v in zip(HW_SETTINGS, (precision, siblings, ema, f16, sib_f16)):
                if v is not None:
                    stack.enter_context(getattr(_HwSettings, s.name + "_scope")(self, v))
            yield self


def _hw_members(s):
    """(hw_X_value, set_hw_X, hw_X, hw_X_scope) of one row of HW_SETTINGS."""
    attr, kept, flag = "_" + s.name, type(s.default), s.c_value is _hw_flag_c

    def value(v):
        c = s.c_value(v)
        if c is None:
            raise ValueError(s.error % (v,))
        return c

    def setter(self, v):
        c = value(v)
        check(getattr(self.lib, s.setter)(self.h, c))
        setattr(self, attr, kept(c))

    def getter(self):
        return getattr(self, attr, s.default)

    @contextlib.contextmanager
    def scope(self, v):
        if v is None:
            yield self
            return
        prev = getattr(self, s.name)
        getattr(self, "set_" + s.name)(v)
        try:
            yield self
        finally:
            if getattr(self, s.name) != prev:
                try:
                    getattr(self, "set_" + s.name)(prev)
                except s.restore_may_fail:
                    pass
    value.__doc__ = "False / 0 -> 0, True / 1 -> 1 (the values of %s); ValueError otherwise, before any device call." % s.setter if flag else s.value_doc
    setter.__doc__ = s.set_doc
    getter.__doc__ = "What set_%s set last (the library's default is False)." % s.name if flag else s.get_doc
    scope.__doc__ = ("Context manager: ``%s`` None leaves the setting alone; otherwise it is set inside and what it was before comes back outside."
                     % ("on" if flag else "v"))
    for fn, name in ((value, s.name + "_value"), (setter, "set_" + s.name), (scope, s.name + "_scope")):
        fn.__name__, fn.__qualname__ = name, "Engine." + name
    return staticmethod(value), setter, property(getter), scope


for _s in HW_SETTINGS:
    for _name, _member in zip((_s.name + "_value", "set_" + _s.name, _s.name, _s.name + "_scope"), _hw_members(_s)):
        setattr(_HwSettings, _name, _member)


def hw_f16_gate(hw_f16, hw_precision, fits, belongs, of):
    """The keyword hw_f16 at one call site: it belongs to seres18_ibn - ``fits`` is the site's test of its architecture, ``belongs`` the
    site's words when it fails - and replaces hw_precision as the name of the arithmetic of ``of`` (the site's words).  ValueError, before
    any device call; returns the keyword as a bool."""
    on = bool(Engine.hw_f16_value(hw_f16))
    if on and not fits:
        raise ValueError(belongs)
    if on and hw_precision is not None:
        raise ValueError("hw_f16 and hw_precision both name the arithmetic of %s: give one of them, got hw_f16=%r and hw_precision=%r"
                         % (of, hw_f16, hw_precision))
    return on


def hw_sib_f16_gate(hw_sib_f16, hw_precision, hw_f16, fits, belongs, of):
    """The keyword hw_sib_f16 at one call site: it belongs to cares18_ibn / emares18_ibn (``fits``, ``belongs`` as in hw_f16_gate) and goes
    without hw_precision and hw_f16, naming the arithmetic of ``of`` itself.  ValueError, before any device call; returns it as a bool."""
    on = bool(Engine.hw_sib_f16_value(hw_sib_f16))
    if on and not fits:
        raise ValueError(belongs)
    if on and (hw_precision is not None or Engine.hw_f16_value(hw_f16)):
        raise ValueError("hw_sib_f16 names the arithmetic of %s itself: give it without hw_precision and hw_f16, got hw_sib_f16=%r, "
                         "hw_precision=%r, hw_f16=%r" % (of, hw_sib_f16, hw_precision, hw_f16))
    return on


class Engine(_HwSettings):
    def __init__(self, device=0):
        self.lib = _ffi.lib()
        h = C.c_void_p()
        check(self.lib.reid_ctx_create(int(device), C.byref(h)))
        self.h = h
        self.device = int(device)
        self.embed_dim = 512
        self.num_class = 0

    def close(self):
        if self.h:
            self.lib.reid_ctx_sync(self.h)
            for bank in list(getattr(self, "_banks", [])):    # a bank belongs to its context: destroyed before it (no device leak
                bank.close()                                  # when the engine goes first)
            for p in getattr(self, "_pinned", []):
                self.lib.reid_host_free(self.h, p)
            self._pinned = []
            self.lib.reid_ctx_destroy(self.h)
            self.h = None

    def register_bank(self, metric):
        """Feature banks created on this engine (nn_matching.NearestNeighborDistanceMetric): `close` frees them first."""
        self.__dict__.setdefault("_banks", []).append(metric)

    def unregister_bank(self, metric):
        banks = self.__dict__.get("_banks", [])
        if metric in banks:
            banks.remove(metric)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- runtime
    def sync(self):
        check(self.lib.reid_ctx_sync(self.h))

    def device_sync(self):
        """hipDeviceSynchronize on this engine's device (every stream); raises if the context's fault word is set."""
        check(self.lib.reid_device_sync(self.h))

    def clear_fault(self):
        """Resets the sticky fault word (an activation outside f16's range in mode 2 / a non-finite embedding)."""
        check(self.lib.reid_ctx_clear_fault(self.h))

    def precision_ok(self, arch, mode):
        """Can the loaded checkpoint of ``arch`` (0 = ResNet18-IBN-SE family, 1 = Swin) run in ``mode``?  (reid_ctx_precision_ok)"""
        return self.lib.reid_ctx_precision_ok(self.h, int(arch), int(mode)) == 0

    def fault_bits(self):
        """The sticky fault word as bits (1 range, 2 non-finite embedding, 4 split-K rendezvous), without synchronising."""
        b = C.c_int()
        check(self.lib.reid_ctx_fault_peek(self.h, C.byref(b)))
        return b.value

    def set_stream(self, hip_stream):
        """Run on another HIP stream (0 / None = the context's own).  Work already enqueued on the old stream shares the
        context's workspaces with what follows, so a switch drains the old stream first."""
        new = int(hip_stream or 0)
        if new != getattr(self, "_stream", 0):
            self.sync()
            if new == -1:      # the HIP null stream (handle 0, which set_stream reads as "own")
                check(self.lib.reid_ctx_set_null_stream(self.h))
            else:
                check(self.lib.reid_ctx_set_stream(self.h, C.c_void_p(new)))
            self._stream = new

    def use_torch_stream(self):
        """Enqueue on torch's current stream of this device (CUDA-tensor entry points of the backbones).  torch's default
        stream is the HIP null stream, handle 0."""
        import torch
        s = torch.cuda.current_stream(self.device).cuda_stream
        self.set_stream(s if s else -1)

    def on_torch_stream(self):
        """Context manager: run on torch's current stream inside, back on the stream the engine had before outside - the
        process-wide engine is shared with the host-path callers (Extractor, frame pipeline), which must not inherit torch's
        stream (with the null stream the copy side-stream is switched off)."""
        import contextlib

        @contextlib.contextmanager
        def scope():
            prev = getattr(self, "_stream", 0)
            self.use_torch_stream()
            try:
                yield self
            finally:
                self.set_stream(prev)        # drains the torch stream first (set_stream syncs on a switch)
        return scope()

    def set_chunk(self, n):
        check(self.lib.reid_ctx_set_chunk(self.h, int(n)))

    def set_precision(self, mode):
        """0 exact fp32 (the reference's arithmetic), 1 fp16 storage / fp32 accumulate, 2 "fp32-class": fp32 storage, the 3x3
        stride-1 convolutions as three f16 matrix-core products per multiply on hi/lo-split operands (fp32 accumulate)."""
        check(self.lib.reid_ctx_set_precision(self.h, int(mode)))
        self._precision = int(mode)

    @property
    def precision(self):
        """The arithmetic mode this context is in (the library's default is 0)."""
        return getattr(self, "_precision", 0)

    def set_side_index(self, index):
        """Camera (ResNet18-IBN-SE: SERes18_IBN.py:269-270) or view (Swin: swin_transformer.py:301-302) index of every image of
        the following embed call; ``None`` / empty clears."""
        idx = np.ascontiguousarray(np.asarray([] if index is None else index).reshape(-1), np.int32)
        check(self.lib.reid_ctx_set_side_index(self.h, _ptr(idx) if idx.size else None, int(idx.size)))

    def malloc(self, nbytes):
        p = C.c_void_p()
        check(self.lib.reid_malloc(self.h, int(nbytes), C.byref(p)))
        return p.value

    def free(self, dptr):
        check(self.lib.reid_free(self.h, C.c_void_p(dptr)))

    def h2d(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        check(self.lib.reid_memcpy_h2d(self.h, C.c_void_p(dptr), _ptr(arr), arr.nbytes))

    def d2h(self, arr, dptr):
        assert arr.flags["C_CONTIGUOUS"]
        check(self.lib.reid_memcpy_d2h(self.h, _ptr(arr), C.c_void_p(dptr), arr.nbytes))
        return arr

    def timer_start(self):
        check(self.lib.reid_timer_start(self.h))

    def timer_stop(self):
        ms = C.c_float()
        check(self.lib.reid_timer_stop(self.h, C.byref(ms)))
        return ms.value

    def profile(self, on):
        check(self.lib.reid_profile_enable(self.h, int(bool(on))))

    def profile_reset(self):
        check(self.lib.reid_profile_reset(self.h))

    def profile_get(self, kind):
        ms, n, fl, by = C.c_double(), C.c_longlong(), C.c_double(), C.c_double()
        check(self.lib.reid_profile_get(self.h, int(kind), C.byref(ms), C.byref(n), C.byref(fl), C.byref(by)))
        return {"ms": ms.value, "launches": n.value, "flops": fl.value, "bytes": by.value}

    # ---- weights
    def load_seres18(self, blob, manifest):
        blob = _f32(blob)
        self._owner = None                       # the plugin objects (Extractor, backbones) mark what THEY loaded afterwards
        check(self.lib.reid_seres18_load(self.h, _ptr(blob), blob.size, manifest.encode()))
        d, nc = C.c_int(), C.c_int()
        check(self.lib.reid_seres18_dims(self.h, C.byref(d), C.byref(nc)))
        self.embed_dim, self.num_class = d.value, nc.value

    def load_swin(self, blob, manifest):
        blob = _f32(blob)
        self._swin_owner = None
        check(self.lib.reid_swin_load(self.h, _ptr(blob), blob.size, manifest.encode()))
        d, nc = C.c_int(), C.c_int()
        check(self.lib.reid_swin_dims(self.h, C.byref(d), C.byref(nc)))
        self.swin_dim, self.swin_num_class = d.value, nc.value

    def swin_embed_f32_nchw(self, x, logits=False):
        """float32[n,3,h,w] (h, w multiples of 224) -> float32[n,96] (and logits)."""
        x = _f32(x)
        if x.ndim != 4 or x.shape[1] != 3 or x.shape[2] % 224 or x.shape[3] % 224:
            raise ValueError("swin_embed_f32_nchw expects float32[n,3,224k,224m], got %s" % (x.shape,))
        n = x.shape[0]
        emb, lg = self._outs(n, logits, self.swin_dim, self.swin_num_class)
        check(self.lib.reid_swin_embed_f32_nchw(self.h, _ptr(x), n, x.shape[2], x.shape[3], _ptr(emb), _ptr(lg)))
        return self._ret(emb, lg, logits)

    def swin_embed_dev(self, d_x, n, h, w, d_emb, d_logits=None):
        check(self.lib.reid_swin_embed_f32_nchw_dev(self.h, C.c_void_p(d_x), int(n), int(h), int(w), C.c_void_p(d_emb),
                                                    C.c_void_p(d_logits or 0)))

    @staticmethod
    def _swin_crop_args(size, mean_std):
        """(H, W) multiples of 224 and mean[3] / std[3] (None: the library's ImageNet default), checked before any device call."""
        try:
            h, w = (int(v) for v in size)
        except (TypeError, ValueError):
            raise ValueError("size must be (H, W), got %r" % (size,))
        if h <= 0 or w <= 0 or h % 224 or w % 224:
            raise ValueError("Swin crops are resized to multiples of 224 (the reference uses 224x224 and 448x224), got size (H, W) = %r" % (size,))
        ms = None
        if mean_std is not None:
            ms = _f32(mean_std).reshape(-1)
            if ms.size != 6 or not np.isfinite(ms).all() or not (ms[3:] > 0).all():
                raise ValueError("mean_std must be (mean[3], std[3]) with finite values and std > 0, got %r" % (mean_std,))
        return h, w, ms

    def swin_embed_ragged_u8(self, crops, size=(224, 224), mean_std=None, logits=False):
        """list of uint8[h_i,w_i,3] -> float32[n,96] (and logits): each crop is resized to ``size`` = (H, W), normalised with ``mean_std``
        = (mean[3], std[3]) (None: ImageNet, reid/data_transforms.py:64) and run through the Swin stem's first convolution in one kernel
        (reid_swin_embed_ragged_u8); packing and passes as embed_ragged_u8."""
        h, w, ms = self._swin_crop_args(size, mean_std)
        n = len(crops)
        src, offs, hw, _keep = self._pack_ragged(crops)
        emb, lg = self._outs(n, logits, self.swin_dim, self.swin_num_class)
        check(self.lib.reid_swin_embed_ragged_u8(self.h, src, _ptr(offs), _ptr(hw), n, h, w, _ptr(ms), _ptr(emb), _ptr(lg)))
        return self._ret(emb, lg, logits)

    def swin_embed_frame_u8(self, frame, boxes_xyxy, size=(224, 224), mean_std=None, logits=False):
        """uint8[H,W,3] frame + int boxes [n,4] (x1,y1,x2,y2; crop = frame[y1:y2, x1:x2]) -> float32[n,96] (and logits); ``size`` and
        ``mean_std`` as swin_embed_ragged_u8 (reid_swin_embed_frame_u8)."""
        h, w, ms = self._swin_crop_args(size, mean_std)
        frame = np.ascontiguousarray(frame, dtype=np.uint8)
        if frame.ndim != 3 or frame.shape[2] != 3:
            raise ValueError("frame must be uint8[H,W,3], got %s" % (frame.shape,))
        boxes = np.ascontiguousarray(boxes_xyxy, dtype=np.int32).reshape(-1, 4)
        n = boxes.shape[0]
        emb, lg = self._outs(n, logits, self.swin_dim, self.swin_num_class)
        check(self.lib.reid_swin_embed_frame_u8(self.h, _ptr(frame), frame.shape[0], frame.shape[1], _ptr(boxes), n, h, w, _ptr(ms), _ptr(emb),
                                                _ptr(lg)))
        return self._ret(emb, lg, logits)

    # ---- Swin descriptors (the evaluation script's --backbone swin_v1 | swin_v2, reid/image_reid_inference.py:145-152)
    def _swin_descriptor_width(self):
        """num_class + 96 of the loaded Swin weights; ValueError when nothing with a classifier is loaded."""
        nc = getattr(self, "swin_num_class", 0)
        if nc <= 0:
            raise ValueError("a Swin descriptor needs loaded Swin weights with a classifier (Engine.load_swin)")
        return nc + self.swin_dim

    def swin_descriptor_f32_nchw(self, x, flip_tta=True):
        """float32 [n,3,h,w] (h, w multiples of 224, normalised by the caller) -> float32 [n, num_class + 96] retrieval descriptor,
        [normalize(logits) | normalize(x_norm)] - the order of the reference's Swin (swin_transformer.py:422-423) - averaged with
        the mirrored image's and renormalised when ``flip_tta``.  Pending side indices (set_side_index) serve both views."""
        x = _f32(x)
        if x.ndim != 4 or x.shape[1] != 3 or x.shape[2] <= 0 or x.shape[3] <= 0 or x.shape[2] % 224 or x.shape[3] % 224:
            raise ValueError("swin_descriptor_f32_nchw expects float32[n,3,224k,224m], got %s" % (x.shape,))
        out = np.empty((x.shape[0], self._swin_descriptor_width()), np.float32)
        check(self.lib.reid_swin_descriptor_f32_nchw(self.h, _ptr(x), x.shape[0], x.shape[2], x.shape[3], int(bool(flip_tta)), _ptr(out)))
        return out

    def swin_descriptor_dev(self, d_x, n, h, w, flip_tta, d_out):
        """The same on device pointers: d_x fp32 [n,3,h,w] -> d_out fp32 [n, num_class + 96] (reid_swin_descriptor_f32_nchw_dev)."""
        n, h, w = int(n), int(h), int(w)
        if n < 0 or h <= 0 or w <= 0 or h % 224 or w % 224:
            raise ValueError("swin_descriptor_dev expects n >= 0 images of 224k x 224m, got n = %d, h = %d, w = %d" % (n, h, w))
        if n and (not d_x or not d_out):
            raise ValueError("swin_descriptor_dev: null device pointer")
        check(self.lib.reid_swin_descriptor_f32_nchw_dev(self.h, C.c_void_p(d_x), n, h, w, int(bool(flip_tta)), C.c_void_p(d_out)))

    def swin_descriptor_ragged_u8(self, crops, size=(448, 224), mean_std=None, flip_tta=True):
        """list of uint8[h_i,w_i,3] -> float32 [n, num_class + 96]: crops resized to ``size`` = (H, W) and normalised as
        swin_embed_ragged_u8; the mirrored view is the RESIZED crop mirrored (Resize -> flip -> ToTensor -> Normalize)."""
        h, w, ms = self._swin_crop_args(size, mean_std)
        crops = list(crops)
        n = len(crops)
        out = np.empty((n, self._swin_descriptor_width()), np.float32)
        src, offs, hw, _keep = self._pack_ragged(crops)
        check(self.lib.reid_swin_descriptor_ragged_u8(self.h, src, _ptr(offs), _ptr(hw), n, h, w, _ptr(ms), int(bool(flip_tta)), _ptr(out)))
        return out

    def swin_descriptor_images_u8(self, images, size=(448, 224), mean_std=None, flip_tta=True):
        """list of uint8[h_i,w_i,3] images of any sizes -> float32 [n, num_class + 96]: the evaluation script's own transform on the
        device - transforms.Resize(size) as PIL computes it (8-bit antialiased bilinear, bit for bit), ToTensor, Normalize(mean_std;
        None: ImageNet) - then the descriptor of swin_descriptor_f32_nchw, to whose result on host-preprocessed images this is
        bit-identical (reid_swin_descriptor_images_u8).  ``size`` as swin_descriptor_ragged_u8; pending side indices serve both views."""
        h, w, ms = self._swin_crop_args(size, mean_std)
        images = list(images)
        n = len(images)
        src, offs, hw, _keep = self._pack_images(images)
        out = np.empty((n, self._swin_descriptor_width()), np.float32)
        check(self.lib.reid_swin_descriptor_images_u8(self.h, src, _ptr(offs), _ptr(hw), n, h, w, _ptr(ms), int(bool(flip_tta)), _ptr(out)))
        return out

    PIL_MAX_SIDE = 4096     # pil_resize_max_side() of libreid_hip_pil_resize.so: the largest source side of the *_images_u8 entries

    @classmethod
    def _pack_images(cls, images):
        """_pack_ragged for the *_images_u8 entries, with their source limit checked before any device call."""
        for i, im in enumerate(images):
            shp = np.shape(im)
            if len(shp) == 3 and max(shp[0], shp[1]) > cls.PIL_MAX_SIDE:
                raise ValueError("image %d is %d x %d, a source side may be %d at most" % (i, shp[0], shp[1], cls.PIL_MAX_SIDE))
        return cls._pack_ragged(images)

    def descriptor_images_u8(self, images, flip_tta=True, mean_std=None, size=None):
        """list of uint8[h_i,w_i,3] images of any sizes -> float32 [n, 512 + num_class]: transforms.Resize((256, 128)) as PIL computes
        it, ToTensor and Normalize(mean_std; None: ImageNet) on the device, then the descriptor of descriptor_f32_nchw, to whose result
        on host-preprocessed images this is bit-identical (reid_descriptor_images_u8).  ``size`` = (H, W), sides 32 .. 512: Resize(size)
        and the any-size forward (reid_descriptor_images_u8_hw; seres18_ibn weights, exact fp32) - the script's VeRi geometry is
        (224, int(ratio * 224))."""
        _, _, ms = self._swin_crop_args((224, 224), mean_std)
        hw_out = None if size is None else check_hw(size)
        images = list(images)
        n = len(images)
        src, offs, hw, _keep = self._pack_images(images)
        nc = getattr(self, "num_class", 0)
        if nc <= 0:
            raise ValueError("a descriptor needs loaded weights with a classifier (Engine.load_seres18)")
        out = np.empty((n, self.embed_dim + nc), np.float32)
        if hw_out is not None:
            check(self.lib.reid_descriptor_images_u8_hw(self.h, src, _ptr(offs), _ptr(hw), n, hw_out[0], hw_out[1], _ptr(ms), int(bool(flip_tta)),
                                                        _ptr(out)))
            return out
        check(self.lib.reid_descriptor_images_u8(self.h, src, _ptr(offs), _ptr(hw), n, _ptr(ms), int(bool(flip_tta)), _ptr(out)))
        return out

    # ---- the shifted mirrored view of the script's strong_inference (reid/data_transforms.py:130-191)
    IMAGENET_MEAN_STD = (0.485, 0.456, 0.406, 0.229, 0.224, 0.225)   # the library's default for mean_std=None
    SHIFT_PAD_MAX = 32

    @staticmethod
    def normalised_zero_fill(mean_std=None):
        """float32 [3]: what a black (0) pixel becomes under ToTensor + Normalize(mean_std; None: ImageNet), in the arithmetic of the
        device's normalisation table (pil_resize_norm_table): t = fp32(0) / fp32(255); (t - mean) / std, every step rounded to fp32.
        The border of the shifted mirrored view - Pad(fill=0) on the 8-bit image comes before Normalize."""
        ms = np.asarray(Engine.IMAGENET_MEAN_STD if mean_std is None else mean_std, np.float32).reshape(-1)
        if ms.size != 6 or not np.isfinite(ms).all() or not (ms[3:] > 0).all():
            raise ValueError("mean_std must be (mean[3], std[3]) with finite values and std > 0, got %r" % (mean_std,))
        t = np.float32(0.0) / np.float32(255.0)
        return ((t - ms[:3]).astype(np.float32) / ms[3:]).astype(np.float32)

    @staticmethod
    def check_shift(shift_tl, n, pad):
        """(top, left) per image as int32 [n, 2] and pad, checked before any device call: pad in 0 .. 32, every shift in [0, 2 pad]."""
        if isinstance(pad, bool) or not isinstance(pad, (int, np.integer)) or not 0 <= pad <= Engine.SHIFT_PAD_MAX:
            raise ValueError("pad must be an integer in 0 .. %d, got %r" % (Engine.SHIFT_PAD_MAX, pad))
        tl = np.asarray(shift_tl)
        if tl.shape != (n, 2) or not np.issubdtype(tl.dtype, np.integer):
            raise ValueError("shift_tl must be integers [n, 2] = (top, left) per image for %d images, got %s %s" % (n, tl.dtype, tl.shape))
        bad = np.argwhere((tl < 0) | (tl > 2 * pad))
        if bad.size:
            i, k = (int(v) for v in bad[0])
            raise ValueError("shift_tl of image %d: %s %d outside [0, 2 pad = %d]" % (i, ("top", "left")[k], int(tl[i, k]), 2 * int(pad)))
        return np.ascontiguousarray(tl, dtype=np.int32), int(pad)

    def descriptor_f32_nchw_shift(self, x, shift_tl, pad=10, fill=None):
        """descriptor_f32_nchw(flip_tta=True) with the script's strong_inference second view: the mirrored image shifted by
        (top - pad, left - pad) = shift_tl[i] - pad over a border of ``fill`` [3] (None: normalised_zero_fill() for ImageNet), i.e.
        crop(pad(mirror(x))).  shift_tl == pad everywhere is the plain mirror and the bits of flip_tta=True
        (reid_descriptor_f32_nchw_shift)."""
        x = _f32(x)
        if x.ndim != 4 or x.shape[1] != 3:
            raise ValueError("descriptor_f32_nchw_shift expects [n,3,H,W] (%d x %d, or sides in [%d, %d]), got %s"
                             % (IMG_H, IMG_W, SIZE_MIN, SIZE_MAX, x.shape))
        h, w = check_hw(x.shape[2:])
        tl, pad = Engine.check_shift(shift_tl, x.shape[0], pad)
        fill = Engine.normalised_zero_fill() if fill is None else _f32(fill).reshape(-1)
        if fill.size != 3:
            raise ValueError("fill must be 3 floats (one per channel), got %r" % (fill,))
        out = np.empty((x.shape[0], self.embed_dim + self.num_class), np.float32)
        check(self.lib.reid_descriptor_f32_nchw_shift(self.h, _ptr(x), x.shape[0], h, w, _ptr(tl), pad, _ptr(fill), _ptr(out)))
        return out

    def descriptor_shift_dev(self, d_x, n, size, shift_tl, pad, fill, d_out):
        """reid_descriptor_f32_nchw_shift_dev: images and descriptors on the device, shift_tl / fill on the host."""
        h, w = check_hw(size)
        tl, pad = Engine.check_shift(shift_tl, int(n), pad)
        fill = _f32(fill).reshape(-1)
        if fill.size != 3:
            raise ValueError("fill must be 3 floats (one per channel), got %r" % (fill,))
        check(self.lib.reid_descriptor_f32_nchw_shift_dev(self.h, C.c_void_p(d_x), int(n), h, w, _ptr(tl), pad, _ptr(fill), C.c_void_p(d_out)))

    def descriptor_images_u8_shift(self, images, shift_tl, pad=10, mean_std=None, size=None):
        """descriptor_images_u8(flip_tta=True) with the shifted mirrored view as its second view; the border is the normalisation
        table's entry for pixel value 0 (normalised_zero_fill(mean_std)).  ``size`` None: (256, 128)
        (reid_descriptor_images_u8_shift)."""
        _, _, ms = self._swin_crop_args((224, 224), mean_std)
        h, w = (IMG_H, IMG_W) if size is None else check_hw(size)
        images = list(images)
        n = len(images)
        tl, pad = Engine.check_shift(shift_tl, n, pad)
        src, offs, hw, _keep = self._pack_images(images)
        nc = getattr(self, "num_class", 0)
        if nc <= 0:
            raise ValueError("a descriptor needs loaded weights with a classifier (Engine.load_seres18)")
        out = np.empty((n, self.embed_dim + nc), np.float32)
        check(self.lib.reid_descriptor_images_u8_shift(self.h, src, _ptr(offs), _ptr(hw), n, h, w, _ptr(ms), _ptr(tl), pad, _ptr(out)))
        return out

    # ---- the attribute distance of the Market-1501 evaluation (reid/image_reid_inference.py:276-289)
    def distmat_add_l2(self, a, inout):
        """inout [n, n] float32 += euclidean_dist(a, a) (reid/losses/utils.py:21-35), a [n, d], 1 <= d <= 32, in place; returns inout
        (reid_distmat_add_l2)."""
        a = _f32(a)
        if a.ndim != 2 or not isinstance(inout, np.ndarray) or inout.dtype != np.float32 or inout.shape != (a.shape[0], a.shape[0]) \
                or not inout.flags.c_contiguous:
            raise ValueError("distmat_add_l2 expects a [n, d] and a C-contiguous float32 inout [n, n]")
        check(self.lib.reid_distmat_add_l2(self.h, _ptr(a), a.shape[0], a.shape[1], _ptr(inout)))
        return inout

    def distmat_add_l2_dev(self, d_a, n, d, d_inout):
        check(self.lib.reid_distmat_add_l2_dev(self.h, C.c_void_p(d_a), int(n), int(d), C.c_void_p(d_inout)))

    def debug_shift_mirror(self, x, shift_tl, pad, fill):
        """shift_mirror_nchw_kernel through the launcher the *_shift entries call (reid_debug_shift_mirror): x [m, 3, h, w].  Returns
        (y [m, 3, h, w], guard [w])."""
        x = _f32(x)
        m, _, h, w = x.shape
        tl = np.ascontiguousarray(shift_tl, dtype=np.int32).reshape(m, 2)
        fill = _f32(fill).reshape(3)
        y = np.empty(x.size + w, np.float32)
        fn = _ffi.debug_lib().reid_debug_shift_mirror
        fn.restype = C.c_int
        check(fn(self.h, _ptr(x), C.c_int(m), C.c_int(h), C.c_int(w), _ptr(tl), C.c_int(int(pad)), _ptr(fill), _ptr(y)))
        return y[:-w].reshape(x.shape), y[-w:]

    def debug_dist_add_l2(self, a, inout):
        """dist_add_l2_kernel through the launcher reid_distmat_add_l2* call (reid_debug_dist_add_l2): a [n, d], inout [n, n] (not
        modified).  Returns (updated [n, n], guard [n])."""
        a = _f32(a)
        n, d = a.shape
        buf = np.empty(n * n + n, np.float32)
        buf[:n * n] = _f32(inout).reshape(-1)
        fn = _ffi.debug_lib().reid_debug_dist_add_l2
        fn.restype = C.c_int
        check(fn(self.h, _ptr(a), C.c_int(n), C.c_int(d), _ptr(buf)))
        return buf[:-n].reshape(n, n), buf[-n:]

    # ---- embedding
    def _outs(self, n, want_logits, dim=None, num_class=None):
        """Host arrays an embed call fills: emb[n, dim] and logits[n, num_class] or None (default sizes: the ResNet18-SE family's)."""
        emb = np.empty((n, self.embed_dim if dim is None else dim), np.float32)
        logits = np.empty((n, self.num_class if num_class is None else num_class), np.float32) if want_logits else None
        return emb, logits

    @staticmethod
    def _ret(emb, lg, logits):
        return (emb, lg) if logits else emb

    def embed_u8(self, crops, logits=False):
        """uint8[n,256,128,3] -> float32[n,512] (and logits[n,num_class])."""
        crops = np.ascontiguousarray(crops, dtype=np.uint8)
        if crops.ndim != 4 or crops.shape[1:] != (IMG_H, IMG_W, 3):
            raise ValueError("embed_u8 expects uint8[n,%d,%d,3], got %s" % (IMG_H, IMG_W, crops.shape))
        emb, lg = self._outs(crops.shape[0], logits)
        check(self.lib.reid_embed_u8(self.h, _ptr(crops), crops.shape[0], _ptr(emb), _ptr(lg)))
        return self._ret(emb, lg, logits)

    @staticmethod
    def _pack_ragged(crops):
        """list of uint8[h_i,w_i,3] -> (source pointer, offsets int64[n], hw int32[n,2], keep-alive).  Crops that already lie one after
        the other in ONE host buffer (views of a stacked array, slices of a pinned slab) are handed over in place - no packing copy."""
        n = len(crops)
        hw = np.empty((n, 2), np.int32)
        offs = np.empty(n, np.int64)
        total = 0
        flat = []
        base = None                              # address of crop 0 while every crop so far starts where the previous one ended
        for i, c in enumerate(crops):
            c = np.ascontiguousarray(c, dtype=np.uint8)
            if c.ndim != 3 or c.shape[2] != 3 or c.shape[0] < 1 or c.shape[1] < 1:
                raise ValueError("crop %d must be uint8[h,w,3], got %s" % (i, c.shape))
            hw[i] = c.shape[:2]
            offs[i] = total
            addr = c.__array_interface__["data"][0]
            if i == 0:
                base = addr
            elif base is not None and addr != base + total:
                base = None
            total += c.size
            flat.append(c)
        if base is not None and n:
            return C.c_void_p(base), offs, hw, flat        # `flat` keeps the views (and so their buffer) alive over the call
        packed = np.concatenate([c.reshape(-1) for c in flat]) if flat else np.empty(0, np.uint8)
        return _ptr(packed), offs, hw, packed

    def embed_ragged_u8(self, crops, logits=False, size=None, mean_std=None):
        """list of uint8[h_i,w_i,3] -> float32[n,512]; resize + normalise run on the device.  Crops that already lie one after
        the other in ONE host buffer (views of a stacked array, slices of a pinned slab) are handed over in place - no packing copy;
        more crops than a pass holds go up pass by pass under the kernels (csrc/api.hip reid_embed_ragged_u8).  ``size`` = (H, W), sides
        32 .. 512, resizes to that instead of (256, 128) and ``mean_std`` = (mean[3], std[3]) replaces the 0.5 / 0.5 of the tracker's
        Normalize (reid_embed_ragged_u8_hw; other sizes: seres18_ibn weights, exact fp32)."""
        hw_out = None if size is None else check_hw(size)
        if mean_std is not None and hw_out is None:
            hw_out = (IMG_H, IMG_W)
        _, _, ms = self._swin_crop_args((224, 224), mean_std)
        n = len(crops)
        src, offs, hw, _keep = self._pack_ragged(crops)
        emb, lg = self._outs(n, logits)
        if hw_out is not None:
            check(self.lib.reid_embed_ragged_u8_hw(self.h, src, _ptr(offs), _ptr(hw), n, hw_out[0], hw_out[1], _ptr(ms), _ptr(emb), _ptr(lg)))
            return self._ret(emb, lg, logits)
        check(self.lib.reid_embed_ragged_u8(self.h, src, _ptr(offs), _ptr(hw), n, _ptr(emb), _ptr(lg)))
        return self._ret(emb, lg, logits)

    # ---- frame pipeline (csrc/bank.hip): submit (asynchronous) / cost (the frame's one synchronisation) / update (asynchronous)
    def pinned(self, nbytes):
        """uint8 numpy array over pinned host memory (freed with the engine)."""
        p = C.c_void_p()
        check(self.lib.reid_host_alloc(self.h, int(nbytes), C.byref(p)))
        self._pinned = getattr(self, "_pinned", [])
        self._pinned.append(p)
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(int(nbytes),))

    def _frame_pack(self, slot, crops):
        """The ragged uint8 crops of a frame into the slot's pinned slab: (slab, offsets int64[n], hw int32[n,2], n)."""
        n = len(crops)
        hw = np.empty((n, 2), np.int32)
        offs = np.empty(n, np.int64)
        total = 0
        for i, c in enumerate(crops):
            if c.ndim != 3 or c.shape[2] != 3 or c.shape[0] < 1 or c.shape[1] < 1 or c.dtype != np.uint8:
                raise ValueError("crop %d must be uint8[h,w,3], got %s %s" % (i, c.dtype, c.shape))
            hw[i] = c.shape[:2]
            offs[i] = total
            total += c.size
        slabs = self.__dict__.setdefault("_slabs", {})
        slab = slabs.get(slot)
        if slab is None or slab.size < total:
            self.sync()          # the old slab may still be the source of an upload
            if slab is not None:                 # superseded: give its pinned memory back now, not at close()
                old = slab.ctypes.data
                for p in list(self._pinned):
                    if p.value == old:
                        self.lib.reid_host_free(self.h, p)
                        self._pinned.remove(p)
            slab = slabs[slot] = self.pinned(max(2 * total, 1 << 22))
        for i, c in enumerate(crops):   # straight into pinned memory: the only host copy of the pixels
            slab[offs[i]: offs[i] + c.size].reshape(c.shape)[...] = c
        return slab, offs, hw, n

    def frame_submit(self, slot, crops):
        """Stage 1: pack the ragged uint8 crops into the slot's pinned slab, enqueue upload + resize + forward; returns at once."""
        slab, offs, hw, n = self._frame_pack(slot, crops)
        check(self.lib.reid_frame_submit(self.h, int(slot), _ptr(slab), _ptr(offs), _ptr(hw), n))
        self.__dict__.setdefault("_frame_n", {})[slot] = n
        self.__dict__.setdefault("_frame_d", {})[slot] = 512
        return n

    def frame_submit_swin(self, slot, crops, size=(224, 224), mean_std=None):
        """Stage 1 for a Swin tracker (reid_frame_submit_swin): as frame_submit, with the forward of swin_embed_ragged_u8 - ``size`` and
        ``mean_std`` as there, checked before any device call.  The slot's embeddings are [n, swin_dim] (96) wide."""
        h, w, ms = self._swin_crop_args(size, mean_std)
        slab, offs, hw, n = self._frame_pack(slot, crops)
        check(self.lib.reid_frame_submit_swin(self.h, int(slot), _ptr(slab), _ptr(offs), _ptr(hw), n, h, w, _ptr(ms)))
        self.__dict__.setdefault("_frame_n", {})[slot] = n
        self.__dict__.setdefault("_frame_d", {})[slot] = self.swin_dim
        return n

    @staticmethod
    def _hw_crop_args(size, mean_std):
        """(H, W) with each side in 32 .. 512 and mean[3] / std[3] (None: the library's 0.5 / 0.5), checked before any device call."""
        h, w = check_hw(size)
        _, _, ms = Engine._swin_crop_args((224, 224), mean_std)
        return h, w, ms

    def frame_submit_hw(self, slot, crops, size, mean_std=None):
        """Stage 1 for a ResNet18-IBN-SE tracker at another crop size (reid_frame_submit_hw): as frame_submit, with the forward of
        embed_ragged_u8(size=) - ``size`` = (H, W), sides 32 .. 512, and ``mean_std`` as there, checked before any device call.  (256, 128)
        is frame_submit; any other size opens with the fused resize + stem + max-pool kernel (libreid_hip_anysize_front.so)."""
        h, w, ms = self._hw_crop_args(size, mean_std)
        slab, offs, hw, n = self._frame_pack(slot, crops)
        check(self.lib.reid_frame_submit_hw(self.h, int(slot), _ptr(slab), _ptr(offs), _ptr(hw), n, h, w, _ptr(ms)))
        self.__dict__.setdefault("_frame_n", {})[slot] = n
        self.__dict__.setdefault("_frame_d", {})[slot] = 512
        return n

    def frame_dim(self, slot):
        """Width d of the embeddings of the frame last submitted to ``slot``: 512 (frame_submit, frame_submit_hw) or the Swin's 96 (frame_submit_swin)."""
        return self.__dict__.get("_frame_d", {}).get(slot, 512)

    def frame_gather(self, slot, per, world):
        """Multi-GPU frames: all-gather the ranks' embeddings of the submitted frame into the slot (equal blocks of `per` rows);
        the slot then holds world * per rows on every rank (`parallel.frame_rows` maps detections to them)."""
        if world > 1:
            rank, w = C.c_int(), C.c_int()
            check(self.lib.reid_comm_info(self.h, C.byref(rank), C.byref(w)))
            if w.value != world:
                raise RuntimeError("frame_gather over %d ranks needs the C-ABI communicator (reid_comm_init); it spans %d" % (world, w.value))
        check(self.lib.reid_frame_gather(self.h, int(slot), int(per)))
        if per > 0:
            self._frame_n[slot] = int(world) * int(per)

    def frame_cost(self, slot, bank=None, slots=None, metric=0, max_dist=-1.0, track_boxes=None, det_boxes=None, want_emb=True):
        """Stage 2 (asynchronous): enqueue the appearance cost / DIoU cost of the submitted frame; `frame_fetch` collects."""
        m = self._frame_n[slot]
        t = 0 if slots is None else len(slots)
        tb = db = None
        if track_boxes is not None and det_boxes is not None:
            tb = np.ascontiguousarray(track_boxes, np.float64).reshape(-1, 4)
            db = np.ascontiguousarray(det_boxes, np.float64).reshape(-1, 4)
            if db.shape[0] != m:
                raise ValueError("det_boxes has %d rows for %d submitted crops" % (db.shape[0], m))
            if slots is not None and tb.shape[0] != t:
                raise ValueError("track_boxes has %d rows for %d tracks" % (tb.shape[0], t))
            t = tb.shape[0]
        sl = None if slots is None else np.ascontiguousarray(slots, np.int32)
        check(self.lib.reid_frame_cost(self.h, int(slot), bank if sl is not None else None, _ptr(sl), t, int(metric),
                                       C.c_float(max_dist), _ptr(tb), _ptr(db), 1 if want_emb else 0))
        self.__dict__.setdefault("_frame_q", {})[slot] = (m, t, want_emb, bank is not None and sl is not None and t and m,
                                                          tb is not None and t and m)

    def frame_fetch(self, slot):
        """The frame's one wait: (emb[m,d] | None, cost[t,m] float32 | None, iou_cost[t,m] float64 | None); d = frame_dim(slot)."""
        m, t, want_emb, has_cost, has_iou = self._frame_q.pop(slot)
        emb = np.empty((m, self.frame_dim(slot)), np.float32) if want_emb else None
        cost = np.empty((t, m), np.float32) if has_cost else None
        iou = np.empty((t, m), np.float64) if has_iou else None
        check(self.lib.reid_frame_fetch(self.h, int(slot), _ptr(emb) if m else None, _ptr(cost), _ptr(iou)))
        return emb, cost, iou

    def frame_match_stream(self, on=True):
        """Cost / update stages of the frame pipeline (and every other access to this context's banks) on a stream of their own
        (reid_frame_match_stream): a look-ahead group's frame-by-frame chain then runs beside the next group's forward."""
        check(self.lib.reid_frame_match_stream(self.h, 1 if on else 0))

    def frame_cost_groups(self, slot, groups, metric=0, max_dist=-1.0, want_emb=True):
        """Stage 2 for K camera streams batched into one slot (reid_frame_cost_groups): ``groups`` = one (bank, slots, track_boxes,
        det_boxes, m) per camera, in the order their crops were submitted; camera g's tracks meet ITS m detections only."""
        k = len(groups)
        banks = (C.c_void_p * k)()
        tc, mc = np.zeros(k, np.int32), np.zeros(k, np.int32)
        sl, tb, db = [], [], []
        boxes = all(g[2] is not None and g[3] is not None for g in groups)
        for i, (bank, slots, tboxes, dboxes, m) in enumerate(groups):
            banks[i] = bank
            tc[i], mc[i] = (0 if slots is None else len(slots)), int(m)
            if slots is not None:
                sl.append(np.asarray(slots, np.int32))
            if boxes:
                t4 = np.asarray(tboxes, np.float64).reshape(-1, 4)
                d4 = np.asarray(dboxes, np.float64).reshape(-1, 4)
                if t4.shape[0] != tc[i] or d4.shape[0] != mc[i]:
                    raise ValueError("camera %d: %d / %d boxes for %d tracks / %d crops" % (i, t4.shape[0], d4.shape[0], tc[i], mc[i]))
                tb.append(t4)
                db.append(d4)
        if int(mc.sum()) != self._frame_n[slot]:
            raise ValueError("the groups hold %d detections, the slot %d" % (int(mc.sum()), self._frame_n[slot]))
        sl = np.ascontiguousarray(np.concatenate(sl), np.int32) if sl else None
        tb = np.ascontiguousarray(np.concatenate(tb)) if boxes else None
        db = np.ascontiguousarray(np.concatenate(db)) if boxes else None
        check(self.lib.reid_frame_cost_groups(self.h, int(slot), k, banks if sl is not None else None, _ptr(tc), _ptr(mc), _ptr(sl), int(metric),
                                              C.c_float(max_dist), _ptr(tb), _ptr(db), 1 if want_emb else 0))
        tm = int((tc.astype(np.int64) * mc).sum())
        self.__dict__.setdefault("_frame_q", {})[slot] = (self._frame_n[slot], tm, want_emb, sl is not None and tm > 0, boxes and tm > 0, tc, mc)

    def frame_fetch_groups(self, slot):
        """The one wait of a batched frame: (emb[m,d] | None, [cost_g[t_g,m_g] float32 | None], [iou_g float64 | None]); d = frame_dim(slot)."""
        m, tm, want_emb, has_cost, has_iou, tc, mc = self._frame_q.pop(slot)
        emb = np.empty((m, self.frame_dim(slot)), np.float32) if want_emb else None
        cost = np.empty(tm, np.float32) if has_cost else None
        iou = np.empty(tm, np.float64) if has_iou else None
        check(self.lib.reid_frame_fetch(self.h, int(slot), _ptr(emb) if m else None, _ptr(cost), _ptr(iou)))
        offs = np.concatenate([[0], np.cumsum(tc.astype(np.int64) * mc)])
        cut = lambda a: [None if a is None else a[offs[g]:offs[g + 1]].reshape(int(tc[g]), int(mc[g])) for g in range(len(tc))]
        return emb, cut(cost), cut(iou)

    def frame_update(self, slot, bank, rows, slots):
        """Stage 3: partial_fit from the slot's device-resident embeddings (row rows[i] -> track slot slots[i]); asynchronous."""
        rows = np.ascontiguousarray(rows, np.int32)
        slots = np.ascontiguousarray(slots, np.int32)
        check(self.lib.reid_frame_update(self.h, int(slot), bank, _ptr(rows), _ptr(slots), len(rows)))

    def embed_frame_u8(self, frame, boxes_xyxy, logits=False, size=None, mean_std=None):
        """uint8[H,W,3] frame + int boxes [n,4] (x1,y1,x2,y2; crop = frame[y1:y2, x1:x2]) -> float32[n,512].  ``size`` = (H, W), sides
        32 .. 512, and ``mean_std`` as embed_ragged_u8 (reid_embed_frame_u8_hw: the same bits as embed_ragged_u8(size=) on the slices)."""
        hw_out = None if size is None else check_hw(size)
        if mean_std is not None and hw_out is None:
            hw_out = (IMG_H, IMG_W)
        _, _, ms = self._swin_crop_args((224, 224), mean_std)
        frame = np.ascontiguousarray(frame, dtype=np.uint8)
        if frame.ndim != 3 or frame.shape[2] != 3:
            raise ValueError("frame must be uint8[H,W,3], got %s" % (frame.shape,))
        boxes = np.ascontiguousarray(boxes_xyxy, dtype=np.int32).reshape(-1, 4)
        n = boxes.shape[0]
        emb, lg = self._outs(n, logits)
        if hw_out is not None:
            check(self.lib.reid_embed_frame_u8_hw(self.h, _ptr(frame), frame.shape[0], frame.shape[1], _ptr(boxes), n, hw_out[0], hw_out[1],
                                                  _ptr(ms), _ptr(emb), _ptr(lg)))
            return self._ret(emb, lg, logits)
        check(self.lib.reid_embed_frame_u8(self.h, _ptr(frame), frame.shape[0], frame.shape[1], _ptr(boxes), n, _ptr(emb),
                                           _ptr(lg)))
        return self._ret(emb, lg, logits)

    def embed_f32_nchw(self, x, logits=False):
        """float32 [n,3,H,W] -> float32 [n,512] (and logits).  (256, 128) runs the loaded architecture in the context's precision;
        any other H, W in 32 .. 512 the any-size forward (reid_embed_f32_nchw_hw: seres18_ibn weights - cares18_ibn with set_hw_siblings(True),
        emares18_ibn with set_hw_ema(True) -
        in exact fp32, or the arithmetic set_hw_precision names)."""
        x = _f32(x)
        if x.ndim != 4 or x.shape[1] != 3:
            raise ValueError("embed_f32_nchw expects float32[n,3,H,W] (%d x %d, or sides in [%d, %d]), got %s"
                             % (IMG_H, IMG_W, SIZE_MIN, SIZE_MAX, x.shape))
        h, w = check_hw(x.shape[2:])
        emb, lg = self._outs(x.shape[0], logits)
        if (h, w) != (IMG_H, IMG_W):
            check(self.lib.reid_embed_f32_nchw_hw(self.h, _ptr(x), x.shape[0], h, w, _ptr(emb), _ptr(lg)))
            return self._ret(emb, lg, logits)
        check(self.lib.reid_embed_f32_nchw(self.h, _ptr(x), x.shape[0], _ptr(emb), _ptr(lg)))
        return self._ret(emb, lg, logits)

    def embed_f32_nchw_dev(self, d_x, n, d_emb, d_logits=None, size=None):
        if size is not None:
            h, w = check_hw(size)
            check(self.lib.reid_embed_f32_nchw_hw_dev(self.h, C.c_void_p(d_x), int(n), h, w, C.c_void_p(d_emb), C.c_void_p(d_logits or 0)))
            return
        check(self.lib.reid_embed_f32_nchw_dev(self.h, C.c_void_p(d_x), int(n), C.c_void_p(d_emb), C.c_void_p(d_logits or 0)))

    def embed_u8_dev(self, d_crops, n, d_emb, d_logits=None):
        check(self.lib.reid_embed_u8_dev(self.h, C.c_void_p(d_crops), int(n), C.c_void_p(d_emb),
                                         C.c_void_p(d_logits or 0)))

    def debug_switch(self, name, value=None):
        """Experiment switch of this context through libreid_hip_debug.so (include/reid_hip_debug.h: reid_debug_set_switch); with
        ``value`` None returns the current value.  The product library itself takes no such switch from the environment."""
        dbg = _ffi.debug_lib()
        if value is None:
            v = C.c_longlong()
            check(dbg.reid_debug_get_switch(self.h, name.encode(), C.byref(v)))
            return v.value
        check(dbg.reid_debug_set_switch(self.h, name.encode(), C.c_longlong(int(value))))

    def debug_mfma_bare(self, shape, zero=False, iters=20000):
        """TFLOP/s of a registers-only f16 MFMA loop on this device (libreid_hip_debug.so, microbench.hip): shape 32 = 32x32x16,
        16 = 16x16x32; random operands unless ``zero``."""
        tf = C.c_float()
        check(_ffi.debug_lib().reid_debug_mfma_bare(self.h, int(shape), int(bool(zero)), int(iters), C.byref(tf)))
        return tf.value

    def debug_switches_from_env(self):
        """A/B tools: REID_DEBUG_SWITCHES="name=value,name=value" -> debug_switch calls (read by the TOOL, in Python)."""
        import os
        spec = os.environ.get("REID_DEBUG_SWITCHES", "")
        for item in filter(None, (t.strip() for t in spec.split(","))):
            name, _, val = item.partition("=")
            self.debug_switch(name.strip(), int(val))
        return spec

    def debug_keep(self, on):
        check(self.lib.reid_ctx_set_debug_keep(self.h, int(on)))

    def debug_stage(self, stage, n, size=None):
        """Tap ``stage`` of the last pass (n images) as a flat array; ``size`` = (H, W) of that pass's input when it was not 256 x 128."""
        sizes = [524288, 131072, 131072, 131072, 65536, 65536, 32768, 32768, 65536, 65536, 512]
        if size is not None:
            sizes = [a * b * c for a, b, c in stage_shapes(*check_hw(size))] + [512]
        out = np.empty(sizes[stage] * n, np.float32)
        cnt = C.c_size_t()
        check(self.lib.reid_debug_stage(self.h, int(stage), _ptr(out), out.size, C.byref(cnt)))
        assert cnt.value == out.size
        return out

    def debug_conv_layer(self, x, w, stride=1, pad=0, scale=None, shift=None, residual=None, relu=False, relu_from=0, pack_from=-1,
                         stats=False, a_scale=None, a_shift=None, a_relu=False):
        """One ResNet-trunk convolution through the forward's launcher (libreid_hip_debug.so reid_debug_conv_layer) in this context's
        precision and switches.  x [n,h,w,cin], w [cout,r,r,cin] fp32.  Returns (out [n,ho,wo,cout] fp32, packed [m, 2 cout] uint16
        f16 bits or None, stats [m / 128, cout, 2] or None); packed is None unless pack_from >= 0 and the launch wrote that form.
        What the launch does not write reads as NaN."""
        x, w = _f32(x), _f32(w)
        n, h, ww, cin = x.shape
        cout, r, s, wc = w.shape
        if r != s or wc != cin:
            raise ValueError("debug_conv_layer expects w[cout, r, r, cin] matching x")
        ho, wo = (h + 2 * pad - r) // stride + 1, (ww + 2 * pad - r) // stride + 1
        m = n * ho * wo
        out = np.empty((n, ho, wo, cout), np.float32)
        pk = np.empty((m, 2 * cout), np.uint16) if pack_from >= 0 else None
        st = np.empty((m // 128, cout, 2), np.float32) if stats else None
        opt = [_f32(a) if a is not None else None for a in (scale, shift, residual, a_scale, a_shift)]
        written = C.c_int(0)
        check(_ffi.debug_lib().reid_debug_conv_layer(
            self.h, _ptr(x), C.c_int(n), C.c_int(h), C.c_int(ww), C.c_int(cin), _ptr(w), C.c_int(cout), C.c_int(r), C.c_int(stride),
            C.c_int(pad), _ptr(opt[0]), _ptr(opt[1]), _ptr(opt[2]), C.c_int(int(bool(relu))), C.c_int(int(relu_from)),
            C.c_int(int(pack_from)), C.c_int(int(bool(stats))), _ptr(opt[3]), _ptr(opt[4]), C.c_int(int(bool(a_relu))), _ptr(out),
            _ptr(pk), _ptr(st), C.byref(written)))
        return out, (pk if written.value else None), st

    def debug_conv_layer_f16(self, x, w, stride=1, pad=0, scale=None, shift=None, residual=None, relu=False, stats=False):
        """One convolution of the fp16-storage trunk through conv_gemm16, the forward's call (libreid_hip_debug.so
        reid_debug_conv_layer_f16).  x [n,h,w,cin], w [cout,r,r,cin], residual [n,ho,wo,cout]: float16 arrays (or their uint16 bits),
        handed over bit for bit.  Returns (out [n,ho,wo,cout] float16, stats [m / 128, cout, 2] fp32 or None, form): form names the
        launch that was made (include/reid_hip_debug.h).  What the launch does not write reads as NaN."""
        bits = lambda a: None if a is None else np.ascontiguousarray(a).view(np.uint16)
        xb, wb, rb = bits(x), bits(w), bits(residual)
        n, h, ww, cin = xb.shape
        cout, r, s, wc = wb.shape
        if r != s or wc != cin:
            raise ValueError("debug_conv_layer_f16 expects w[cout, r, r, cin] matching x")
        ho, wo = (h + 2 * pad - r) // stride + 1, (ww + 2 * pad - r) // stride + 1
        if rb is not None and rb.size != n * ho * wo * cout:
            raise ValueError("debug_conv_layer_f16: residual must be [n, ho, wo, cout]")
        out = np.empty((n, ho, wo, cout), np.uint16)
        st = np.empty((n * ho * wo // 128, cout, 2), np.float32) if stats else None
        sc, sh = (None if a is None else _f32(a) for a in (scale, shift))
        form = C.c_int(0)
        check(_ffi.debug_lib().reid_debug_conv_layer_f16(
            self.h, _ptr(xb), C.c_int(n), C.c_int(h), C.c_int(ww), C.c_int(cin), _ptr(wb), C.c_int(cout), C.c_int(r), C.c_int(stride),
            C.c_int(pad), _ptr(sc), _ptr(sh), _ptr(rb), C.c_int(int(bool(relu))), C.c_int(int(bool(stats))), _ptr(out), _ptr(st),
            C.byref(form)))
        return out.view(np.float16), st, form.value

    def debug_conv_c64_se(self, x, w_folded, shift=None, residual=None, relu=False, se_w1=None, se_w2t=None, stats=False):
        """The layer-1 kernel (conv3x3_c64_f16.hip) on raw operands (libreid_hip_debug.so reid_debug_conv_c64_se): x / residual
        [n,64,32,64] and w_folded [64,576] float16 (or uint16 bits), shift [64] fp32; se_w1 / se_w2t [8,64] fp32 ask for the fused SE
        tail.  Returns (out [n,64,32,64] float16, stats [n,64,2] or None, form)."""
        bits = lambda a: None if a is None else np.ascontiguousarray(a).view(np.uint16)
        xb, wb, rb = bits(x), bits(w_folded), bits(residual)
        n = xb.shape[0]
        if xb.shape[1:] != (64, 32, 64) or wb.size != 64 * 576 or (rb is not None and rb.shape != xb.shape):
            raise ValueError("debug_conv_c64_se expects x / residual [n, 64, 32, 64] and w_folded [64, 576]")
        out = np.empty(xb.shape, np.uint16)
        st = np.empty((n, 64, 2), np.float32) if stats else None
        sh, w1, w2 = (None if a is None else _f32(a) for a in (shift, se_w1, se_w2t))
        if (sh is not None and sh.size != 64) or any(a is not None and a.size != 512 for a in (w1, w2)):
            raise ValueError("debug_conv_c64_se expects shift [64] and se_w1 / se_w2t [8, 64]")
        form = C.c_int(0)
        check(_ffi.debug_lib().reid_debug_conv_c64_se(
            self.h, C.c_int(n), _ptr(xb), _ptr(wb), _ptr(sh), _ptr(rb), C.c_int(int(bool(relu))), _ptr(w1), _ptr(w2), _ptr(out), _ptr(st),
            C.byref(form)))
        return out.view(np.float16), st, form.value

    def debug_norm_finish(self, form, x, stats, in_gamma, in_beta, bn_scale=None, bn_shift=None, hw=None):
        """The IBN finish of conv1 through the forward's launcher (libreid_hip_debug.so reid_debug_norm_finish).  x [n, hw, c] (fp32,
        or uint16 f16 bits for forms 4 and 5) or None for form 0; stats [n, tiles, c, 2]; in_gamma / in_beta [half].  Returns
        (out, out16, a_scale, a_shift), None where the form has no such output: out [n, hw, c] fp32 (forms 1-3), out16 [n hw, 2c]
        (forms 2-3) or [n, hw, c] (forms 4-5) uint16, a_scale / a_shift [n, c] (forms 0, 5).  Form 0 takes the image size as hw.
        Unwritten outputs read as NaN."""
        stats = _f32(stats)
        n, tiles, c, _ = stats.shape
        half = int(np.asarray(in_gamma).size)
        hw = int(hw) if x is None else x.shape[1]
        xa = None if form == 0 else (np.ascontiguousarray(x, np.uint16) if form >= 4 else _f32(x))
        out = np.empty((n, hw, c), np.float32) if 1 <= form <= 3 else None
        o16 = np.empty((n * hw, 2 * c), np.uint16) if form in (2, 3) else (np.empty((n, hw, c), np.uint16) if form >= 4 else None)
        ab = [np.empty((n, c), np.float32) for _ in range(2)] if form in (0, 5) else [None, None]
        opt = [_f32(a) if a is not None else None for a in (in_gamma, in_beta, bn_scale, bn_shift)]
        check(_ffi.debug_lib().reid_debug_norm_finish(
            self.h, C.c_int(form), C.c_int(n), C.c_int(hw), C.c_int(c), C.c_int(half), C.c_int(tiles), _ptr(xa), _ptr(stats),
            _ptr(opt[0]), _ptr(opt[1]), _ptr(opt[2]), _ptr(opt[3]), _ptr(out), _ptr(o16), _ptr(ab[0]), _ptr(ab[1])))
        return out, o16, ab[0], ab[1]

    def debug_se_tail(self, form, stats, w1, w2t, y, shortcut):
        """The SE gate + combine through the forward's launchers (libreid_hip_debug.so reid_debug_se_tail; forms in
        include/reid_hip_debug.h).  stats [n, tiles, c, 2], w1 / w2t [mid, c], y / shortcut [n, hw, c] (fp32, or uint16 f16 bits for
        forms 10-11).  Returns (out [n, hw, c] fp32, out16 [n hw, 2c] packed or [n, hw, c] f16 bits, gate [n, c]), None where the form
        has no such output.  Unwritten outputs read as NaN."""
        stats = _f32(stats)
        n, tiles, c, _ = stats.shape
        mid = w1.shape[0]
        hw = y.shape[1]
        f16 = form >= 10
        cv = (lambda a: np.ascontiguousarray(a, np.uint16)) if f16 else _f32
        ya, sa = cv(y), cv(shortcut)
        tail = 1 <= form <= 9
        want_out = not f16 and (not tail or (form - 1) % 3 != 1)
        want_pk = tail and (form - 1) % 3 != 0
        out = np.empty((n, hw, c), np.float32) if want_out else None
        o16 = np.empty((n, hw, c), np.uint16) if f16 else (np.empty((n * hw, 2 * c), np.uint16) if want_pk else None)
        gate = np.empty((n, c), np.float32) if form in (0, 11) else None
        check(_ffi.debug_lib().reid_debug_se_tail(
            self.h, C.c_int(form), C.c_int(n), C.c_int(hw), C.c_int(c), C.c_int(mid), C.c_int(tiles), _ptr(stats), _ptr(_f32(w1)),
            _ptr(_f32(w2t)), _ptr(ya), _ptr(sa), _ptr(out), _ptr(o16), _ptr(gate)))
        return out, o16, gate

    def debug_sibling_tail(self, arch, prm, y, shortcut):
        """The exact-fp32 TripletAttention (arch 1) / EMA (arch 2) tail through the forward's launcher (libreid_hip_debug.so
        reid_debug_sibling_tail).  y / shortcut [n, h, w, c] fp32; returns relu(tail(y) + shortcut) [n, h, w, c].  Unwritten outputs read as NaN."""
        y, shortcut = _f32(y), _f32(shortcut)
        n, h, w, c = y.shape
        out = np.empty((n, h, w, c), np.float32)
        check(_ffi.debug_lib().reid_debug_sibling_tail(self.h, C.c_int(arch), C.c_int(n), C.c_int(h), C.c_int(w), C.c_int(c), _ptr(_f32(prm)),
                                                       _ptr(y), _ptr(shortcut), _ptr(out)))
        return out

    def debug_gem_neck(self, x, p, scale, shift, f16=False):
        """GeM + BNNeck through the forward's launcher (libreid_hip_debug.so reid_debug_gem_neck).  x [n, hw, c] fp32 (or uint16 f16
        bits with f16=True).  Returns (gem [n, c], emb [n, c])."""
        x = np.ascontiguousarray(x, np.uint16) if f16 else _f32(x)
        n, hw, c = x.shape
        g, e = np.empty((n, c), np.float32), np.empty((n, c), np.float32)
        check(_ffi.debug_lib().reid_debug_gem_neck(
            self.h, C.c_int(int(bool(f16))), C.c_int(n), C.c_int(hw), C.c_int(c), C.c_float(p), _ptr(x), _ptr(_f32(scale)),
            _ptr(_f32(shift)), _ptr(g), _ptr(e)))
        return g, e

    def debug_gem_neck_fused(self, stats, w1, w2t, y, shortcut, p, scale, shift):
        """GeM + BNNeck of the last block's tail in one launch (libreid_hip_debug.so reid_debug_gem_neck_fused): operands as in
        debug_se_tail (fp32) and debug_gem_neck.  Returns (gem [n, c], emb [n, c])."""
        stats = _f32(stats)
        n, tiles, c, _ = stats.shape
        y, shortcut = _f32(y), _f32(shortcut)
        g, e = np.empty((n, c), np.float32), np.empty((n, c), np.float32)
        check(_ffi.debug_lib().reid_debug_gem_neck_fused(
            self.h, C.c_int(n), C.c_int(y.shape[1]), C.c_int(c), C.c_int(w1.shape[0]), C.c_int(tiles), C.c_float(p), _ptr(stats),
            _ptr(_f32(w1)), _ptr(_f32(w2t)), _ptr(y), _ptr(shortcut), _ptr(_f32(scale)), _ptr(_f32(shift)), _ptr(g), _ptr(e)))
        return g, e

    def debug_stem(self, form, x, w, scale, shift):
        """The stem + max-pool through the forward's launchers (libreid_hip_debug.so reid_debug_stem; forms in include/reid_hip_debug.h).
        x [n, 256, 128, 3] uint8 crops or fp32 (already normalised), w [64, 7, 7, 3].  Returns (out, out16), None where the form has no
        such output: out fp32 [n, 128, 64, 64] (form 0) or [n, 64, 32, 64] (1, 2, 6); out16 uint16 f16 bits [n 64 32, 128] = [xh | xl']
        (form 2) or [n, 64, 32, 64] (3-5).  Unwritten outputs read as NaN."""
        is_u8 = np.asarray(x).dtype == np.uint8
        x = np.ascontiguousarray(x, np.uint8) if is_u8 else _f32(x)
        n = x.shape[0]
        if x.shape[1:] != (IMG_H, IMG_W, 3) or np.shape(w) != (64, 7, 7, 3):
            raise ValueError("debug_stem expects x[n, 256, 128, 3] and w[64, 7, 7, 3]")
        out = np.empty((n, 128, 64, 64) if form == 0 else (n, 64, 32, 64), np.float32) if form in (0, 1, 2, 6) else None
        o16 = np.empty((n * 2048, 128), np.uint16) if form == 2 else (np.empty((n, 64, 32, 64), np.uint16) if form in (3, 4, 5) else None)
        check(_ffi.debug_lib().reid_debug_stem(self.h, C.c_int(form), C.c_int(int(is_u8)), _ptr(x), C.c_int(n), _ptr(_f32(w)),
                                               _ptr(_f32(scale)), _ptr(_f32(shift)), _ptr(out), _ptr(o16)))
        return out, o16

    def debug_resize_norm(self, packed, offsets, hw, pitch=0):
        """resize_norm_kernel through its launcher (reid_debug_resize_norm): windows of hw[i] = (h, w) pixels at byte offsets[i] of the
        uint8 buffer `packed`, rows `pitch` pixels apart (0: packed crops).  Returns fp32 [n, 256, 128, 3]."""
        packed = np.ascontiguousarray(packed, np.uint8).reshape(-1)
        offsets = np.ascontiguousarray(offsets, np.int64)
        hw = np.ascontiguousarray(hw, np.int32).reshape(-1, 2)
        n = len(offsets)
        end = max(int(o) + ((int(h) - 1) * (pitch or int(w)) + int(w)) * 3 for o, (h, w) in zip(offsets, hw))
        if len(hw) != n or end > packed.size:
            raise ValueError("debug_resize_norm: a window leaves the buffer")
        out = np.empty((n, IMG_H, IMG_W, 3), np.float32)
        check(_ffi.debug_lib().reid_debug_resize_norm(self.h, _ptr(packed), _ptr(offsets), _ptr(hw), C.c_int(n), C.c_int(int(pitch)), _ptr(out)))
        return out

    def debug_pil_resize(self, images, size, mean_std=None, want_u8=True, packed=None, offsets=None, hw=None):
        """The two kernels of libreid_hip_pil_resize.so through the launcher the *_images_u8 entries call (reid_debug_pil_resize):
        list of uint8[h_i,w_i,3] -> (uint8 [n, H, W, 3] = PIL's Image.resize((W, H), BILINEAR), float32 [n, 3, H, W] = ToTensor +
        Normalize of it); ``size`` = (H, W), each from 1 to 1024.  ``packed`` / ``offsets`` / ``hw`` instead of ``images``: the raw
        arguments (items may share source bytes, offsets in any order).  Floats the launch leaves alone read NaN."""
        try:
            h, w = (int(v) for v in size)
        except (TypeError, ValueError):
            raise ValueError("size must be (H, W), got %r" % (size,))
        if not (1 <= h <= 1024 and 1 <= w <= 1024):
            raise ValueError("debug_pil_resize: output sides from 1 to 1024, got %r" % (size,))
        _, _, ms = self._swin_crop_args((224, 224), mean_std)
        if packed is None:
            src, offs, hws, _keep = self._pack_images(list(images))
        else:
            packed = np.ascontiguousarray(packed, np.uint8).reshape(-1)
            offs = np.ascontiguousarray(offsets, np.int64).reshape(-1)
            hws = np.ascontiguousarray(hw, np.int32).reshape(-1, 2)
            if len(hws) != len(offs) or len(offs) < 1 or int(offs.min()) < 0 or int(hws.min()) < 1 or int(hws.max()) > self.PIL_MAX_SIDE or \
                    max(int(o) + int(a) * int(b) * 3 for o, (a, b) in zip(offs, hws)) > packed.size:
                raise ValueError("debug_pil_resize: an image leaves the buffer or the limits")
            src = _ptr(packed)
        n = len(offs)
        if n < 1:
            raise ValueError("debug_pil_resize: at least one image")
        u8 = np.empty((n, h, w, 3), np.uint8) if want_u8 else None
        f32 = np.empty((n, 3, h, w), np.float32)
        check(_ffi.debug_lib().reid_debug_pil_resize(self.h, src, _ptr(offs), _ptr(hws), C.c_int(n), C.c_int(h), C.c_int(w), _ptr(ms), _ptr(u8),
                                                     _ptr(f32)))
        return u8, f32

    def debug_bank_cost96(self, bank, slots, dets, metric=_ffi.METRIC_COS, gate=None):
        """reid_debug_bank_cost96: the frame pipeline's cost launch for a 96-wide bank handle on host operands -> cost[t, m] float32
        (entries the launch leaves alone read NaN)."""
        sl = np.ascontiguousarray(slots, np.int32)
        x = np.ascontiguousarray(dets, np.float32).reshape(-1, 96)
        out = np.full((len(sl), len(x)), np.nan, np.float32)
        check(_ffi.debug_lib().reid_debug_bank_cost96(self.h, bank, _ptr(sl), len(sl), _ptr(x), len(x), int(metric),
                                                      C.c_float(-1.0 if gate is None else gate), _ptr(out)))
        return out

    def debug_swin_crop_front(self, packed, offsets, hw, c1_w, c1_b, size=(224, 224), mean_std=None, pitch=0, mirror=False):
        """swin_crop_front_kernel alone through its launcher (reid_debug_swin_crop_front): windows as debug_resize_norm, ``size`` = (H, W),
        mean_std = (mean[3], std[3]) (None: ImageNet), c1_w [12, 2, 2, 3] / c1_b [12] -> fp32 [n, H / 2, W / 2, 12].  ``mirror``:
        swin_crop_front_mirror_kernel (reid_debug_swin_crop_front_mirror), the resized image's columns reversed."""
        h_out, w_out, ms = self._swin_crop_args(size, mean_std)
        if ms is None:
            ms = _f32([0.485, 0.456, 0.406, 0.229, 0.224, 0.225])
        packed = np.ascontiguousarray(packed, np.uint8).reshape(-1)
        offsets = np.ascontiguousarray(offsets, np.int64)
        hw = np.ascontiguousarray(hw, np.int32).reshape(-1, 2)
        n = len(offsets)
        end = max(int(o) + ((int(h) - 1) * (pitch or int(w)) + int(w)) * 3 for o, (h, w) in zip(offsets, hw))
        if len(hw) != n or end > packed.size or int(offsets.min()) < 0 or int(hw.min()) < 1:
            raise ValueError("debug_swin_crop_front: a window leaves the buffer")
        c1_w, c1_b = _f32(c1_w).reshape(-1), _f32(c1_b).reshape(-1)
        if c1_w.size != 144 or c1_b.size != 12:
            raise ValueError("debug_swin_crop_front expects c1_w[12,2,2,3] and c1_b[12]")
        out = np.empty((n, h_out // 2, w_out // 2, 12), np.float32)
        fn = _ffi.debug_lib().reid_debug_swin_crop_front_mirror if mirror else _ffi.debug_lib().reid_debug_swin_crop_front
        check(fn(self.h, _ptr(packed), _ptr(offsets), _ptr(hw), C.c_int(n), C.c_int(int(pitch)), C.c_int(h_out), C.c_int(w_out), _ptr(ms), _ptr(c1_w),
                 _ptr(c1_b), _ptr(out)))
        return out

    def debug_swin_conv1(self, x, c1_w, c1_b, mirror=False):
        """sfe_conv1_kernel alone through its launcher (reid_debug_swin_conv1): x fp32 [n, 3, h, w] -> fp32 [n, h / 2, w / 2, 12].
        ``mirror``: sfe_conv1_mirror_kernel (reid_debug_swin_conv1_mirror), the image read with reversed columns."""
        x, c1_w, c1_b = _f32(x), _f32(c1_w).reshape(-1), _f32(c1_b).reshape(-1)
        n, c, h, w = x.shape
        if c != 3 or h % 2 or w % 2 or c1_w.size != 144 or c1_b.size != 12:
            raise ValueError("debug_swin_conv1 expects x[n,3,2k,2m], c1_w[12,2,2,3] and c1_b[12]")
        out = np.empty((n, h // 2, w // 2, 12), np.float32)
        fn = _ffi.debug_lib().reid_debug_swin_conv1_mirror if mirror else _ffi.debug_lib().reid_debug_swin_conv1
        check(fn(self.h, _ptr(x), C.c_int(n), C.c_int(h), C.c_int(w), _ptr(c1_w), _ptr(c1_b), _ptr(out)))
        return out

    def debug_swin_descriptor(self, e1, e2, cls_w, out_rows=None, ld=None):
        """swin_descriptor_kernel alone through its launcher (reid_debug_swin_descriptor): e1, e2 (None: one view) fp32 [n, 96], cls_w
        [num_class, 96] -> fp32 [out_rows, ld] whose rows [0, n) x columns [0, num_class + 96) hold the descriptors; the rest is NaN."""
        e1, cls_w = _f32(e1), _f32(cls_w)
        e2 = None if e2 is None else _f32(e2)
        if e1.ndim != 2 or e1.shape[1] != 96 or e1.shape[0] < 1 or cls_w.ndim != 2 or cls_w.shape[1] != 96 or cls_w.shape[0] < 1 or \
                (e2 is not None and e2.shape != e1.shape):
            raise ValueError("debug_swin_descriptor expects e1 (and e2) [n,96] and cls_w [num_class,96]")
        n, nc = e1.shape[0], cls_w.shape[0]
        out_rows, ld = n if out_rows is None else int(out_rows), nc + 96 if ld is None else int(ld)
        if out_rows < n or ld < nc + 96:
            raise ValueError("debug_swin_descriptor: out_rows >= n and ld >= num_class + 96")
        out = np.empty((out_rows, ld), np.float32)
        check(_ffi.debug_lib().reid_debug_swin_descriptor(self.h, _ptr(e1), _ptr(e2), _ptr(cls_w), C.c_int(n), C.c_int(nc), C.c_int(out_rows),
                                                          C.c_int(ld), _ptr(out)))
        return out

    def debug_maxpool(self, x):
        """MaxPool(3, 2, 1) through the forward's launcher (reid_debug_maxpool): x [n, h, w, c] fp32, or uint16 f16 bits; same type back."""
        f16 = np.asarray(x).dtype == np.uint16
        x = np.ascontiguousarray(x, np.uint16) if f16 else _f32(x)
        n, h, w, c = x.shape
        out = np.empty((n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c), x.dtype)
        check(_ffi.debug_lib().reid_debug_maxpool(self.h, C.c_int(int(f16)), _ptr(x), C.c_int(n), C.c_int(h), C.c_int(w), C.c_int(c), _ptr(out)))
        return out

    def debug_window_attn_cos(self, mode, qkv, bias, scale, shifted):
        """The Swin v2 cosine window attention alone (libreid_hip_debug.so reid_debug_window_attn_cos).  qkv [n, h, w, 3 * heads * 32]
        fp32, bias [heads, 49, 49] (query, key), scale [heads].  mode 0 -> fp32 [n, h, w, C]; mode 2 -> the [oh | ol'] pair decoded
        to float64 oh + ol' / 2^11; mode 1 (qkv rounded to f16 on the device) -> the f16 result as fp32."""
        qkv, bias, scale = _f32(qkv), _f32(bias), _f32(scale)
        n, h, w, c3 = qkv.shape
        heads = bias.shape[0]
        assert c3 == 3 * heads * 32 and bias.shape == (heads, 49, 49) and scale.shape == (heads,)
        c = heads * 32
        out = np.empty((n, h, w, c), np.float32) if mode == 0 else None
        o16 = None if mode == 0 else np.empty((n * h * w, 2 * c if mode == 2 else c), np.uint16)
        check(_ffi.debug_lib().reid_debug_window_attn_cos(
            self.h, C.c_int(mode), _ptr(qkv), C.c_int(n), C.c_int(h), C.c_int(w), C.c_int(heads), C.c_int(int(bool(shifted))), _ptr(bias),
            _ptr(scale), _ptr(out), _ptr(o16)))
        if mode == 0:
            return out
        f = o16.view(np.float16)
        if mode == 2:
            return (f[:, :c].astype(np.float64) + f[:, c:].astype(np.float64) / 2048.0).reshape(n, h, w, c)
        return f.astype(np.float32).reshape(n, h, w, c)

    def debug_post_norm(self, side, x, y, g, b, in_place=False):
        """The Swin v2 post-norm alone (reid_debug_post_norm): out = x + (LayerNorm(y) g + b), x / y [t, c].  Returns (out fp32 [t, c],
        side output or None: side 1 -> the f16 copy as fp32, side 2 -> the [oh | ol'] pair decoded to float64)."""
        x, y = _f32(x), _f32(y)
        t, c = x.shape
        out = np.empty((t, c), np.float32)
        o16 = None if side == 0 else np.empty((t, 2 * c if side == 2 else c), np.uint16)
        check(_ffi.debug_lib().reid_debug_post_norm(
            self.h, C.c_int(side), _ptr(x), _ptr(y), C.c_int(t), C.c_int(c), _ptr(_f32(g)), _ptr(_f32(b)), C.c_int(int(bool(in_place))),
            _ptr(out), _ptr(o16)))
        if side == 0:
            return out, None
        f = o16.view(np.float16)
        return out, (f[:, :c].astype(np.float64) + f[:, c:].astype(np.float64) / 2048.0) if side == 2 else f.astype(np.float32)

    @staticmethod
    def _unpack16(o16, c):
        """[yh | yl'] uint16 f16 bits [t, 2c] -> float64 yh + yl' / 2^11."""
        f = o16.view(np.float16)
        return f[:, :c].astype(np.float64) + f[:, c:].astype(np.float64) / 2048.0

    def debug_window_attn(self, form, qkv, pos, shifted, raw=False):
        """One Swin v1 window-attention kernel through launch_window_attn (libreid_hip_debug.so reid_debug_window_attn; forms in
        include/reid_hip_debug.h).  qkv [n, h, w, 3 * heads * 32] fp32, pos [13, 13].  Returns [n, h, w, C]: fp32 (forms 0, 5), the
        [oh | ol'] pair decoded to float64 (1, 4), the f16 result as fp32 (2, 3); raw=True: the fp32 / uint16 array as the launch left it."""
        qkv, pos = _f32(qkv), _f32(pos).reshape(-1)
        n, h, w, c3 = qkv.shape
        c = c3 // 3
        if c3 != 3 * c or c % 32 or pos.size != 169:
            raise ValueError("debug_window_attn expects qkv[n, h, w, 3 * heads * 32] and pos[13, 13]")
        out = np.empty((n, h, w, c), np.float32) if form in (0, 5) else None
        o16 = None if form in (0, 5) else np.empty((n * h * w, 2 * c if form in (1, 4) else c), np.uint16)
        check(_ffi.debug_lib().reid_debug_window_attn(
            self.h, C.c_int(form), _ptr(qkv), C.c_int(n), C.c_int(h), C.c_int(w), C.c_int(c // 32), C.c_int(int(bool(shifted))), _ptr(pos),
            _ptr(out), _ptr(o16)))
        if raw:
            return out if o16 is None else o16
        if o16 is None:
            return out
        if form in (1, 4):
            return self._unpack16(o16, c).reshape(n, h, w, c)
        return o16.view(np.float16).astype(np.float32).reshape(n, h, w, c)

    def debug_layernorm(self, form, x, g, b):
        """The Swin LayerNorm (eps 1e-5) through the forward's launchers (reid_debug_layernorm): x [t, c].  form 0 -> fp32 [t, c]; 1 -> uint16
        f16 bits [t, c]; 2 -> uint16 [t, 2c] = [yh | yl']."""
        x = _f32(x)
        t, c = x.shape
        out = np.empty((t, c), np.float32) if form == 0 else None
        o16 = None if form == 0 else np.empty((t, 2 * c if form == 2 else c), np.uint16)
        check(_ffi.debug_lib().reid_debug_layernorm(self.h, C.c_int(form), _ptr(x), C.c_int(t), C.c_int(c), _ptr(_f32(g)), _ptr(_f32(b)),
                                                    _ptr(out), _ptr(o16)))
        return out if form == 0 else o16

    def debug_ln_linear(self, x, ln_g, ln_b, w, bias=None):
        """LayerNorm 1 + to_qkv of the fp32-class mode in one kernel (reid_debug_ln_linear): x [t, c], w [n, c] -> fp32 [t, n]."""
        x, w = _f32(x), _f32(w)
        t, c = x.shape
        n = w.shape[0]
        out = np.empty((t, n), np.float32)
        check(_ffi.debug_lib().reid_debug_ln_linear(self.h, _ptr(x), _ptr(_f32(ln_g)), _ptr(_f32(ln_b)), _ptr(w),
                                                    _ptr(_f32(bias) if bias is not None else None), C.c_int(t), C.c_int(c), C.c_int(n), _ptr(out)))
        return out

    def debug_swin_sfe(self, c1, in_g, in_b, bn_s, bn_t, c2_w, c2_b, fc_w, fc_b):
        """ShadowFeatureExtraction after its first convolution (reid_debug_swin_sfe): c1 [n, h1, w1, 12], c2_w [48, 48] in (kh, kw, c) order,
        fc_w [96, 48].  Returns (ab [n, 24], tok [n, h1 / 2, w1 / 2, 96])."""
        c1 = _f32(c1)
        n, h1, w1, _ = c1.shape
        prm = [_f32(a).reshape(-1) for a in (in_g, in_b, bn_s, bn_t, c2_w, c2_b, fc_w, fc_b)]
        if c1.shape[3] != 12 or [a.size for a in prm] != [6, 6, 6, 6, 2304, 48, 4608, 96]:
            raise ValueError("debug_swin_sfe: operand shapes")
        ab, tok = np.empty((n, 24), np.float32), np.empty((n, h1 // 2, w1 // 2, 96), np.float32)
        check(_ffi.debug_lib().reid_debug_swin_sfe(self.h, _ptr(c1), C.c_int(n), C.c_int(h1), C.c_int(w1), *[_ptr(a) for a in prm], _ptr(ab),
                                                   _ptr(tok)))
        return ab, tok

    def debug_swin_tail(self, x, g, b, p, bn_s, bn_t):
        """The Swin tail (reid_debug_swin_tail): x [n, ntok, 96] -> (gem [n, 96], emb [n, 96])."""
        x = _f32(x)
        n, ntok, c = x.shape
        prm = [_f32(a).reshape(-1) for a in (g, b, bn_s, bn_t)]
        if c != 96 or any(a.size != 96 for a in prm):
            raise ValueError("debug_swin_tail expects x[n, ntok, 96] and 96-channel parameters")
        gem, emb = np.empty((n, 96), np.float32), np.empty((n, 96), np.float32)
        check(_ffi.debug_lib().reid_debug_swin_tail(self.h, _ptr(x), C.c_int(n), C.c_int(ntok), _ptr(prm[0]), _ptr(prm[1]), C.c_float(p),
                                                    _ptr(prm[2]), _ptr(prm[3]), _ptr(gem), _ptr(emb)))
        return gem, emb

    def debug_swin_merge(self, stage, x):
        """Patch merging in front of ``stage`` (2 .. 4) on the loaded Swin weights, in this context's precision (reid_debug_swin_merge):
        x [n, h, w, 48 * 2^(stage - 1)] -> fp32 [n, h / 2, w / 2, 96 * 2^(stage - 1)]."""
        x = _f32(x)
        n, h, w, cin = x.shape
        if cin != 48 << (stage - 1):
            raise ValueError("debug_swin_merge: stage %d takes %d channels" % (stage, 48 << (stage - 1)))
        out = np.empty((n, h // 2, w // 2, 2 * cin), np.float32)
        check(_ffi.debug_lib().reid_debug_swin_merge(self.h, C.c_int(stage), _ptr(x), C.c_int(n), C.c_int(h), C.c_int(w), _ptr(out)))
        return out

    def debug_swin_fuse(self, sfe, x1, x2, x3, x4):
        """The top-down fusion on the loaded Swin weights, in this context's precision (reid_debug_swin_fuse).  sfe / x1 [n, h1, w1, 96], x2 ..
        x4 the later stage outputs.  Returns [a0, f3, f2, f1]; with the context in precision 1 the first three are f16 arrays."""
        maps = [_f32(a) for a in (sfe, x1, x2, x3, x4)]
        n, h1, w1, _ = maps[0].shape
        shapes = [(n, h1 >> s, w1 >> s, 96 << s) for s in (0, 0, 1, 2, 3)]
        if [a.shape for a in maps] != shapes:
            raise ValueError("debug_swin_fuse: expected maps of shapes %r" % (shapes,))
        dt = np.uint16 if self.precision == 1 else np.float32
        outs = [np.empty(shapes[4], dt), np.empty(shapes[3], dt), np.empty(shapes[2], dt), np.empty(shapes[1], np.float32)]
        check(_ffi.debug_lib().reid_debug_swin_fuse(self.h, *[_ptr(a) for a in maps], C.c_int(n), C.c_int(h1), C.c_int(w1),
                                                    *[_ptr(a) for a in outs]))
        return [a.view(np.float16) if a.dtype == np.uint16 else a for a in outs]

    def debug_swin_stage(self, stage, n, h=224, w=224):
        """Stage activations of the last Swin pass as NHWC arrays (0 sfe, 1..4 stage outputs, 5 GeM output [n,96])."""
        if stage == 5:
            shape = (n, 96)
        else:
            s = max(stage - 1, 0)
            shape = (n, (h // 4) >> s, (w // 4) >> s, 96 << s)
        out = np.empty(shape, np.float32)
        cnt = C.c_size_t()
        check(self.lib.reid_debug_swin_stage(self.h, int(stage), _ptr(out), out.size, C.byref(cnt)))
        assert cnt.value == out.size, (cnt.value, out.size)
        return out

    # ---- matching
    @staticmethod
    def distmat_precision_value(v):
        """None / "f32" -> 0 (reid_distmat*: today's call and bits), "f16x3" -> 2 (reid_distmat_x3*); ValueError otherwise, "f16"
        included - the fp16-storage mode has no distance matrix -, before any device call."""
        if v is None:
            return 0
        if isinstance(v, str) and v in DISTMAT_PRECISION_NAMES:
            return DISTMAT_PRECISION_NAMES[v]
        raise ValueError("distmat precision must be None / \"f32\" (exact fp32) or \"f16x3\" (fp32-class, libreid_hip_distmat_x3.so), got %r" % (v,))

    def distmat(self, x, y, metric=_ffi.METRIC_L2, precision=None):
        """out[m][n] = metric(x[m][d], y[n][d]).  precision None / "f32": reid_distmat; "f16x3": reid_distmat_x3, the dot product in the
        fp32-class arithmetic (domain |x| < 65504, |y| < 31.98; other bits than the exact entry, no rank promised)."""
        fn = "reid_distmat_x3" if Engine.distmat_precision_value(precision) == 2 else "reid_distmat"
        x, y = _f32(x), _f32(y)
        if x.ndim != 2 or y.ndim != 2 or x.shape[1] != y.shape[1]:
            raise ValueError("distmat expects x[m,d], y[n,d]")
        out = np.empty((x.shape[0], y.shape[0]), np.float32)
        check(getattr(self.lib, fn)(self.h, _ptr(x), x.shape[0], _ptr(y), y.shape[0], x.shape[1], int(metric), _ptr(out)))
        return out

    def distmat_dev(self, d_x, m, d_y, n, d, metric, d_out, precision=None):
        fn = "reid_distmat_x3_dev" if Engine.distmat_precision_value(precision) == 2 else "reid_distmat_dev"
        check(getattr(self.lib, fn)(self.h, C.c_void_p(d_x), int(m), C.c_void_p(d_y), int(n), int(d), int(metric), C.c_void_p(d_out)))

    @staticmethod
    def select_precision_entry(name, precision, k=None):
        """The C entry a selection call reaches: ``name`` for precision None / "f32" (today's call and bits), ``name`` + "_x3" for
        "f16x3" (candidates from the fp32-class arithmetic, the same answer bit for bit; |x| < 65504, |y| < 31.98, k <= 24).  Any
        other precision, or a k outside 1 .. 24 with "f16x3", is a ValueError before the device is touched."""
        if Engine.distmat_precision_value(precision) != 2:
            return name
        if k is not None and not (isinstance(k, (int, np.integer)) and not isinstance(k, bool) and 1 <= k <= SELECT_X3_KMAX):
            raise ValueError("knn with precision \"f16x3\" takes 1 <= k <= %d, got %r" % (SELECT_X3_KMAX, k))
        return name.replace("_dev", "") + "_x3" + ("_dev" if name.endswith("_dev") else "")

    def argmin_rows(self, x, y, metric=_ffi.METRIC_L2, precision=None):
        fn = Engine.select_precision_entry("reid_argmin_rows", precision)
        x, y = _f32(x), _f32(y)
        idx = np.empty(x.shape[0], np.int32)
        val = np.empty(x.shape[0], np.float32)
        check(getattr(self.lib, fn)(self.h, _ptr(x), x.shape[0], _ptr(y), y.shape[0], x.shape[1], int(metric), _ptr(idx), _ptr(val)))
        return idx, val

    def argmin_rows_dev(self, d_x, m, d_y, n, d, metric, d_idx, d_val=None, precision=None):
        fn = Engine.select_precision_entry("reid_argmin_rows_dev", precision)
        check(getattr(self.lib, fn)(self.h, C.c_void_p(d_x), int(m), C.c_void_p(d_y), int(n), int(d), int(metric),
                                    C.c_void_p(d_idx), C.c_void_p(d_val or 0)))

    def knn(self, xq, xb, k, precision=None):
        fn = Engine.select_precision_entry("reid_knn", precision, k)
        xq, xb = _f32(xq), _f32(xb)
        D = np.empty((xq.shape[0], k), np.float32)
        I = np.empty((xq.shape[0], k), np.int32)
        check(getattr(self.lib, fn)(self.h, _ptr(xq), xq.shape[0], _ptr(xb), xb.shape[0], xq.shape[1], int(k), _ptr(D), _ptr(I)))
        return D, I

    def knn_dev(self, d_xq, nq, d_xb, nb, d, k, d_D, d_I, precision=None):
        fn = Engine.select_precision_entry("reid_knn_dev", precision, k)
        check(getattr(self.lib, fn)(self.h, C.c_void_p(d_xq), int(nq), C.c_void_p(d_xb), int(nb), int(d), int(k),
                                    C.c_void_p(d_D), C.c_void_p(d_I)))

    def debug_select_x3(self, d_x, m, d_y, n, d, metric, k, d_D, d_I, force_fallback_every=0):
        """reid_debug_select_x3 on device operands: the launcher of the "f16x3" selection entries with its test hook; returns
        {"proven", "recomputed", "form", "kk"}."""
        stats = (C.c_int32 * 4)()
        fn = _ffi.debug_lib().reid_debug_select_x3
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        check(fn(self.h, C.c_void_p(d_x), int(m), C.c_void_p(d_y), int(n), int(d), int(metric), int(k), C.c_void_p(d_D or 0), C.c_void_p(d_I),
                 int(force_fallback_every), stats))
        return dict(zip(("proven", "recomputed", "form", "kk"), (int(v) for v in stats)))

    def debug_knn_wide(self, enable=1, force=0):
        """reid_debug_knn_wide: enable = 0 sends every search through the fused fp32 kernel; force > 0 sends every row whose index is
        a multiple of it through the exact-row fallback of the large k-NN path."""
        fn = _ffi.debug_lib().reid_debug_knn_wide
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int]
        check(fn(self.h, int(enable), int(force)))

    def debug_knn_wide_eligible(self, nq, nb, d, k):
        """reid_debug_knn_wide_eligible: does reid_knn_dev take the large k-NN path (csrc/knn_wide.hip) at this shape?"""
        fn = _ffi.debug_lib().reid_debug_knn_wide_eligible
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p] + [C.c_int] * 4
        return bool(fn(self.h, int(nq), int(nb), int(d), int(k)))

    def debug_knn_wide_run(self, xq, xb, k, tile_rows=0, stages=True):
        """reid_debug_knn_wide_run: the large k-NN path on host operands.  Returns a dict: D [nq, k], I [nq, k], guard_D / guard_I (the
        guard rows behind them, as uint32 / int32: untouched = all bits set), nflagged, and with ``stages`` (one tile only) mat
        [nq, ceil256(nb)], keys uint64 [nq, 32], flags int32 [nq], sc float32 [4]."""
        xq, xb = _f32(xq), _f32(xb)
        nq, nb, d = xq.shape[0], xb.shape[0], xq.shape[1]
        nbpad = (nb + 255) // 256 * 256
        D = np.empty((nq + 1, k), np.float32)
        I = np.empty((nq + 1, k), np.int32)
        nfl = C.c_int32(-1)
        out = {}
        if stages:
            out = {"mat": np.empty((nq, nbpad), np.float32), "keys": np.empty((nq, 32), np.uint64), "flags": np.empty(nq, np.int32),
                   "sc": np.empty(4, np.float32)}
        fn = _ffi.debug_lib().reid_debug_knn_wide_run
        fn.restype = C.c_int
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p] + [C.c_int] * 4 + [C.c_void_p] * 7
        check(fn(self.h, _ptr(xq), nq, _ptr(xb), nb, d, int(k), int(tile_rows), _ptr(D), _ptr(I),
                 *[_ptr(out[n]) if stages else None for n in ("mat", "keys", "flags", "sc")], C.cast(C.byref(nfl), C.c_void_p)))
        out.update(D=D[:nq], I=I[:nq], guard_D=D[nq].view(np.uint32), guard_I=I[nq], nflagged=int(nfl.value))
        return out

    def descriptor_f32_nchw(self, x, flip_tta=True):
        """float32 [n,3,H,W] (normalised by the caller) -> float32 [n, 512 + num_class] retrieval descriptor; sizes as embed_f32_nchw."""
        x = _f32(x)
        if x.ndim != 4 or x.shape[1] != 3:
            raise ValueError("descriptor_f32_nchw expects [n,3,H,W] (%d x %d, or sides in [%d, %d]), got %s"
                             % (IMG_H, IMG_W, SIZE_MIN, SIZE_MAX, x.shape))
        h, w = check_hw(x.shape[2:])
        de, nc = self.embed_dim, self.num_class
        out = np.empty((x.shape[0], de + nc), np.float32)
        if (h, w) != (IMG_H, IMG_W):
            check(self.lib.reid_descriptor_f32_nchw_hw(self.h, _ptr(x), x.shape[0], h, w, int(bool(flip_tta)), _ptr(out)))
            return out
        check(self.lib.reid_descriptor_f32_nchw(self.h, _ptr(x), x.shape[0], int(bool(flip_tta)), _ptr(out)))
        return out

    def descriptor_dev(self, d_x, n, flip_tta, d_out, size=None):
        if size is not None:
            h, w = check_hw(size)
            check(self.lib.reid_descriptor_f32_nchw_hw_dev(self.h, C.c_void_p(d_x), int(n), h, w, int(bool(flip_tta)), C.c_void_p(d_out)))
            return
        check(self.lib.reid_descriptor_f32_nchw_dev(self.h, C.c_void_p(d_x), int(n), int(bool(flip_tta)), C.c_void_p(d_out)))

    # ---- the kernels of libreid_hip_anysize.so on host operands (libreid_hip_debug.so; tests/test_gpu_anysize.py).  Each returns its
    # outputs WITH the guard pixel the harness keeps behind them (c more floats, NaN unless a kernel wrote out of bounds).
    def debug_swin_linear(self, x, w, bias=None, res=None, precision=0, act=False, out_form=0, ldc=None, alias=False, x_fp32=False):
        """One Linear layer through linear() / linear16() of csrc/swin.hip (reid_debug_swin_linear, include/reid_hip_debug.h): x [m, k],
        w [n, k], bias [n], res [m, n].  out_form 0 fp32, 1 f16 rows (precision 1), 2 the [yh | yl'] pair (precision 2); ``alias``: the
        residual is the output buffer; ``x_fp32``: precision 2 with x left unpacked (the classifier's call).  Returns (form, raw, front, ld):
        the launchers' form code and the WHOLE guarded output as the launch left it - float32 (form 0) or uint16 f16 bits, ``front``
        guard elements and then m + 8 rows of ``ld`` elements (ldc, or 2 n for form 2), bytes nothing wrote still 0xff."""
        x, w = _f32(x), _f32(w)
        (m, k), n = x.shape, w.shape[0]
        ldc = n if ldc is None else int(ldc)
        ld, front = (2 * n if out_form == 2 else ldc), (64 if out_form == 0 else 128)
        raw = np.empty(front + (m + 8) * ld, np.float32 if out_form == 0 else np.uint16)
        b = None if bias is None else _f32(bias)
        r = None if res is None else _f32(res)
        form = C.c_int(0)
        check(_ffi.debug_lib().reid_debug_swin_linear(
            self.h, _ptr(x), _ptr(w), _ptr(b), _ptr(r), C.c_int(m), C.c_int(n), C.c_int(k), C.c_int(int(precision)),
            C.c_int(int(bool(act)) | 2 * int(bool(alias)) | 4 * int(bool(x_fp32))), C.c_int(int(out_form)), C.c_int(ldc),
            _ptr(raw if out_form == 0 else None), _ptr(None if out_form == 0 else raw), C.byref(form)))
        return form.value, raw, front, ld

    def debug_two_linear_form(self, x, w1, b1, w2, b2, res=None, act=False, ln=None, alias=False):
        """The fused pair of linears of csrc/two_linear_f16.hip in one launch (reid_debug_two_linear_form, include/reid_hip_debug.h):
        out = res + w2 . act(w1 . [LN](x) + b1) + b2 with x / res [m, c], w1 [hid, c], w2 [c, hid], in the context's own precision (2, or
        the launcher refuses).  ``ln`` = (gamma, beta): the LN build (x fp32 through the kernel's prologue); ``alias``: the forward's
        aliasing - LN build: one buffer is x, res and out (``res`` must be None); packed build: res is the output rows.  Returns
        (status, raw, front): the call's status WITHOUT raising (0, -1 a refusal, -3 the range guard; the message stays in
        reid_last_error) and the WHOLE guarded output, ``front`` floats and then m + 8 rows of c, bytes nothing wrote still 0xff."""
        x, w1, w2 = _f32(x), _f32(w1), _f32(w2)
        (m, c), hid = x.shape, w1.shape[0]
        if w1.shape != (hid, c) or w2.shape != (c, hid):
            raise ValueError("debug_two_linear_form: operand shapes")
        front = 64
        raw = np.empty(front + (m + 8) * c, np.float32)
        r = None if res is None else _f32(res)
        g, b = (None, None) if ln is None else (_f32(ln[0]), _f32(ln[1]))
        st = _ffi.debug_lib().reid_debug_two_linear_form(
            self.h, _ptr(x), _ptr(w1), _ptr(_f32(b1)), _ptr(w2), _ptr(_f32(b2)), _ptr(r), C.c_int(m), C.c_int(c), C.c_int(hid),
            C.c_int(int(bool(act)) | 2 * int(ln is not None) | 4 * int(bool(alias))), _ptr(g), _ptr(b), _ptr(raw))
        return int(st), raw, front

    def debug_any_ca_tail(self, y, shortcut, prm):
        """The TripletAttention tail of libreid_hip_anysize_ca.so through the any-size forward's launcher (reid_debug_any_ca_tail): y,
        shortcut [n, h, w, c], prm [3, 100].  Returns (out [n h w c + c], maps [n, 2 per], gates [n per + c]) in the layouts of
        include/reid_hip_debug.h, guards included."""
        y, shortcut, prm = _f32(y), _f32(shortcut), _f32(prm)
        n, h, w, c = y.shape
        if shortcut.shape != y.shape or prm.size != 300:
            raise ValueError("debug_any_ca_tail: operand shapes")
        per = h * w + c * w + h * c
        out = np.empty(y.size + c, np.float32)
        maps = np.empty((n, 2 * per), np.float32)
        gates = np.empty(n * per + c, np.float32)
        check(_ffi.debug_lib().reid_debug_any_ca_tail(self.h, n, h, w, c, _ptr(prm), _ptr(y), _ptr(shortcut), _ptr(out), _ptr(maps), _ptr(gates)))
        return out, maps, gates

    def debug_any_ema_tail(self, y, shortcut, prm):
        """The EMA tail of libreid_hip_anysize_ema.so through the any-size forward's launcher (reid_debug_any_ema_tail): y, shortcut
        [n, h, w, c], prm the cg * cg * 10 + 4 * cg floats of Se18Block::ema (cg = c / 32).  Returns (out [n h w c + c], sig [n, h + w, c],
        small [n 4 c + c]) in the layouts of include/reid_hip_debug.h, guards included."""
        y, shortcut, prm = _f32(y), _f32(shortcut), _f32(prm)
        n, h, w, c = y.shape
        cg = c // 32
        if shortcut.shape != y.shape or c % 32 or prm.size != cg * cg * 10 + 4 * cg:
            raise ValueError("debug_any_ema_tail: operand shapes")
        out = np.empty(y.size + c, np.float32)
        sig = np.empty((n, h + w, c), np.float32)
        small = np.empty(n * 4 * c + c, np.float32)
        check(_ffi.debug_lib().reid_debug_any_ema_tail(self.h, n, h, w, c, _ptr(prm), _ptr(y), _ptr(shortcut), _ptr(out), _ptr(sig), _ptr(small)))
        return out, sig, small

    def debug_any_norm(self, x, half, in_gamma, in_beta, bn_scale=None, bn_shift=None):
        x = _f32(x)
        n, hw, c = x.shape
        out = np.empty(x.size + c, np.float32)
        g, b = _f32(in_gamma), _f32(in_beta)
        bs, bh = (None, None) if bn_scale is None else (_f32(bn_scale), _f32(bn_shift))
        check(_ffi.debug_lib().reid_debug_any_norm(self.h, n, hw, c, int(half), _ptr(x), _ptr(g), _ptr(b), _ptr(bs), _ptr(bh), _ptr(out)))
        return out

    def debug_any_se_tail(self, y, shortcut, w1, w2t):
        y, shortcut, w1, w2t = _f32(y), _f32(shortcut), _f32(w1), _f32(w2t)
        n, hw, c = y.shape
        out = np.empty(y.size + c, np.float32)
        gate = np.empty(n * c + c, np.float32)
        check(_ffi.debug_lib().reid_debug_any_se_tail(self.h, n, hw, c, w1.shape[0], _ptr(w1), _ptr(w2t), _ptr(y), _ptr(shortcut), _ptr(out),
                                                      _ptr(gate)))
        return out, gate

    def debug_any_gem(self, x, p, scale, shift):
        x, scale, shift = _f32(x), _f32(scale), _f32(shift)
        n, hw, c = x.shape
        gem = np.empty(n * c + c, np.float32)
        emb = np.empty(n * c + c, np.float32)
        check(_ffi.debug_lib().reid_debug_any_gem(self.h, n, hw, c, C.c_float(p), _ptr(x), _ptr(scale), _ptr(shift), _ptr(gem), _ptr(emb)))
        return gem, emb

    def debug_descriptor(self, e1, l1, e2=None, l2=None):
        """descriptor_kernel through the launcher the descriptor entries call (reid_debug_descriptor): e1 / e2 [n, de], l1 / l2 [n, dl], the
        second view both or neither.  Returns (out [n, de + dl], guard [de + dl] - the row behind the output, NaN unless the kernel
        wrote out of bounds)."""
        e1, l1 = _f32(e1), _f32(l1)
        (n, de), dl = e1.shape, l1.shape[1]
        if l1.shape[0] != n or (e2 is None) != (l2 is None):
            raise ValueError("debug_descriptor: e1 [n, de], l1 [n, dl] and both or neither of e2, l2")
        e2, l2 = (None, None) if e2 is None else (_f32(e2), _f32(l2))
        if e2 is not None and (e2.shape != e1.shape or l2.shape != l1.shape):
            raise ValueError("debug_descriptor: the second view must have the first one's shapes")
        d = de + dl
        out = np.empty((n + 1) * d, np.float32)
        check(_ffi.debug_lib().reid_debug_descriptor(self.h, _ptr(e1), _ptr(l1), _ptr(e2), _ptr(l2), n, de, dl, _ptr(out)))
        return out[:-d].reshape(n, d), out[-d:]

    def debug_flip_w(self, x):
        """flip_w_nchw_kernel through the launcher the 256 x 128 descriptor entries call (reid_debug_flip_w): x [rows, w].  Returns
        (y [rows, w], guard [w])."""
        x = _f32(x)
        rows, w = x.shape
        y = np.empty((rows + 1) * w, np.float32)
        check(_ffi.debug_lib().reid_debug_flip_w(self.h, _ptr(x), C.c_longlong(rows), w, _ptr(y)))
        return y[:-w].reshape(rows, w), y[-w:]

    def debug_any_conv(self, x, wt, stride, hw_precision=2, scale=None, shift=None, res=None, relu=False, relu_from=0):
        """One trunk convolution of the any-size forward (reid_debug_any_conv): x [n, h, w, cin], wt [cout, r, r, cin] with r = 3 (pad 1) or
        1 (pad 0).  Returns (out [n, ho, wo, cout], guard [cout] - the row behind the last pixel, NaN unless the kernel wrote out of
        bounds -, the tile form launched: 0 for exact fp32)."""
        x, wt = _f32(x), _f32(wt)
        n, h, w, cin = x.shape
        cout, r = wt.shape[0], wt.shape[1]
        pad = 1 if r == 3 else 0
        ho, wo = (h + 2 * pad - r) // stride + 1, (w + 2 * pad - r) // stride + 1
        sc, sh = (None, None) if scale is None else (_f32(scale), _f32(shift))
        rr = None if res is None else _f32(res)
        if rr is not None and rr.size != n * ho * wo * cout:
            raise ValueError("debug_any_conv: the residual must have the output's %d elements" % (n * ho * wo * cout))
        out = np.empty(n * ho * wo * cout + cout, np.float32)
        form = C.c_int(0)
        check(_ffi.debug_lib().reid_debug_any_conv(self.h, int(hw_precision), _ptr(x), n, h, w, cin, _ptr(wt), cout, r, int(stride), pad, _ptr(sc),
                                                   _ptr(sh), _ptr(rr), int(bool(relu)), int(relu_from), _ptr(out), C.byref(form)))
        return out[:-cout].reshape(n, ho, wo, cout), out[-cout:], form.value

    # ---- libreid_hip_anysize_f16.so (reid_debug_any_*_f16): f16 operands are np.float16 arrays, handed over as their bits
    def debug_any_conv_f16(self, x, wt, stride, scale=None, shift=None, res=None, relu=False, relu_from=0):
        """One trunk convolution of the fp16-storage any-size forward: x float16 [n, h, w, cin], wt float16 [cout, r, r, cin], r = 3 (pad 1)
        or 1 (pad 0).  Returns (out float16 [n, ho, wo, cout], guard [cout] - NaN unless the kernel wrote out of bounds -, the tile form)."""
        x, wt = _f16(x), _f16(wt)
        n, h, w, cin = x.shape
        cout, r = wt.shape[0], wt.shape[1]
        pad = 1 if r == 3 else 0
        ho, wo = (h + 2 * pad - r) // stride + 1, (w + 2 * pad - r) // stride + 1
        sc, sh = (None, None) if scale is None else (_f32(scale), _f32(shift))
        rr = None if res is None else _f16(res)
        if rr is not None and rr.size != n * ho * wo * cout:
            raise ValueError("debug_any_conv_f16: the residual must have the output's %d elements" % (n * ho * wo * cout))
        out = np.empty(n * ho * wo * cout + cout, np.float16)
        form = C.c_int(0)
        check(_ffi.debug_lib().reid_debug_any_conv_f16(self.h, _ptr(x), n, h, w, cin, _ptr(wt), cout, r, int(stride), pad, _ptr(sc), _ptr(sh),
                                                       _ptr(rr), int(bool(relu)), int(relu_from), _ptr(out), C.byref(form)))
        return out[:-cout].reshape(n, ho, wo, cout), out[-cout:], form.value

    def debug_any_stem_f16(self, x, w16, scale, shift):
        """Stem + max-pool of that forward: x fp32 [n, h, w, 3], w16 float16 [64, 192].  Returns (stem float16 [n, H1, W1, 64], its guard
        [64], pool float16 [n, H2, W2, 64], its guard [64])."""
        x, w16, scale, shift = _f32(x), _f16(w16), _f32(scale), _f32(shift)
        n, h, w, _ = x.shape
        if w16.size != 64 * 192 or scale.size != 64 or shift.size != 64 or x.shape[3] != 3:
            raise ValueError("debug_any_stem_f16: x [n, h, w, 3], w16 [64, 192], scale [64], shift [64]")
        h1, w1 = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        h2, w2 = (h1 - 1) // 2 + 1, (w1 - 1) // 2 + 1
        stem = np.empty(n * h1 * w1 * 64 + 64, np.float16)
        pool = np.empty(n * h2 * w2 * 64 + 64, np.float16)
        check(_ffi.debug_lib().reid_debug_any_stem_f16(self.h, _ptr(x), n, h, w, _ptr(w16), _ptr(scale), _ptr(shift), _ptr(stem), _ptr(pool)))
        return stem[:-64].reshape(n, h1, w1, 64), stem[-64:], pool[:-64].reshape(n, h2, w2, 64), pool[-64:]

    def debug_any_norm_f16(self, x, half, in_gamma, in_beta):
        x = _f16(x)
        n, hw, c = x.shape
        out = np.empty(x.size + c, np.float16)
        g, b = _f32(in_gamma), _f32(in_beta)
        check(_ffi.debug_lib().reid_debug_any_norm_f16(self.h, n, hw, c, int(half), _ptr(x), _ptr(g), _ptr(b), _ptr(out)))
        return out

    def debug_any_se_tail_f16(self, y, shortcut, w1, w2t, alias=False):
        y, shortcut, w1, w2t = _f16(y), _f16(shortcut), _f32(w1), _f32(w2t)
        n, hw, c = y.shape
        out = np.empty(y.size + c, np.float16)
        gate = np.empty(n * c + c, np.float32)
        check(_ffi.debug_lib().reid_debug_any_se_tail_f16(self.h, n, hw, c, w1.shape[0], _ptr(w1), _ptr(w2t), _ptr(y), _ptr(shortcut),
                                                          int(bool(alias)), _ptr(out), _ptr(gate)))
        return out, gate

    def debug_any_ca_tail_f16(self, y, shortcut, prm, out=None):
        """The TripletAttention tail of libreid_hip_anysize_sib_f16.so through the any-size forward's launcher
        (reid_debug_any_ca_tail_f16): y, shortcut float16 [n, h, w, c], prm [3, 100].  Returns (out float16 [n h w c + c], maps [n, 2 per],
        gates [n per + c]) as debug_any_ca_tail does, guards included.  ``out``: a float16 buffer of that size to write into."""
        y, shortcut, prm = _f16(y), _f16(shortcut), _f32(prm)
        n, h, w, c = y.shape
        if shortcut.shape != y.shape or prm.size != 300 or (out is not None and (out.dtype != np.float16 or out.size != y.size + c)):
            raise ValueError("debug_any_ca_tail_f16: operand shapes")
        per = h * w + c * w + h * c
        out = np.empty(y.size + c, np.float16) if out is None else out
        maps = np.empty((n, 2 * per), np.float32)
        gates = np.empty(n * per + c, np.float32)
        check(_ffi.debug_lib().reid_debug_any_ca_tail_f16(self.h, n, h, w, c, _ptr(prm), _ptr(y), _ptr(shortcut), _ptr(out), _ptr(maps),
                                                          _ptr(gates)))
        return out, maps, gates

    def debug_any_ema_tail_f16(self, y, shortcut, prm, out=None):
        """The EMA tail of libreid_hip_anysize_sib_f16.so through the any-size forward's launcher (reid_debug_any_ema_tail_f16): y,
        shortcut float16 [n, h, w, c], prm as debug_any_ema_tail takes it.  Returns (out float16 [n h w c + c], sig [n, h + w, c], small
        [n 4 c + c]) as debug_any_ema_tail does, guards included.  ``out``: a float16 buffer of that size to write into."""
        y, shortcut, prm = _f16(y), _f16(shortcut), _f32(prm)
        n, h, w, c = y.shape
        cg = c // 32
        if shortcut.shape != y.shape or c % 32 or prm.size != cg * cg * 10 + 4 * cg or \
                (out is not None and (out.dtype != np.float16 or out.size != y.size + c)):
            raise ValueError("debug_any_ema_tail_f16: operand shapes")
        out = np.empty(y.size + c, np.float16) if out is None else out
        sig = np.empty((n, h + w, c), np.float32)
        small = np.empty(n * 4 * c + c, np.float32)
        check(_ffi.debug_lib().reid_debug_any_ema_tail_f16(self.h, n, h, w, c, _ptr(prm), _ptr(y), _ptr(shortcut), _ptr(out), _ptr(sig),
                                                           _ptr(small)))
        return out, sig, small

    def debug_any_gem_f16(self, x, p, scale, shift):
        x, scale, shift = _f16(x), _f32(scale), _f32(shift)
        n, hw, c = x.shape
        gem = np.empty(n * c + c, np.float32)
        emb = np.empty(n * c + c, np.float32)
        check(_ffi.debug_lib().reid_debug_any_gem_f16(self.h, n, hw, c, C.c_float(p), _ptr(x), _ptr(scale), _ptr(shift), _ptr(gem), _ptr(emb)))
        return gem, emb

    def debug_any_front(self, crops, size, stem_w, scale, shift, mean_std=None, fused=True, frame=None):
        """The front end of the any-size forward from uint8 windows (reid_debug_any_front): resize to ``size`` = (H, W) + normalise +
        stem (stem_w [64, 192], scale / shift [64]) + max-pool, ``fused`` = any_front_kernel, else the three launches.  ``crops``: a list of
        uint8[h_i, w_i, 3], or with ``frame`` = uint8[fh, fw, 3] int boxes [n, 4] (x1, y1, x2, y2) of windows of that frame.  Returns
        (pool [n, H2, W2, 64], guard [W2 * 64] - the pixel row behind the output, NaN unless the kernel wrote out of bounds)."""
        h, w, ms = self._hw_crop_args(size, mean_std)
        stem_w, scale, shift = _f32(stem_w), _f32(scale), _f32(shift)
        if stem_w.size != 64 * 192 or scale.size != 64 or shift.size != 64:
            raise ValueError("debug_any_front: stem_w [64, 192], scale [64], shift [64]")
        if frame is None:
            src, offs, hw, _keep = self._pack_ragged(crops)
            n, pitch, nbytes = len(crops), 0, int(sum(int(a) * int(b) * 3 for a, b in hw))
        else:
            frame = np.ascontiguousarray(frame, dtype=np.uint8)
            boxes = np.asarray(crops, np.int64).reshape(-1, 4)
            fh, fw = frame.shape[:2]
            if frame.ndim != 3 or frame.shape[2] != 3 or not ((boxes[:, 0] >= 0) & (boxes[:, 1] >= 0) & (boxes[:, 2] <= fw) & (boxes[:, 3] <= fh) &
                                                             (boxes[:, 2] > boxes[:, 0]) & (boxes[:, 3] > boxes[:, 1])).all():
                raise ValueError("debug_any_front: frame uint8[fh, fw, 3] and non-empty boxes inside it")
            n, pitch, nbytes = boxes.shape[0], fw, frame.size
            offs = np.ascontiguousarray((boxes[:, 1] * fw + boxes[:, 0]) * 3, np.int64)
            hw = np.ascontiguousarray(np.stack([boxes[:, 3] - boxes[:, 1], boxes[:, 2] - boxes[:, 0]], 1), np.int32)
            src = _ptr(frame)
        if n < 1:
            raise ValueError("debug_any_front: at least one window")
        h2, w2 = stage_shapes(h, w)[1][:2]
        out = np.empty(n * h2 * w2 * 64 + w2 * 64, np.float32)
        check(_ffi.debug_lib().reid_debug_any_front(self.h, int(bool(fused)), src, C.c_int64(nbytes), _ptr(offs), _ptr(hw), n, pitch, h, w, _ptr(ms),
                                                    _ptr(stem_w), _ptr(scale), _ptr(shift), _ptr(out)))
        return out[:-w2 * 64].reshape(n, h2, w2, 64), out[-w2 * 64:]

    def cam_debias_dev(self, d_x, cams, n, d, la=0.05, iters=0):
        cams = np.ascontiguousarray(cams, dtype=np.int32).reshape(-1)
        if cams.shape[0] != n:
            raise ValueError("cam_debias_dev: %d camera ids for %d rows" % (cams.shape[0], n))
        check(self.lib.reid_cam_debias_dev(self.h, C.c_void_p(d_x), _ptr(cams), int(n), int(d), C.c_float(la), int(iters)))

    def smooth_tracklets_dev(self, d_x, seqs, valid, n, d, keep=0.1):
        seqs = np.ascontiguousarray(seqs, dtype=np.int32).reshape(-1)
        v = None if valid is None else np.ascontiguousarray(np.asarray(valid).reshape(-1) != 0, dtype=np.uint8)
        if seqs.shape[0] != n or (v is not None and v.shape[0] != n):
            raise ValueError("smooth_tracklets_dev: seqs / valid must have %d entries" % n)
        check(self.lib.reid_smooth_tracklets_dev(self.h, C.c_void_p(d_x), _ptr(seqs), _ptr(v), int(n), int(d), C.c_float(keep)))

    def rank_eval_dev(self, d_qf, ql, qc, nq, d_gf, gl, gc, ng, d):
        """Features in HBM, labels / cameras host int64 arrays -> (cmc_sum int32[ng], ap float64[nq], valid int32[nq])."""
        ql, qc, gl, gc = (np.ascontiguousarray(a, dtype=np.int64) for a in (ql, qc, gl, gc))
        cmc = np.empty(ng, np.int32)
        ap = np.empty(nq, np.float64)
        valid = np.empty(nq, np.int32)
        check(self.lib.reid_rank_eval_dev(self.h, C.c_void_p(d_qf), _ptr(ql), _ptr(qc), int(nq), C.c_void_p(d_gf), _ptr(gl),
                                          _ptr(gc), int(ng), int(d), _ptr(cmc), _ptr(ap), _ptr(valid)))
        return cmc, ap, valid

    def cam_debias(self, x, cams, la=0.05, iters=0):
        """diminish_camera_bias (reid/inference_utils.py:5-15) on the device; returns a new float32 [n, d] array."""
        x = np.array(_f32(x), copy=True)
        cams = np.ascontiguousarray(cams, dtype=np.int32).reshape(-1)
        if x.ndim != 2 or cams.shape[0] != x.shape[0]:
            raise ValueError("cam_debias expects x[n,d] and cams[n]")
        check(self.lib.reid_cam_debias(self.h, _ptr(x), _ptr(cams), x.shape[0], x.shape[1], C.c_float(la), int(iters)))
        return x

    def smooth_tracklets(self, x, seqs, valid=None, keep=0.1):
        """smooth_tracklets (reid/inference_utils.py:18-27) on the device; returns a new float32 [n, d] array."""
        x = np.array(_f32(x), copy=True)
        seqs = np.ascontiguousarray(seqs, dtype=np.int32).reshape(-1)
        if x.ndim != 2 or seqs.shape[0] != x.shape[0]:
            raise ValueError("smooth_tracklets expects x[n,d] and seqs[n]")
        v = None if valid is None else np.ascontiguousarray(np.asarray(valid).reshape(-1) != 0, dtype=np.uint8)
        check(self.lib.reid_smooth_tracklets(self.h, _ptr(x), _ptr(seqs), _ptr(v), x.shape[0], x.shape[1], C.c_float(keep)))
        return x

    def rerank_jaccard(self, x, k1=20, k2=6, rank=None):
        """float32 [n, n] k-reciprocal Jaccard distance (reid/faiss_utils.py:147-244); rank: optional int32 [n, k1]."""
        x = _f32(x)
        n, d = x.shape
        out = np.empty((n, n), np.float32)
        if rank is not None:
            rank = np.ascontiguousarray(rank, dtype=np.int32)
            if rank.shape != (n, int(k1)):
                raise ValueError(f"rank must be [{n}, {k1}], got {rank.shape}")
        check(self.lib.reid_rerank_jaccard(self.h, _ptr(x), n, d, int(k1), int(k2), _ptr(rank) if rank is not None else None,
                                           _ptr(out)))
        return out

    def rerank_jaccard_dev(self, d_x, n, d, k1, k2, d_out, d_rank=None):
        check(self.lib.reid_rerank_jaccard_dev(self.h, C.c_void_p(d_x), int(n), int(d), int(k1), int(k2),
                                               C.c_void_p(d_rank or 0), C.c_void_p(d_out)))

    def diou(self, bbox, candidates):
        b = np.ascontiguousarray(bbox, dtype=np.float64).reshape(4)
        c = np.ascontiguousarray(candidates, dtype=np.float64).reshape(-1, 4)
        out = np.empty(c.shape[0], np.float64)
        check(self.lib.reid_diou(self.h, _ptr(b), _ptr(c), c.shape[0], _ptr(out)))
        return out

    def diou_cost(self, tracks, dets):
        t = np.ascontiguousarray(tracks, dtype=np.float64).reshape(-1, 4)
        d = np.ascontiguousarray(dets, dtype=np.float64).reshape(-1, 4)
        out = np.empty((t.shape[0], d.shape[0]), np.float64)
        check(self.lib.reid_diou_cost(self.h, _ptr(t), t.shape[0], _ptr(d), d.shape[0], _ptr(out)))
        return out

    def rank_eval(self, qf, ql, qc, gf, gl, gc):
        qf, gf = _f32(qf), _f32(gf)
        ql, qc, gl, gc = (np.ascontiguousarray(a, dtype=np.int64) for a in (ql, qc, gl, gc))
        nq, ng = qf.shape[0], gf.shape[0]
        cmc = np.empty(ng, np.int32)
        ap = np.empty(nq, np.float64)
        valid = np.empty(nq, np.int32)
        check(self.lib.reid_rank_eval(self.h, _ptr(qf), _ptr(ql), _ptr(qc), nq, _ptr(gf), _ptr(gl), _ptr(gc), ng,
                                      qf.shape[1], _ptr(cmc), _ptr(ap), _ptr(valid)))
        return cmc, ap, valid

    # ---- single operators
    def conv2d_nhwc(self, x, w, stride=1, pad=0, scale=None, shift=None, residual=None, relu=False):
        x, w = _f32(x), _f32(w)
        n, h, ww, cin = x.shape
        cout, r, s, _ = w.shape
        ho, wo = (h + 2 * pad - r) // stride + 1, (ww + 2 * pad - s) // stride + 1
        out = np.empty((n, ho, wo, cout), np.float32)
        sc = _f32(scale) if scale is not None else None
        sh = _f32(shift) if shift is not None else None
        res = _f32(residual) if residual is not None else None
        check(self.lib.reid_conv2d_nhwc(self.h, _ptr(x), n, h, ww, cin, _ptr(w), cout, r, s, stride, pad, _ptr(sc), _ptr(sh),
                                        _ptr(res), int(bool(relu)), _ptr(out)))
        return out

    def gemm_nt(self, a, b, bias=None):
        a, b = _f32(a), _f32(b)
        out = np.empty((a.shape[0], b.shape[0]), np.float32)
        bi = _f32(bias) if bias is not None else None
        check(self.lib.reid_gemm_nt(self.h, _ptr(a), a.shape[0], _ptr(b), b.shape[0], a.shape[1], _ptr(bi), _ptr(out)))
        return out


def get_engine(device=0):
    """Process-wide engine per device (one context per (process, device))."""
    device = int(device)
    if device not in _ENGINES:
        _ENGINES[device] = Engine(device)
    return _ENGINES[device]
