"""What every Python entry point does with the five any-size settings (hw_precision, hw_siblings, hw_ema, hw_f16, hw_sib_f16), enumerated
on a stand-in engine (no GPU): which combinations of architecture, keywords and size raise what, and which setter calls - restores
included - the accepted ones make before the first real device call.

`cases()` yields (id, record) in a fixed order; a record is [kind, message, calls]: kind the exception's type name, "_Stop" (the stand-in
was asked for device work) or "returned"; message the full text of a ValueError ("" otherwise); calls the (name, value) pairs of every
set_hw_* / set_precision call - and of every get_engine(device) - in order.  tests/golden/hw_settings_trace.json holds these records as
the parent commit of the settings refactor produced them (`python tests/hw_settings_cases.py OUT.json PARENT_HASH`);
tests/test_hw_settings_host.py compares.

The cross product per entry point: every arch / model name it accepts plus one it refuses; hw_precision absent, "f32", "f16x3", "bogus"
(Extractor has no such keyword: its `precision` is what names the arithmetic of another size, and takes these values); each 0/1 keyword
it takes absent, True, 2; where it takes a size, none, a good one and a bad one.  The stream classes run on a shared context, fresh or
with both fp16 settings left on by an earlier user.  Checkpoints are made once per architecture and packed once (a cache around
synth / weights: nothing the rules read)."""
import contextlib
import hashlib
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from reid_amd import backbone, extractor, inference_utils, models, reid_inference, synth, tracking, weights  # noqa: E402
from reid_amd import engine as engine_mod  # noqa: E402
from reid_amd.engine import Engine  # noqa: E402

SETTINGS = ("hw_precision", "hw_siblings", "hw_ema", "hw_f16", "hw_sib_f16")
ABSENT = "absent"
PRECISIONS = (ABSENT, "f32", "f16x3", "bogus")
FLAGS = (ABSENT, True, 2)
ENTRY_POINTS = ("factory", "build_model", "Extractor", "inference_efficient", "evaluate_reid", "extract_descriptors", "CameraStream",
                "MultiCameraStream", "LookaheadCameraStream")
# keyword -> what its bad value's ValueError must name; per entry point, the keywords it takes
KEYWORDS = {"factory": SETTINGS, "build_model": SETTINGS, "Extractor": ("precision",) + SETTINGS[1:],
            "inference_efficient": ("hw_precision", "hw_ema", "hw_f16", "hw_sib_f16"),
            "evaluate_reid": ("hw_precision", "hw_ema", "hw_f16", "hw_sib_f16"), "extract_descriptors": ("hw_precision", "hw_f16", "hw_sib_f16"),
            "CameraStream": ("hw_precision", "hw_ema", "hw_f16", "hw_sib_f16"), "MultiCameraStream": ("hw_precision", "hw_ema", "hw_f16", "hw_sib_f16"),
            "LookaheadCameraStream": ("hw_precision", "hw_ema", "hw_f16", "hw_sib_f16")}


class _Stop(Exception):
    """The stand-in was asked for device work."""


def _plain(v):
    return bool(v) if isinstance(v, (bool, np.bool_)) else int(v) if isinstance(v, np.integer) else v


class StandIn:
    """Stands where an Engine would: answers what the argument checks read and what lies between them and the scopes (weights "load",
    device memory is a number), records every set_hw_* / set_precision call and keeps the matching attribute, and raises _Stop at any
    other device call.  The scopes are the Engine's own, run on this object."""
    embed_dim, num_class, swin_dim, swin_num_class = 512, 751, 96, 751
    _owner = _swin_owner = None

    def __init__(self, left_on=False):
        self.calls = []
        self.precision, self.hw_precision, self.hw_siblings, self.hw_ema = 0, -1, False, False
        self.hw_f16 = self.hw_sib_f16 = bool(left_on)

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        raise _Stop(name)

    def handed_out(self, device):
        """What get_engine does in the stand-in's world: on record too, so that an argument check that moves behind it shows."""
        self.calls.append(["get_engine", device])
        return self

    def set_precision(self, mode):
        self.calls.append(["set_precision", _plain(mode)])
        self.precision = int(mode)

    def fault_bits(self):
        return 0

    def precision_ok(self, arch, mode):
        return True

    def load_seres18(self, blob, manifest):
        self._owner = None

    def load_swin(self, blob, manifest):
        self._swin_owner = None

    def malloc(self, nbytes):
        return 4096

    def free(self, dptr):
        pass

    def sync(self):
        pass


def _recording_setter(name):
    value = getattr(Engine, name + "_value")

    def setter(self, v):
        n = value(v)                                       # a bad value raises as the Engine's setter does, before anything is recorded
        self.calls.append(["set_" + name, _plain(v)])
        setattr(self, name, n if name == "hw_precision" else bool(n))
    return setter


for _name in SETTINGS:
    setattr(StandIn, _name + "_value", staticmethod(getattr(Engine, _name + "_value")))
    setattr(StandIn, "set_" + _name, _recording_setter(_name))
    setattr(StandIn, _name + "_scope", getattr(Engine, _name + "_scope"))
if hasattr(Engine, "hw_scope"):
    StandIn.hw_scope = Engine.hw_scope


def _cached(fn):
    memo = {}

    def cached(*a, **k):
        key = (tuple(id(v) if isinstance(v, dict) else v for v in a), tuple(sorted(k.items())))
        if key not in memo:
            memo[key] = (a, fn(*a, **k))                   # `a` is kept so that an id stays the dict's
        return memo[key][1]
    return cached


@contextlib.contextmanager
def _stand_in_world(current):
    """get_engine of every module hands out current[0] (and records it); checkpoints and their packed forms are made once; $REID_PRECISION
    is unset."""
    saved = [(m, "get_engine", m.get_engine) for m in (engine_mod, backbone, inference_utils, reid_inference, tracking)]
    saved += [(synth, "seres18_state_dict", synth.seres18_state_dict), (synth, "swin_state_dict", synth.swin_state_dict),
              (extractor, "pack_checkpoint", extractor.pack_checkpoint), (weights, "normalize_state_dict", weights.normalize_state_dict),
              (weights, "pack_seres18", weights.pack_seres18), (weights, "pack_swin", weights.pack_swin)]
    env = os.environ.pop("REID_PRECISION", None)
    try:
        for m, name, fn in saved:
            setattr(m, name, (lambda device=0: current[0].handed_out(device)) if name == "get_engine" else _cached(fn))
        yield
    finally:
        for m, name, fn in saved:
            setattr(m, name, fn)
        if env is not None:
            os.environ["REID_PRECISION"] = env


def _kw_product(names, precision_key="hw_precision"):
    """Every combination of the keywords `names` as a dict (absent ones left out), hw_precision - or Extractor's precision - first."""
    for values in itertools.product(*[PRECISIONS if n == precision_key else FLAGS for n in names]):
        yield {n: v for n, v in zip(names, values) if v is not ABSENT}


def _id(*parts):
    def show(p):
        if isinstance(p, dict):
            return ",".join("%s=%s" % (k, v) for k, v in p.items()) or "-"
        return str(p).replace(" ", "")
    return "/".join(show(p) for p in parts)


def _record(current, call, left_on=False):
    current[0] = eng = StandIn(left_on)
    try:
        call(eng)
        kind, msg = "returned", ""
    except _Stop:
        kind, msg = "_Stop", ""
    except ValueError as e:
        kind, msg = "ValueError", str(e)
    except Exception as e:                                 # noqa: BLE001 - the type is the record
        kind, msg = type(e).__name__, ""
    return [kind, msg, eng.calls]


def _model_cases(current):
    inputs = {"seres18_ibn": ((64, 32), (256, 128), (31, 32)), "swin_transformer": ((224, 224), (31, 32))}
    factories = {"seres18_ibn": backbone.seres18_ibn, "cares18_ibn": backbone.cares18_ibn, "emares18_ibn": backbone.emares18_ibn,
                 "swin_transformer": backbone.swin_t}
    for entry in ("factory", "build_model"):
        for name in tuple(factories) + (("resnet50",) if entry == "build_model" else ()):
            for kw in _kw_product(SETTINGS):
                for hw in inputs.get(name, inputs["seres18_ibn"]):
                    def call(eng, name=name, kw=kw, hw=hw, entry=entry):
                        if entry == "factory":
                            model = factories[name](num_classes=5, **kw)
                        else:
                            model = models.build_model(name, 5, loss="triplet", pretrained=False, **kw)
                        model(np.zeros((1, 3) + hw, np.float32))
                    yield _id(entry, name, kw, hw), _record(current, call)


def _extractor_cases(current):
    sds = {"seres18_ibn": synth.seres18_state_dict(0, num_class=5), "cares18_ibn": synth.cares18_state_dict(0, num_class=5),
           "emares18_ibn": synth.emares18_state_dict(0, num_class=5), "swin": synth.swin_state_dict(0, num_class=5), "not_a_checkpoint": {}}
    crop = [np.zeros((9, 7, 3), np.uint8)]
    for name, sd in sds.items():
        for kw in _kw_product(KEYWORDS["Extractor"], "precision"):
            for size in (None, (64, 128), (31, 128)):
                def call(eng, sd=sd, kw=kw, size=size):
                    extractor.Extractor(sd, **dict(kw, **({} if size is None else {"size": size})))(crop)
                yield _id("Extractor", name, kw, size), _record(current, call)


EVAL_ARCHS = ("seres18", "swin", "seres18_hw", "cares18_hw", "emares18_hw", "resnet50")


def _eval_cases(current):
    crops, lab = [np.zeros((9, 7, 3), np.uint8)], np.zeros(1, np.int64)
    for entry in ("inference_efficient", "evaluate_reid"):
        for arch in EVAL_ARCHS:
            for kw in _kw_product(KEYWORDS[entry]):
                for size in (None, (96, 72), (31, 72)):
                    def call(eng, entry=entry, arch=arch, kw=kw, size=size):
                        if entry == "inference_efficient":
                            reid_inference.inference_efficient(eng, crops, 4096, arch=arch, size=size, **kw)
                        else:
                            reid_inference.evaluate_reid(crops, lab, lab, lab, crops, lab, lab, lab, engine=eng, arch=arch, size=size,
                                                         verbose=False, **kw)
                    yield _id(entry, arch, kw, size), _record(current, call)
    floats = np.zeros((1, 3, 96, 72), np.float32)          # float images carry their size: (64, 64) is a good size that is not theirs
    for kw in _kw_product(KEYWORDS["extract_descriptors"]):
        for kind, images in (("u8", crops), ("f32", floats)):
            for size in (None, (96, 72), (31, 72), (64, 64)):
                def call(eng, kw=kw, images=images, size=size):
                    inference_utils.extract_descriptors(images, size=size, **kw)
                yield _id("extract_descriptors", kind, kw, size), _record(current, call)


def _stream_cases(current):
    blob = np.zeros(4, np.float32)
    classes = (("CameraStream", tracking.CameraStream, ()), ("MultiCameraStream", tracking.MultiCameraStream, (2,)),
               ("LookaheadCameraStream", tracking.LookaheadCameraStream, ()))
    for entry, cls, extra in classes:
        for arch in EVAL_ARCHS:
            for kw in _kw_product(KEYWORDS[entry]):
                for size in (None, (128, 64), (31, 64)):
                    for left_on in (False, True):
                        def call(eng, cls=cls, extra=extra, arch=arch, kw=kw, size=size):
                            cls(blob, "", *extra, arch=arch, own_context=False, **dict(kw, **({} if size is None else {"size": size})))
                        yield _id(entry, arch, kw, size, "left_on" if left_on else "fresh"), _record(current, call, left_on)


def cases():
    """(id, [kind, message, calls]) of every case, in a fixed order."""
    current = [None]
    with _stand_in_world(current):
        for gen in (_model_cases, _extractor_cases, _eval_cases, _stream_cases):
            for item in gen(current):
                yield item


def ids_digest(ids):
    return hashlib.sha256("\n".join(ids).encode()).hexdigest()


def pack(items, parent):
    """The trace file's form: the distinct records once, the cases as indices into them in enumeration order, and a digest of the ids
    (an enumerator that walks other cases than the recorded ones is told apart from code that behaves differently)."""
    distinct, index, refs, ids = [], {}, [], []
    for cid, rec in items:
        key = json.dumps(rec)
        if key not in index:
            index[key] = len(distinct)
            distinct.append(rec)
        refs.append(index[key])
        ids.append(cid)
    return {"parent_commit": parent, "what": "records of tests/hw_settings_cases.py on the parent commit; never regenerated from later code",
            "n_cases": len(ids), "ids_sha256": ids_digest(ids), "records": distinct, "cases": refs}


if __name__ == "__main__":
    out, parent = sys.argv[1], sys.argv[2]
    with open(out, "w") as f:
        json.dump(pack(list(cases()), parent), f, separators=(",", ":"))
        f.write("\n")
