"""sha256 of what the eight embed entry points return (embeddings, and logits) over precisions, host_pipeline 0 / 1, one pass, several
passes with a ragged last one and n = 1, then the status every entry returns for bad arguments, missing weights, n == 0, bad crops /
boxes and a missing crops library.  A/B of two builds - every line must match:
    python tools/probes/entry_hash.py > new.txt;  REID_HIP_LIB=<other build>/libreid_hip.so python tools/probes/entry_hash.py > old.txt
(the debug library, which moves host_pipeline, is taken from the directory of the product library under test)"""
import ctypes as C
import hashlib
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, ".")
from reid_amd import _ffi, synth, weights

_ffi.DEBUG_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(_ffi.LIB_PATH)), "libreid_hip_debug.so")
from reid_amd.engine import Engine

print("library under test: %s" % _ffi.LIB_PATH, file=sys.stderr)

FH, FW = 480, 640


def sha(*arrs):
    return " ".join(hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16] for a in arrs)


def p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def boxes_for(n, seed):
    rng = np.random.default_rng(seed)
    x1, y1 = rng.integers(0, FW - 130, n), rng.integers(0, FH - 260, n)
    b = np.stack([x1, y1, x1 + rng.integers(3, 130, n), y1 + rng.integers(8, 260, n)], 1).astype(np.int32)
    b[0] = [FW - 50, FH - 90, FW, FH]                     # touches the frame's border
    return b


def dev_call(eng, fn, x, n, dim, nc):
    """A *_dev entry on a device copy of x: fn(d_x, d_emb, d_logits)."""
    d_x, d_e, d_l = eng.malloc(max(x.nbytes, 16)), eng.malloc(n * dim * 4 + 16), eng.malloc(n * nc * 4 + 16)
    try:
        eng.h2d(d_x, x)
        fn(d_x, d_e, d_l)
        eng.sync()
        return eng.d2h(np.empty((n, dim), np.float32), d_e), eng.d2h(np.empty((n, nc), np.float32), d_l)
    finally:
        for d in (d_x, d_e, d_l):
            eng.free(d)


def hashes():
    eng = Engine(0)
    eng.load_seres18(*weights.pack_seres18(synth.seres18_state_dict(0))[:2])
    crops = synth.smooth_crops_u8(19, 3)
    x = ((crops.astype(np.float32) / 255.0 - 0.5) / 0.5).transpose(0, 3, 1, 2).copy()
    rag = synth.ragged_crops_u8(19, 4)
    frame = np.random.default_rng(5).integers(0, 256, (FH, FW, 3), dtype=np.uint8)
    eng.set_chunk(8)
    for mode in (0, 2, 1):
        eng.set_precision(mode)
        for hp in (0, 1):
            eng.debug_switch("host_pipeline", hp)
            for n in (1, 5, 19) if mode != 1 else (19,):
                tag = "se mode %d pipeline %d n %2d" % (mode, hp, n)
                print(tag, "u8          ", sha(*eng.embed_u8(crops[:n], logits=True)))
                print(tag, "f32_nchw    ", sha(*eng.embed_f32_nchw(x[:n], logits=True)))
                print(tag, "ragged_u8   ", sha(*eng.embed_ragged_u8(rag[:n], logits=True)))
                print(tag, "frame_u8    ", sha(*eng.embed_frame_u8(frame, boxes_for(n, n), logits=True)))
                if hp == 0:
                    nc = eng.num_class
                    print(tag, "u8_dev      ", sha(*dev_call(eng, lambda a, e, l: eng.embed_u8_dev(a, n, e, l), crops[:n], n, 512, nc)))
                    print(tag, "f32_nchw_dev", sha(*dev_call(eng, lambda a, e, l: eng.embed_f32_nchw_dev(a, n, e, l), x[:n], n, 512, nc)))
    eng.set_precision(0)
    eng.load_swin(*weights.pack_swin(synth.swin_state_dict(0, num_class=8))[:2])
    eng.set_chunk(2)
    for mode in (0, 2):
        eng.set_precision(mode)
        for h, w in ((224, 224), (448, 224)):
            imgs = synth.images_f32(5, 7, h, w)
            for hp in (0, 1):
                eng.debug_switch("host_pipeline", hp)
                for n in (1, 5):
                    tag = "swin %dx%d mode %d pipeline %d n %d" % (h, w, mode, hp, n)
                    print(tag, "f32_nchw    ", sha(*eng.swin_embed_f32_nchw(imgs[:n], logits=True)))
                    print(tag, "ragged_u8   ", sha(*eng.swin_embed_ragged_u8(rag[:n], size=(h, w), logits=True)))
                    print(tag, "frame_u8    ", sha(*eng.swin_embed_frame_u8(frame, boxes_for(n, n), size=(h, w), logits=True)))
                    if hp == 0:
                        print(tag, "f32_nchw_dev", sha(*dev_call(eng, lambda a, e, l: eng.swin_embed_dev(a, n, h, w, e, l), imgs[:n], n, 96, 8)))
    eng.debug_switch("host_pipeline", 1)
    eng.set_precision(0)
    eng.set_chunk(1024)
    return eng


def entry_calls(eng, n, dim=512, emb_null=False, hw_bad=None, off_bad=None, box_bad=None, only=None):
    """{entry: status} of every host / device entry with n items (n may be 0 or -1) and one defect at most."""
    lib, h = eng.lib, eng.h
    k = max(n, 1)
    rng = np.random.default_rng(11)
    crops = rng.integers(0, 256, (k, 256, 128, 3), dtype=np.uint8)
    x = rng.uniform(-1, 1, (k, 3, 256, 128)).astype(np.float32)
    xs = rng.uniform(-1, 1, (k, 3, 224, 224)).astype(np.float32)
    hw = np.tile(np.asarray([[6, 5]], np.int32), (k, 1))
    offs = (np.arange(k) * 90).astype(np.int64)
    if hw_bad is not None:
        hw[k - 1] = hw_bad
    if off_bad is not None:
        offs[k - 1] = off_bad
    packed = rng.integers(0, 256, k * 90 + 90, dtype=np.uint8)
    frame = rng.integers(0, 256, (60, 80, 3), dtype=np.uint8)
    boxes = np.tile(np.asarray([[1, 2, 30, 50]], np.int32), (k, 1))
    if box_bad is not None:
        boxes[k - 1] = box_bad
    emb = None if emb_null else np.zeros((k, 512), np.float32)
    d = eng.malloc(max(xs.nbytes, x.nbytes))
    d_e = eng.malloc(k * 512 * 4)
    eng.h2d(d, xs)                                       # the device entries read finite values, whatever their element type
    de = None if emb_null else C.c_void_p(d_e)
    calls = {
        "reid_embed_u8_dev": lambda: lib.reid_embed_u8_dev(h, C.c_void_p(d), n, de, None),
        "reid_embed_f32_nchw_dev": lambda: lib.reid_embed_f32_nchw_dev(h, C.c_void_p(d), n, de, None),
        "reid_embed_u8": lambda: lib.reid_embed_u8(h, p(crops), n, p(emb), None),
        "reid_embed_f32_nchw": lambda: lib.reid_embed_f32_nchw(h, p(x), n, p(emb), None),
        "reid_embed_ragged_u8": lambda: lib.reid_embed_ragged_u8(h, p(packed), p(offs), p(hw), n, p(emb), None),
        "reid_embed_frame_u8": lambda: lib.reid_embed_frame_u8(h, p(frame), 60, 80, p(boxes), n, p(emb), None),
        "reid_swin_embed_f32_nchw_dev": lambda: lib.reid_swin_embed_f32_nchw_dev(h, C.c_void_p(d), n, 224, 224, de, None),
        "reid_swin_embed_f32_nchw": lambda: lib.reid_swin_embed_f32_nchw(h, p(xs), n, 224, 224, p(emb), None),
        "reid_swin_embed_ragged_u8": lambda: lib.reid_swin_embed_ragged_u8(h, p(packed), p(offs), p(hw), n, 224, 224, None, p(emb), None),
        "reid_swin_embed_frame_u8": lambda: lib.reid_swin_embed_frame_u8(h, p(frame), 60, 80, p(boxes), n, 224, 224, None, p(emb), None),
    }
    try:
        return {name: fn() for name, fn in calls.items() if only is None or only in name}
    finally:
        eng.sync()
        eng.free(d)
        eng.free(d_e)


def statuses(loaded):
    def table(state, eng):
        rows = [("emb = NULL, n = 1", dict(n=1, emb_null=True)), ("n = -1", dict(n=-1)), ("n = 0", dict(n=0)), ("n = 1", dict(n=1)),
                ("crop with h = 0 (last of 2)", dict(n=2, hw_bad=[0, 5], only="ragged")),
                ("crop with w = 0 (n = 1)", dict(n=1, hw_bad=[5, 0], only="ragged")),
                ("negative offset (last of 2)", dict(n=2, off_bad=-3, only="ragged")),
                ("empty box (last of 2)", dict(n=2, box_bad=[10, 10, 10, 50], only="frame")),
                ("box beyond the frame (n = 1)", dict(n=1, box_bad=[0, 0, 81, 50], only="frame")),
                ("box with x1 < 0 (n = 1)", dict(n=1, box_bad=[-1, 0, 40, 50], only="frame")),
                ("size 200x224, n = 1", None)]
        for what, kw in rows:
            if kw is None:
                emb, z = np.zeros((1, 96), np.float32), np.zeros(400, np.uint8)
                o, s = np.zeros(1, np.int64), np.asarray([[6, 5]], np.int32)
                b = np.asarray([[1, 2, 30, 50]], np.int32)
                got = {"reid_swin_embed_ragged_u8": eng.lib.reid_swin_embed_ragged_u8(eng.h, p(z), p(o), p(s), 1, 200, 224, None, p(emb), None),
                       "reid_swin_embed_frame_u8": eng.lib.reid_swin_embed_frame_u8(eng.h, p(np.zeros((60, 80, 3), np.uint8)), 60, 80, p(b), 1, 200,
                                                                                    224, None, p(emb), None)}
            else:
                got = entry_calls(eng, **kw)
            for name, st in got.items():
                print("STATUS %-12s %-30s %-30s %d   fault %d" % (state, what, name, st, eng.fault_bits()))
    fresh = Engine(0)
    table("no weights", fresh)
    fresh.close()
    table("weights", loaded)


def missing_crops_library():
    """The crops entries in a child process whose product library lies in a directory without libreid_hip_swin_crops.so."""
    src = os.path.dirname(os.path.abspath(_ffi.LIB_PATH))
    with tempfile.TemporaryDirectory() as tmp:
        for f in os.listdir(src):
            if f.startswith("libreid_hip") and f.endswith(".so") and "swin_crops" not in f:
                shutil.copy(os.path.join(src, f), tmp)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=dict(os.environ, REID_HIP_LIB=os.path.join(tmp, "libreid_hip.so")),
                           capture_output=True, text=True, timeout=300)
        sys.stdout.write(r.stdout.replace(tmp, "<dir>"))
        if r.returncode:
            sys.stdout.write("child exit %d\n%s" % (r.returncode, r.stderr[-2000:]))


def child():
    eng = Engine(0)
    eng.load_swin(*weights.pack_swin(synth.swin_state_dict(0, num_class=8))[:2])
    for n in (0, 1):
        for name, st in entry_calls(eng, n, only="swin_embed").items():
            msg = eng.lib.reid_last_error().decode() if st else ""
            print("STATUS %-12s %-30s %-30s %d   fault %d  %s" % ("no crops lib", "n = %d" % n, name, st, eng.fault_bits(), msg.split(":")[0]))
    eng.close()


# ---- the reid_*_hw entries (ResNet18-IBN-SE and its siblings at any input size) through Engine
HW_SIZES = ((128, 64), (75, 53), (256, 128))             # the last one runs the any-size forward under the switch anysize_force


def hw_entry_hashes(eng, tag):
    """Every _hw entry at HW_SIZES with the loaded weights and the settings the caller made: n = 1 and several passes with a ragged last one
    (chunk 2: passes of 8 at 128 x 64, of 16 at 75 x 53, of 2 at 256 x 128)."""
    rag = synth.ragged_crops_u8(19, 4)
    frame = np.random.default_rng(5).integers(0, 256, (FH, FW, 3), dtype=np.uint8)
    nc = eng.num_class
    eng.set_chunk(2)
    for h, w in HW_SIZES:
        forced = (h, w) == (256, 128)
        eng.debug_switch("anysize_force", int(forced))
        x = np.random.default_rng(h * w).uniform(-1, 1, (19, 3, h, w)).astype(np.float32)
        for n in (1, 5) if forced else (1, 19):
            t = "%s %dx%d n %2d" % (tag, h, w, n)
            if not forced:                               # Engine hands 256 x 128 host images to the entry without a size
                print(t, "f32_nchw    ", sha(*eng.embed_f32_nchw(x[:n], logits=True)))
            print(t, "f32_nchw_dev", sha(*dev_call(eng, lambda a, e, l: eng.embed_f32_nchw_dev(a, n, e, l, size=(h, w)), x[:n], n, 512, nc)))
            print(t, "ragged_u8   ", sha(*eng.embed_ragged_u8(rag[:n], logits=True, size=(h, w))))
            print(t, "frame_u8    ", sha(*eng.embed_frame_u8(frame, boxes_for(n, n), logits=True, size=(h, w))))
    eng.debug_switch("anysize_force", 0)


def hw_stage_hashes(eng, tag):
    """The eleven taps of one pass of 3 images at 75 x 53 under debug_keep."""
    x = np.random.default_rng(7).uniform(-1, 1, (3, 3, 75, 53)).astype(np.float32)
    eng.set_chunk(1024)
    eng.debug_keep(1)
    eng.embed_f32_nchw(x, logits=True)
    for s in range(11):
        print("%s stage %2d" % (tag, s), sha(eng.debug_stage(s, 3, size=(75, 53))))
    eng.debug_keep(0)


def hw_refusal(eng, what, h=128, w=64):
    x, emb = np.zeros((1, 3, h, w), np.float32), np.zeros((1, 512), np.float32)
    st = eng.lib.reid_embed_f32_nchw_hw(eng.h, p(x), 1, h, w, p(emb), None)
    msg = eng.lib.reid_last_error().decode() if st else ""
    print("STATUS hw %-45s %d   fault %d  %s" % (what, st, eng.fault_bits(), msg.split(";")[0]))


def hw_entries():
    eng = Engine(0)
    load = lambda sd: eng.load_seres18(*weights.pack_seres18(sd)[:2])
    load(synth.seres18_state_dict(0))
    hw_entry_hashes(eng, "hw seres18 default   ")
    hw_stage_hashes(eng, "hw seres18 default   ")
    hw_refusal(eng, "a side of 31", 31, 64)
    eng.set_precision(1)
    hw_refusal(eng, "precision mode 1 without hw_precision")
    eng.set_precision(0)
    eng.set_hw_precision(2)
    hw_entry_hashes(eng, "hw seres18 precision2")
    eng.set_hw_precision(None)
    eng.set_hw_f16(True)
    hw_entry_hashes(eng, "hw seres18 f16       ")
    hw_stage_hashes(eng, "hw seres18 f16       ")
    eng.set_hw_f16(False)
    load(synth.cares18_state_dict(0))
    hw_refusal(eng, "cares18_ibn without hw_siblings")
    eng.set_hw_f16(True)
    hw_refusal(eng, "hw_f16 with cares18_ibn loaded")
    eng.set_hw_f16(False)
    eng.set_hw_siblings(True)
    hw_entry_hashes(eng, "hw cares18 siblings  ")
    eng.set_hw_siblings(False)
    load(synth.emares18_state_dict(0))
    hw_refusal(eng, "emares18_ibn without hw_ema")
    eng.set_hw_ema(True)
    hw_entry_hashes(eng, "hw emares18 ema      ")
    eng.close()


def missing_anysize_f16_library():
    """The hw_f16 forward in a child process whose product library lies in a directory without libreid_hip_anysize_f16.so."""
    src = os.path.dirname(os.path.abspath(_ffi.LIB_PATH))
    with tempfile.TemporaryDirectory() as tmp:
        for f in os.listdir(src):
            if f.startswith("libreid_hip") and f.endswith(".so") and "anysize_f16" not in f:
                shutil.copy(os.path.join(src, f), tmp)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-hw"], env=dict(os.environ, REID_HIP_LIB=os.path.join(tmp, "libreid_hip.so")),
                           capture_output=True, text=True, timeout=300)
        sys.stdout.write(r.stdout.replace(tmp, "<dir>"))
        if r.returncode:
            sys.stdout.write("child exit %d\n%s" % (r.returncode, r.stderr[-2000:]))


def child_hw():
    eng = Engine(0)
    eng.load_seres18(*weights.pack_seres18(synth.seres18_state_dict(0))[:2])
    eng.set_hw_f16(True)
    x, emb = np.zeros((1, 3, 128, 64), np.float32), np.zeros((1, 512), np.float32)
    for n in (0, 1, 1):                                  # twice: a failed open is tried, and reported, again
        st = eng.lib.reid_embed_f32_nchw_hw(eng.h, p(x), n, 128, 64, p(emb), None)
        msg = eng.lib.reid_last_error().decode() if st else ""
        print("STATUS %-12s %-30s %-30s %d   fault %d  %s" % ("no f16 lib", "n = %d" % n, "reid_embed_f32_nchw_hw", st, eng.fault_bits(), msg.split(":")[0]))
    eng.set_hw_f16(False)
    st = eng.lib.reid_embed_f32_nchw_hw(eng.h, p(x), 1, 128, 64, p(emb), None)
    print("STATUS %-12s %-30s %-30s %d   fault %d  %s" % ("no f16 lib", "n = 1, hw_f16 off", "reid_embed_f32_nchw_hw", st, eng.fault_bits(), sha(emb)))
    eng.close()


if __name__ == "__main__":
    if "--child" in sys.argv:
        child()
    elif "--child-hw" in sys.argv:
        child_hw()
    else:
        e = hashes()
        statuses(e)
        e.close()
        missing_crops_library()
        hw_entries()
        missing_anysize_f16_library()
