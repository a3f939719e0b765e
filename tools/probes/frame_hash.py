"""sha256 of what the ResNet frame pipeline returns (CameraStream, MultiCameraStream, LookaheadCameraStream; modes 0 / 1 / 2; match stream
on / off, banks seeded from the host, budget 3).  A/B of two builds - every line must match:
    python tools/probes/frame_hash.py > new.txt;  REID_HIP_LIB=<other build>/libreid_hip.so python tools/probes/frame_hash.py > old.txt
(entries of include/reid_hip.h that the build under test does not export yet are left unbound)"""
import ctypes
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, ".")
from reid_amd import _ffi, synth, weights

_built = ctypes.CDLL(_ffi.LIB_PATH)
for _name in [n for n in _ffi._SIGS if not hasattr(_built, n)]:
    print("not exported by the library under test: %s" % _name, file=sys.stderr)
    del _ffi._SIGS[_name]
_ffi.DEBUG_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(_ffi.LIB_PATH)), "libreid_hip_debug.so")
from reid_amd.tracking import CameraStream, LookaheadCameraStream, MultiCameraStream

print("library under test: %s" % _ffi.LIB_PATH, file=sys.stderr)


def sha(*arrs):
    return " ".join("-" * 16 if a is None else hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16] for a in arrs)


blob = weights.pack_seres18(synth.seres18_state_dict(0))[:2]
pool = synth.ragged_crops_u8(40, seed=3)
rng = np.random.default_rng(1)
sizes = rng.integers(1, 12, 8)
frames = [[pool[(5 * f + i) % 40] for i in range(int(s))] for f, s in enumerate(sizes)]
boxes = np.concatenate([rng.uniform(0, 500, (16, 2)), rng.uniform(20, 120, (16, 2))], 1)
tracks = [0, 1, 2, 3]
seed = rng.normal(size=(4, 512)).astype(np.float32)

for mode in (0, 1, 2):
    for ms in (True, False):
        cam = CameraStream(*blob, precision=mode, budget=3, max_tracks=8, match_stream=ms)
        cam.metric.partial_fit(seed, tracks, tracks)
        cam.submit(frames[0])
        for f, crops in enumerate(frames):
            tg = tracks
            feats, cost, iou = cam.step(tg, boxes[:len(tg)], boxes[:len(crops)], frames[f + 1] if f + 1 < len(frames) else None)
            k = min(len(crops), 4)
            cam.commit(list(range(k)), tracks[:k], tracks)
            print("camera mode %d ms %d frame %d  %s" % (mode, ms, f, sha(feats, cost, iou)))
        cam.close(destroy=True)
    mc = MultiCameraStream(*blob, 2, precision=mode, budget=3, max_tracks=8)
    mc.metrics[0].partial_fit(seed, tracks, tracks)
    mc.metrics[1].partial_fit(seed[:2], tracks[:2], tracks[:2])
    mc.submit([frames[0], frames[1]])
    for f in range(6):
        tg = [tracks, tracks[:2]]
        res = mc.step(tg, [boxes[:len(t)] for t in tg], [boxes[:len(frames[f])], boxes[:len(frames[f + 1])]],
                      [frames[f + 1], frames[f + 2]] if f + 1 < 6 else None)
        ks = [min(len(frames[f]), 4), min(len(frames[f + 1]), 2)]
        mc.commit([list(range(k)) for k in ks], [tracks[:k] for k in ks], [tracks, tracks[:2]])
        for c in range(2):
            print("multi mode %d frame %d camera %d  %s" % (mode, f, c, sha(*res[c])))
    mc.close(destroy=True)
    la = LookaheadCameraStream(*blob, frames_per_pass=2, precision=mode, budget=3, max_tracks=8)
    groups = [frames[i:i + 2] for i in range(0, 8, 2)]
    la.metric.partial_fit(seed, tracks, tracks)
    la.submit_group(groups[0])
    for g, group in enumerate(groups):
        for j, crops in enumerate(group):
            f = 2 * g + j
            tg = tracks
            nxt = groups[g + 1] if j == la.handover and g + 1 < len(groups) else None
            res = la.step(j, tg, boxes[:len(tg)], boxes[:len(crops)], next_group=nxt)
            k = min(len(crops), 4)
            la.commit(j, list(range(k)), tracks[:k], tracks)
            print("lookahead mode %d frame %d  %s" % (mode, f, sha(*res)))
    la.close(destroy=True)
