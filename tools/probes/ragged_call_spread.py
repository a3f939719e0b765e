"""min / median / max host time of one reid_embed_ragged_u8 call (30 ragged crops, consecutive views of one pinned slab: the per-frame call of
a tracker that does not use the frame pipeline) over CALLS calls, in the headline arithmetic; repeated REPEATS times for the run-to-run spread.
A/B of two builds: REID_HIP_LIB=<other build>/libreid_hip.so python3 tools/probes/ragged_call_spread.py [CALLS [REPEATS]]"""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
from reid_amd import synth, weights
from reid_amd.engine import Engine

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 300
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 3
eng = Engine(0)
eng.load_seres18(*weights.pack_seres18(synth.seres18_state_dict(0))[:2])
eng.set_precision(2)
crops = synth.ragged_crops_u8(30, 2)
slab = eng.pinned(sum(c.size for c in crops))
views, at = [], 0
for c in crops:
    slab[at: at + c.size] = c.reshape(-1)
    views.append(slab[at: at + c.size].reshape(c.shape))
    at += c.size
for _ in range(20):
    eng.embed_ragged_u8(views)
for r in range(repeats):
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        eng.embed_ragged_u8(views)
        t.append((time.perf_counter() - t0) * 1e6)
    t.sort()
    print("SPREAD embed_ragged_u8 30 crops  repeat %d  min %7.1f  med %7.1f  max %7.1f us  (%d)" % (r, t[0], t[len(t) // 2], t[-1], len(t)))
eng.close()
