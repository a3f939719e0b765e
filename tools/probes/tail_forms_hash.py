"""sha256 of every output of the block-tail debug forms (SE tail forms 0-9 on exact-gate and random operands, IBN finish forms 1-3, se_tail +
GeM) at the shapes of tests/test_gpu_tail_stream.py, and whether SE form 0 equals forms 1-9 ("=" or "!<elements that differ>"): an A/B of two
builds - run it with each build's checkout as the working directory and diff the two outputs:
    cd <checkout> && python3 <this repo>/tools/probes/tail_forms_hash.py"""
import hashlib, os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "tests"))
import test_gpu_tail_stream as t
from reid_amd import synth, weights
from reid_amd.engine import get_engine
eng = get_engine(0)
eng.load_seres18(*weights.pack_seres18(synth.seres18_state_dict(0))[:2])
def h(a):
    return "-" if a is None else hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:12]
for gate in ("exact", "random"):
    for shape, tiles in t.SE_CASES:
        n, hw, c, mid = shape
        ops = t.se_operands(n, hw, c, mid, tiles, gate, n + hw + (gate == "random"))
        want = eng.debug_se_tail(0, *ops)[0]
        line = []
        for form in range(1, 10):
            out, pk, _ = eng.debug_se_tail(form, *ops)
            agree = "" if out is None else ("=" if np.array_equal(out, want) else "!%d" % int((out != want).sum()))
            line.append("%d:%s%s/%s" % (form, agree, h(out), h(pk)))
        print("SE", gate, shape, tiles, "form0", h(want), " ".join(line), flush=True)
for shape, tiles in t.PACK_CASES:
    n, hw, c, half = shape
    rng = np.random.default_rng(n + hw + c)
    x = rng.normal(size=(n, hw, c)).astype(np.float32)
    s1 = (rng.normal(size=(n, tiles, c)) * 0.3 * hw / tiles).astype(np.float32)
    s2 = (rng.uniform(1.0, 2.0, (n, tiles, c)) * hw / tiles).astype(np.float32)
    stats = np.stack([s1, s2], -1)
    gamma = rng.uniform(0.5, 1.5, half).astype(np.float32)
    beta = rng.normal(size=half).astype(np.float32)
    print("IN", shape, tiles, " ".join("%d:%s" % (f, h(eng.debug_norm_finish(f, x, stats, gamma, beta)[1 if f > 1 else 0])) for f in (1, 2, 3)), flush=True)
for hw, p in t.GEM_CASES:
    stats, w1, w2t, y, sc, scale, shift = t.gem_operands(hw, 300 + hw)
    x = eng.debug_se_tail(4, stats, w1, w2t, y, sc)[0]
    g, e = eng.debug_gem_neck(x, p, scale, shift)
    print("GEM", hw, p, h(x), h(g), h(e), flush=True)
