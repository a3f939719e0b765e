"""The frame pipeline with a Swin-T tracker on the MI355X (pytest -m gpu): reid_frame_submit_swin and the 96-wide cost kernel.

  kernel      bank_cost96_kernel (csrc/bank96.hip) through reid_debug_bank_cost96 against the float64 bank of tests/bank_ref.py.
  embeddings  frame_fetch after frame_submit_swin against swin_embed_ragged_u8, bit for bit.
  stream      CameraStream / MultiCameraStream / LookaheadCameraStream with arch="swin".
  both        a ResNet slot and a Swin slot on one context.
  refusals    no weights, a bad size, a missing libreid_hip_bank96.so.

Error bound of the kernel (tests/bank_ref.py derives the two formulas from the fp32 error model; nothing here is fitted).  Every sum
bank_cost96_kernel forms - a dot product, a detection's squared norm - is a chain of n = 6 + 4 roundings: lane l of a 16-lane group adds
its 6 products (elements 4l .. 4l + 3 and 64 + 2l, 64 + 2l + 1 of the row), and the 4-level butterfly adds the 16 lanes.  The samples'
squared norms are the write kernels': 1 product per thread at d = 96, 6 shuffle levels and 2 more additions, 9 <= n roundings.  With
u = 2^-24 and SAFETY = 2:  cosine |err| <= 2 (2n + 6) u = 52 u;  squared euclidean |err| <= 2 (2n + 3) u (|a|^2 + |b|^2) = 46 u (...).
bank_cost_kernel at d = 96 has n = ceil(96 / 64) + 8 = 10 as well, but another order of the additions: the two kernels agree within
these bounds, not bit for bit.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from reid_amd import _ffi, synth, weights
from reid_amd._ffi import check

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bank_ref as br  # noqa: E402
import swin_crops_ref as cref  # noqa: E402

pytestmark = pytest.mark.gpu

COS, L2 = _ffi.METRIC_COS, _ffi.METRIC_L2SQR
D = 96
STEP = 32            # samples of a track a block takes per step: 4 groups x NW96 = 8 waves (csrc/bank96.hip)
NUM_CLASS = 5


@pytest.fixture(scope="module")
def eng():
    from reid_amd.engine import get_engine
    e = get_engine(0)
    yield e
    e.set_precision(0)
    e.set_chunk(1024)
    e.debug_switch("bank_fast", 1)


@pytest.fixture(scope="module")
def crops():
    return cref.crop_set()[1]


@pytest.fixture(scope="module")
def blobs():
    return {v: weights.pack_swin(synth.swin_state_dict(0, num_class=NUM_CLASS, version=v))[:2] for v in ("v1", "v2")}


def _load(eng, blobs, version, mode):
    eng.set_precision(0)
    eng.load_swin(*blobs[version])
    eng.set_precision(mode)


class bank_fast:
    """Context manager: the cost kernel choice (debug switch `bank_fast`), restored on the way out."""

    def __init__(self, eng, value):
        self.eng, self.value = eng, value

    def __enter__(self):
        self.old = self.eng.debug_switch("bank_fast")
        self.eng.debug_switch("bank_fast", self.value)

    def __exit__(self, *exc):
        self.eng.debug_switch("bank_fast", self.old)


class DevBank:
    def __init__(self, eng, max_tracks, budget, d=D):
        self.eng, self.lib, self.budget, self.d = eng, eng.lib, budget, d
        self.h = C.c_void_p()
        check(self.lib.reid_bank_create(eng.h, max_tracks, budget, d, C.byref(self.h)))

    def update(self, feats, slots):
        f = np.ascontiguousarray(feats, np.float32).reshape(-1, self.d)
        s = np.ascontiguousarray(slots, np.int32)
        check(self.lib.reid_bank_update(self.eng.h, self.h, f.ctypes.data_as(C.c_void_p), s.ctypes.data_as(C.c_void_p), len(s)))

    def cost(self, slots, dets, metric, max_distance=None):
        s = np.ascontiguousarray(slots, np.int32)
        x = np.ascontiguousarray(dets, np.float32).reshape(-1, self.d)
        out = np.full((len(s), len(x)), np.nan, np.float32)
        check(self.lib.reid_bank_cost(self.eng.h, self.h, s.ctypes.data_as(C.c_void_p), len(s), x.ctypes.data_as(C.c_void_p), len(x),
                                      metric, C.c_float(-1.0 if max_distance is None else max_distance), out.ctypes.data_as(C.c_void_p)))
        return out

    def cost_dev(self, slots, dets, metric, max_distance=None):
        """reid_bank_cost_dev on a device copy of dets."""
        s = np.ascontiguousarray(slots, np.int32)
        x = np.ascontiguousarray(dets, np.float32).reshape(-1, self.d)
        out = np.full((len(s), len(x)), np.nan, np.float32)
        d_x, d_o = self.eng.malloc(x.nbytes), self.eng.malloc(out.nbytes)
        try:
            self.eng.h2d(d_x, x)
            check(self.lib.reid_bank_cost_dev(self.eng.h, self.h, s.ctypes.data_as(C.c_void_p), len(s), C.c_void_p(d_x), len(x), metric,
                                              C.c_float(-1.0 if max_distance is None else max_distance), C.c_void_p(d_o)))
            self.eng.sync()
            self.eng.d2h(out, d_o)
        finally:
            self.eng.free(d_x)
            self.eng.free(d_o)
        return out

    def close(self):
        self.eng.sync()
        self.lib.reid_bank_destroy(self.h)


# ----------------------------------------------------------------------------- 1. the kernel alone
# slot -> samples written.  0 .. 5: none, one group, a partial and a full wave, one sample into the second wave; STEP - 1 .. STEP + 1: the
# last group of the last wave idle, every group busy once, one sample into the second step; 130 writes at budget 100: a full, wrapped ring
TOTALS = {0: 0, 1: 1, 2: 3, 3: 4, 4: 5, 5: STEP - 1, 6: STEP, 7: STEP + 1, 8: 130}
BUDGET = 100


@pytest.fixture(scope="module")
def filled(eng):
    """(device bank, float64 reference, track directions): written once, read by every kernel test."""
    rng = np.random.default_rng(11)
    dirs = rng.normal(0, 1, (len(TOTALS), D)) * rng.uniform(0.5, 3.0, (len(TOTALS), 1))
    dev, ref = DevBank(eng, len(TOTALS), BUDGET), br.RefBank(BUDGET)
    for slot, total in TOTALS.items():
        if total:
            feats = (dirs[slot] + rng.normal(0, 1.0, (total, D))).astype(np.float32)
            dev.update(feats, np.full(total, slot, np.int32))
            ref.append(feats, [slot] * total)
    assert ref.count(8) == BUDGET and ref.count(0) == 0
    yield dev, ref, dirs
    dev.close()


@pytest.mark.parametrize("metric", [COS, L2], ids=["cosine", "euclidean"])
@pytest.mark.parametrize("m", [1, 15, 16, 17, 33])
def test_cost96_kernel_against_float64(eng, filled, m, metric):
    """Raw and gated costs of every track (sample counts TOTALS) against m detections: within the derived bound of the float64 bank; a
    track without samples is inf / the gate value; the launch writes every entry (they were NaN before it) and nothing behind them (the
    harness checks 16 guard words)."""
    dev, ref, dirs = filled
    rng = np.random.default_rng(100 * m + metric)
    dets = (dirs[rng.integers(0, len(TOTALS), m)] + rng.normal(0, 1.0, (m, D))).astype(np.float32)
    slots = list(TOTALS)
    held = [s for s in slots if TOTALS[s]]
    raw = eng.debug_bank_cost96(dev.h, slots, dets, metric)
    assert raw.shape == (len(slots), m) and not np.isnan(raw).any()
    assert np.all(np.isposinf(raw[0]))
    worst = br.assert_close_to_ref(raw[1:], ref, held, dets, metric, br.CHAIN_96, None, "raw m=%d" % m)
    print("m=%d metric=%d: largest error / bound %.3f" % (m, metric, worst))
    thr = float(np.median(ref.cost(held, dets, metric)))            # places the gate among the entries, nothing else
    gated = eng.debug_bank_cost96(dev.h, slots, dets, metric, thr)
    assert not np.isnan(gated).any() and np.all(gated[0] == br.gate32(thr))
    br.assert_close_to_ref(gated[1:], ref, held, dets, metric, br.CHAIN_96, thr, "gated m=%d" % m)
    assert (gated[1:] == br.gate32(thr)).any() and (gated[1:] < br.gate32(thr)).any()
    # any order of the tracks, a track twice: rows move with their slots
    order = [8, 0, 3, 8, 6]
    np.testing.assert_array_equal(eng.debug_bank_cost96(dev.h, order, dets, metric), raw[order])


def test_cost96_kernel_drops_nan_costs(eng):
    """One NaN sample row and one zero detection row: under the cosine metric the NaN sample drops out of the minimum and the zero
    detection (0 / 0) matches nothing - inf raw, the gate value gated; under the euclidean metric the zero detection is an ordinary row."""
    rng = np.random.default_rng(5)
    good = rng.normal(0, 1, (3, D)).astype(np.float32)
    bad = good[0].copy()
    bad[17] = np.nan
    dets = rng.normal(0, 1, (3, D)).astype(np.float32)
    dets[1] = 0.0
    dev, ref = DevBank(eng, 4, 8), br.RefBank(8)
    try:
        dev.update(np.stack([good[0], bad, good[1]]), [0, 0, 0])       # track 0: two good samples around a NaN one
        dev.update(np.stack([bad]), [1])                               # track 1: the NaN sample only
        ref.append(good[:2], [0, 0])
        for metric in (COS, L2):
            raw = eng.debug_bank_cost96(dev.h, [0, 1], dets, metric)
            gated = eng.debug_bank_cost96(dev.h, [0, 1], dets, metric, 0.5)
            assert not np.isnan(raw).any() and not np.isnan(gated).any()
            assert np.all(np.isposinf(raw[1])) and np.all(gated[1] == br.gate32(0.5))
            cols = [0, 2] if metric == COS else [0, 1, 2]
            br.assert_close_to_ref(raw[:1, cols], ref, [0], dets[cols], metric, br.CHAIN_96, None, "NaN sample, metric %d" % metric)
            if metric == COS:
                assert np.isposinf(raw[0, 1]) and gated[0, 1] == br.gate32(0.5)
    finally:
        dev.close()


def test_bank_fast_0_is_the_generic_kernel(eng, filled):
    """With the `bank_fast` switch at 0 the frame pipeline's launch is bank_cost_kernel, the kernel reid_bank_cost and
    reid_bank_cost_dev run on a 96-wide bank with either setting: the same bits.  At 1 the two kernels agree within their bounds."""
    dev, ref, dirs = filled
    rng = np.random.default_rng(8)
    dets = (dirs[rng.integers(0, len(TOTALS), 21)] + rng.normal(0, 1.0, (21, D))).astype(np.float32)
    slots = list(TOTALS)
    for metric in (COS, L2):
        for thr in (None, 0.7 if metric == COS else 150.0):
            want = dev.cost(slots, dets, metric, thr)
            np.testing.assert_array_equal(dev.cost_dev(slots, dets, metric, thr), want)
            with bank_fast(eng, 0):
                np.testing.assert_array_equal(eng.debug_bank_cost96(dev.h, slots, dets, metric, thr), want)
                np.testing.assert_array_equal(dev.cost(slots, dets, metric, thr), want)
        fast = eng.debug_bank_cost96(dev.h, slots[1:], dets, metric)
        slow = dev.cost(slots[1:], dets, metric)
        tol = ref.bound(slots[1:], dets, metric, br.CHAIN_96) + ref.bound(slots[1:], dets, metric, br.chain_generic(D))
        assert np.all(np.abs(fast.astype(np.float64) - slow) <= tol)


# ----------------------------------------------------------------------------- 2. embeddings
def _frame_emb(eng, slot, crops, **kw):
    eng.frame_submit_swin(slot, crops, **kw)
    eng.frame_cost(slot, want_emb=True)
    emb, cost, iou = eng.frame_fetch(slot)
    assert cost is None and iou is None
    return emb


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["fp32", "fp16-storage", "fp32-class"])
@pytest.mark.parametrize("version", ["v1", "v2"])
def test_frame_embeddings_equal_the_blocking_entry(eng, crops, blobs, version, mode):
    """frame_fetch after frame_submit_swin returns the bits of swin_embed_ragged_u8 on the same crops: one crop and seven, both slots."""
    _load(eng, blobs, version, mode)
    for slot, m in ((0, 1), (1, 7)):
        want = eng.swin_embed_ragged_u8(crops[:m])
        got = _frame_emb(eng, slot, crops[:m])
        assert got.shape == (m, D) and got.dtype == np.float32 and np.isfinite(got).all()
        np.testing.assert_array_equal(got, want)
        assert eng.frame_dim(slot) == D
    assert eng.fault_bits() == 0


def test_frame_embeddings_at_448x224_with_another_mean_std(eng, crops, blobs):
    _load(eng, blobs, "v1", 2)
    kw = dict(size=(448, 224), mean_std=cref.OTHER_MEAN_STD)
    want = eng.swin_embed_ragged_u8(crops[5:8], **kw)
    np.testing.assert_array_equal(_frame_emb(eng, 0, crops[5:8], **kw), want)
    assert not np.array_equal(want, eng.swin_embed_ragged_u8(crops[5:8], size=(448, 224)))


def test_frame_embeddings_in_three_passes_and_an_empty_frame(eng, crops, blobs):
    """m = 11 with passes of 4 crops (4 + 4 + 3), and m = 0."""
    _load(eng, blobs, "v1", 2)
    eleven = crops + crops[:2]
    want = eng.swin_embed_ragged_u8(eleven)
    eng.set_chunk(4)
    try:
        np.testing.assert_array_equal(_frame_emb(eng, 1, eleven), want)
    finally:
        eng.set_chunk(1024)
    assert _frame_emb(eng, 0, []).shape == (0, D)
    np.testing.assert_array_equal(_frame_emb(eng, 0, eleven), want)


# ----------------------------------------------------------------------------- 3. the stream classes
ALL_A, ALL_B = [10, 11, 12, 13, 14], [20, 21, 22, 23, 24]


def _scenario(base, sizes, first):
    """Six frames (crop indices), and per frame (tracks fed by detection rows 0, 1, ..; active tracks): five tracks, the fourth leaves
    `active_targets` at frame 2 - its slot is cleared - and returns at frame 4; with budget 3 the ring of track `base` wraps."""
    t = [base + i for i in range(5)]
    gone = [t[0], t[1], t[2], t[4]]
    plan = [(t, t), ([t[1], t[2], t[3], t[4], t[0]], t), ([t[2], t[4], t[0]], gone), ([t[4], t[0], t[1], t[2]], gone),
            ([t[3], t[0], t[1], t[2]], t), (t, t)]
    frames = [[(first + 3 * f + i) % 9 for i in range(m)] for f, m in enumerate(sizes)]
    assert all(3 <= m <= 9 and m >= len(p[0]) for m, p in zip(sizes, plan))
    return frames, plan


SCN = {"A": _scenario(10, [5, 7, 3, 9, 4, 6], 0), "B": _scenario(20, [6, 5, 8, 4, 5, 7], 4)}
STREAM_BUDGET, STREAM_MODE = 3, 2


def _boxes(rng, n):
    return np.concatenate([rng.uniform(0, 500, (n, 2)), rng.uniform(20, 200, (n, 2))], 1)


def _walk(name):
    """Per frame of scenario `name`: (crop indices, targets of the step, track boxes, detection boxes, rows, tracks, active)."""
    frames, plan = SCN[name]
    rng = np.random.default_rng(len(name) + ord(name[0]))
    alive = []
    for idx, (tg, active) in zip(frames, plan):
        yield idx, list(alive), _boxes(rng, len(alive)), _boxes(rng, len(idx)), list(range(len(tg))), list(tg), list(active)
        alive = list(active)


def _run_camera(crops, blob, name, metric, max_dist, match_stream):
    from reid_amd.tracking import CameraStream
    steps, log = list(_walk(name)), []
    cam = CameraStream(*blob, precision=STREAM_MODE, max_dist=max_dist, budget=STREAM_BUDGET, metric=metric, max_tracks=8,
                       match_stream=match_stream, arch="swin")
    try:
        cam.submit([crops[i] for i in steps[0][0]])      # no partial_fit anywhere: the bank is created inside the first step
        for f, (idx, targets, tb, db, rows, tg, active) in enumerate(steps):
            nxt = [crops[i] for i in steps[f + 1][0]] if f + 1 < len(steps) else None
            feats, cost, iou = cam.step(targets, tb, db, nxt)
            cam.commit(rows, tg, active)
            log.append((feats.copy(), cost.copy(), None if iou is None else iou.copy()))
    finally:
        cam.close(destroy=True)
    return log


def _run_multi(crops, blob, metric, max_dist):
    from reid_amd.tracking import MultiCameraStream
    steps, log = [list(_walk("A")), list(_walk("B"))], [[], []]
    cams = MultiCameraStream(*blob, 2, precision=STREAM_MODE, max_dist=max_dist, budget=STREAM_BUDGET, metric=metric, max_tracks=8, arch="swin")
    try:
        cams.submit([[crops[i] for i in s[0][0]] for s in steps])
        for f in range(6):
            cur = [s[f] for s in steps]
            nxt = [[crops[i] for i in s[f + 1][0]] for s in steps] if f + 1 < 6 else None
            res = cams.step([c[1] for c in cur], [c[2] for c in cur], [c[3] for c in cur], nxt)
            cams.commit([c[4] for c in cur], [c[5] for c in cur], [c[6] for c in cur])
            for c in range(2):
                log[c].append((res[c][0].copy(), res[c][1].copy(), None if res[c][2] is None else res[c][2].copy()))
    finally:
        cams.close(destroy=True)
    return log


def _run_lookahead(crops, blob, metric, max_dist):
    from reid_amd.tracking import LookaheadCameraStream
    steps, log = list(_walk("A")), []
    groups = [steps[i:i + 2] for i in range(0, 6, 2)]
    as_crops = lambda group: [[crops[i] for i in st[0]] for st in group]
    s = LookaheadCameraStream(*blob, frames_per_pass=2, precision=STREAM_MODE, max_dist=max_dist, budget=STREAM_BUDGET, metric=metric,
                              max_tracks=8, arch="swin")
    try:
        s.submit_group(as_crops(groups[0]))
        for g, group in enumerate(groups):
            for j, (idx, targets, tb, db, rows, tg, active) in enumerate(group):
                nxt = as_crops(groups[g + 1]) if j == s.handover and g + 1 < len(groups) else None
                feats, cost, iou = s.step(j, targets, tb, db, next_group=nxt)
                s.commit(j, rows, tg, active)
                log.append((feats.copy(), cost.copy(), None if iou is None else iou.copy()))
    finally:
        s.close(destroy=True)
    return log


def _same(a, b):
    assert len(a) == len(b) == 6
    for (fa, ca, ia), (fb, cb, ib) in zip(a, b):
        np.testing.assert_array_equal(fa, fb)
        np.testing.assert_array_equal(ca, cb)
        assert (ia is None) == (ib is None)
        if ia is not None:
            np.testing.assert_array_equal(ia, ib)


@pytest.mark.parametrize("metric", ["cosine", "euclidean"])
def test_streams_with_a_swin_tracker(eng, crops, blobs, metric):
    """CameraStream(arch="swin") over six frames of 3 - 9 crops from a cold start (the bank is created inside the first step): every
    frame's gated cost follows the float64 bank fed the device's own features, the DIoU cost is reid_diou_cost's, match_stream on and off
    give the same bits; a two-camera MultiCameraStream and LookaheadCameraStream(frames_per_pass=2) return the features and costs of the
    cameras' own CameraStream runs bit for bit (a Swin embedding does not depend on the pass it is computed in)."""
    code = COS if metric == "cosine" else L2
    _load(eng, blobs, "v1", STREAM_MODE)
    all_emb = eng.swin_embed_ragged_u8(crops).astype(np.float64)
    probe = br.RefBank(9)
    probe.append(all_emb, range(9))
    pair = probe.cost(range(9), all_emb, code)
    max_dist = float(np.median(pair[~np.eye(9, dtype=bool)]))       # places the gate among the costs, nothing else
    blob = blobs["v1"]
    on = {n: _run_camera(crops, blob, n, metric, max_dist, True) for n in ("A", "B")}
    compared = 0
    for name in ("A", "B"):
        ref = br.RefBank(STREAM_BUDGET)
        for (idx, targets, tb, db, rows, tg, active), (feats, cost, iou) in zip(_walk(name), on[name]):
            np.testing.assert_array_equal(feats, all_emb[idx].astype(np.float32))
            assert feats.shape == (len(idx), D) and cost.shape == (len(targets), len(idx))
            if targets:
                br.assert_close_to_ref(cost.astype(np.float32), ref, targets, feats, code, br.CHAIN_96, max_dist, "%s %s" % (name, idx))
                np.testing.assert_array_equal(iou, eng.diou_cost(tb, db))
                compared += cost.size
            else:
                assert iou is None
            ref.partial_fit(feats[rows], tg, active)
        assert ref.count(SCN[name][1][0][0][0]) == STREAM_BUDGET
    assert compared > 150
    _same(_run_camera(crops, blob, "A", metric, max_dist, False), on["A"])
    multi = _run_multi(crops, blob, metric, max_dist)
    _same(multi[0], on["A"])
    _same(multi[1], on["B"])
    _same(_run_lookahead(crops, blob, metric, max_dist), on["A"])


# ----------------------------------------------------------------------------- 4. both backbones on one context
def _resnet_frame(e, blob_manifest, crops, feats, load=True):
    """Slot 0 through the ResNet: (embeddings, cost against a 512-wide bank holding `feats` on tracks 0 .. 2, the bank)."""
    if load:
        e.load_seres18(*blob_manifest)
    e.set_precision(STREAM_MODE)
    bank = DevBank(e, 4, 5, 512)
    bank.update(feats, [0, 1, 2, 0, 1, 2])
    e.frame_submit(0, crops)
    e.frame_cost(0, bank.h, [2, 0, 1], COS, 0.6)
    emb, cost, _ = e.frame_fetch(0)
    return emb, cost, bank


def test_a_resnet_slot_and_a_swin_slot_on_one_context(eng, crops, blobs):
    """Slot 0 submitted by frame_submit, slot 1 by frame_submit_swin: 512- and 96-wide embeddings come back; a bank of the other
    width is REID_ERR_ARG naming both widths and leaves the slot as it was; the ResNet slot's embeddings and costs are those of a
    context that never saw a Swin."""
    from reid_amd.engine import Engine
    sd = synth.seres18_state_dict(0, num_class=NUM_CLASS)
    se = weights.pack_seres18(sd)[:2]
    feats = np.random.default_rng(2).normal(0, 1, (6, 512)).astype(np.float32)
    fresh = Engine(0)
    try:
        want_emb, want_cost, fb = _resnet_frame(fresh, se, crops[:6], feats)
        fb.close()
    finally:
        fresh.close()
    _load(eng, blobs, "v2", STREAM_MODE)
    eng.load_seres18(*se)
    eng.set_precision(STREAM_MODE)
    b512, b96 = DevBank(eng, 4, 5, 512), DevBank(eng, 4, 5, 96)
    try:
        b512.update(feats, [0, 1, 2, 0, 1, 2])
        b96.update(feats[:, :96], [0, 1, 2, 0, 1, 2])
        eng.frame_submit(0, crops[:6])
        eng.frame_submit_swin(1, crops[:4])
        assert (eng.frame_dim(0), eng.frame_dim(1)) == (512, D)
        sl = np.array([2, 0, 1], np.int32)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        for slot, bank in ((1, b512), (0, b96)):
            assert eng.lib.reid_frame_cost(eng.h, slot, bank.h, p(sl), 3, COS, C.c_float(0.6), None, None, 1) == -1
            msg = eng.lib.reid_last_error()
            assert b"512" in msg and b"96" in msg, msg
            assert eng.lib.reid_frame_update(eng.h, slot, bank.h, p(sl), p(sl), 3) == -1
            assert eng.lib.reid_frame_fetch(eng.h, slot, None, None, None) == -3      # no cost stage was queued
        eng.frame_cost(0, b512.h, sl, COS, 0.6)
        eng.frame_cost(1, b96.h, sl, COS, 0.6)
        emb0, cost0, _ = eng.frame_fetch(0)
        emb1, cost1, _ = eng.frame_fetch(1)
        assert emb0.shape == (6, 512) and emb1.shape == (4, D) and cost0.shape == (3, 6) and cost1.shape == (3, 4)
        np.testing.assert_array_equal(emb0, want_emb)
        np.testing.assert_array_equal(cost0, want_cost)
        np.testing.assert_array_equal(emb1, eng.swin_embed_ragged_u8(crops[:4]))
        ref = br.RefBank(5)
        ref.append(feats[:, :96], [0, 1, 2, 0, 1, 2])
        br.assert_close_to_ref(cost1, ref, sl, emb1, COS, br.CHAIN_96, 0.6, "swin slot")
        eng.frame_update(1, b96.h, [0, 3], [3, 3])                                     # the Swin slot feeds its bank
        fed = br.RefBank(5)
        fed.append(emb1[[0, 3]], [3, 3])
        br.assert_close_to_ref(b96.cost([3], emb1, L2), fed, [3], emb1, L2, br.chain_generic(D), None, "bank fed from the Swin slot")
        assert eng.fault_bits() == 0
    finally:
        b512.close()
        b96.close()


# ----------------------------------------------------------------------------- 5. refusals
def _raw_submit(e, crops, out_h=224, out_w=224, mean_std=None):
    pk, offsets, hw = cref.packed(crops)
    ms = None if mean_std is None else np.ascontiguousarray(mean_std, np.float32)
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    rc = e.lib.reid_frame_submit_swin(e.h, 0, p(pk), p(offsets), p(hw), len(crops), out_h, out_w, p(ms))
    e.sync()                                                         # pk is pageable and leaves scope: nothing may stay queued
    return rc


def test_refusals_come_before_anything_is_queued(eng, crops, blobs):
    from reid_amd.engine import Engine
    _load(eng, blobs, "v1", 0)
    want = _frame_emb(eng, 0, crops[:2])
    eng.frame_submit_swin(0, crops[:2])
    eng.frame_cost(0, want_emb=True)                                # a pending frame: a refused submit must leave it alone
    assert _raw_submit(eng, crops[:2], out_h=200) == -1
    assert _raw_submit(eng, crops[:2], out_w=448 + 1) == -1
    assert _raw_submit(eng, crops[:2], mean_std=[0.5, 0.5, 0.5, 0.2, 0.0, 0.2]) == -1
    np.testing.assert_array_equal(eng.frame_fetch(0)[0], want)
    with pytest.raises(ValueError):
        eng.frame_submit_swin(0, crops[:2], size=(200, 224))
    fresh = Engine(0)                                                # a second context, without Swin weights
    try:
        assert _raw_submit(fresh, crops[:2]) == -3
        assert b"reid_swin_load" in fresh.lib.reid_last_error()
        assert fresh.fault_bits() == 0
    finally:
        fresh.close()
    assert eng.fault_bits() == 0
    np.testing.assert_array_equal(_frame_emb(eng, 0, crops[:2]), want)


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from reid_amd import _ffi, synth, weights
from reid_amd.engine import get_engine
assert _ffi.LIB_PATH.startswith(sys.argv[1]), _ffi.LIB_PATH
eng = get_engine(0)
eng.load_swin(*weights.pack_swin(synth.swin_state_dict(0, num_class=5))[:2])
crop = [np.full((5, 4, 3), 7, np.uint8)]
before = eng.swin_embed_ragged_u8(crop)
try:
    eng.frame_submit_swin(0, crop)
except _ffi.ReidHipError as e:
    print("RAISED", e.status, e)
    ok = e.status == -3 and "libreid_hip_bank96.so" in str(e)
    ok = ok and eng.fault_bits() == 0 and np.array_equal(eng.swin_embed_ragged_u8(crop), before)
    sys.exit(0 if ok else 3)
sys.exit(4)
"""


def test_missing_library_is_an_error_of_the_swin_submit(tmp_path):
    """A copy of the package without libreid_hip_bank96.so, in a fresh child process: reid_frame_submit_swin returns REID_ERR_STATE
    naming the library before anything is queued, and the blocking crops entry works before and after it."""
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = "libreid_hip_bank96.so"
    shutil.copytree(os.path.join(root, "reid_amd"), tmp_path / "reid_amd", ignore=shutil.ignore_patterns("__pycache__"))
    shutil.copytree(os.path.join(root, "real-time-reid-tracking_amd"), tmp_path / "real-time-reid-tracking_amd",
                    ignore=shutil.ignore_patterns("__pycache__", "csrc", lib))
    assert not (tmp_path / "real-time-reid-tracking_amd" / lib).exists()
    r = subprocess.run([sys.executable, "-c", _CHILD, str(tmp_path)], capture_output=True, text=True, timeout=300, cwd=str(tmp_path),
                       env=dict(os.environ))
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "RAISED -3" in r.stdout and lib in r.stdout
