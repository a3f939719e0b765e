"""The any-size settings in Python (no GPU): every entry point's argument rules and setter calls equal, case for case, what the parent
commit of the settings refactor (8bfd4d39e7ce, named in the file too) produced - tests/golden/hw_settings_trace.json, written once by
tests/hw_settings_cases.py on that commit and never regenerated from later code - and Engine.hw_scope on a recording stand-in."""
import json
import os
import sys

import pytest

from reid_amd import _ffi
from reid_amd.engine import HW_SETTINGS, Engine

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hw_settings_cases as hc  # noqa: E402


@pytest.fixture(scope="module")
def trace(golden_dir):
    return json.load(open(os.path.join(golden_dir, "hw_settings_trace.json")))


@pytest.fixture(scope="module")
def items():
    return list(hc.cases())


def test_every_case_is_what_the_parent_commit_did(trace, items):
    assert trace["parent_commit"] == "8bfd4d39e7cebed9afd5ba9429a3a4c7280ecdde"
    ids = [cid for cid, _ in items]
    assert len(ids) == trace["n_cases"] == len(trace["cases"]) and hc.ids_digest(ids) == trace["ids_sha256"], "the enumerator walks other cases"
    differ = [(cid, rec, trace["records"][ref]) for (cid, rec), ref in zip(items, trace["cases"]) if rec != trace["records"][ref]]
    for cid, got, want in differ[:20]:
        print("%s\n  now:      %s\n  recorded: %s" % (cid, got, want))
    assert not differ, "%d of %d cases differ from the recorded ones" % (len(differ), len(ids))


def test_the_trace_is_not_vacuous(items):
    """Every entry point reaches its scopes or setters in some case (a _Stop with setter calls on record), and every keyword it takes is
    refused with a ValueError naming it in some case where it has its bad value."""
    by_entry = {e: [] for e in hc.ENTRY_POINTS}
    for cid, rec in items:
        by_entry[cid.split("/")[0]].append((cid, rec))
    for entry, rows in by_entry.items():
        assert any(rec[0] == "_Stop" and any(c[0].startswith("set_") for c in rec[2]) for _, rec in rows), entry
        for kw in hc.KEYWORDS[entry]:
            bad = "%s=%s" % (kw, "bogus" if kw in ("hw_precision", "precision") else 2)
            assert any(rec[0] == "ValueError" and kw in rec[1] and bad in cid for cid, rec in rows), (entry, kw)
    for s in hc.SETTINGS:                                                  # and every setter is on record somewhere
        assert any(c[0] == "set_" + s for _, rec in items for c in rec[2]), s


# ---------------------------------------------------------------------------------------------- Engine.hw_scope
class _Rec:
    """The five attributes and recording setters, nothing else: Engine.hw_scope is run on it unbound.  A setter named in `refuse` raises
    ReidHipError from its second call on - the restore of a scope that set it once."""

    def __init__(self, refuse=None, **start):
        self.calls, self.refuse = [], refuse
        self.hw_precision, self.hw_siblings, self.hw_ema, self.hw_f16, self.hw_sib_f16 = -1, False, False, False, False
        self.__dict__.update(start)


def _recording_setter(name):
    def setter(self, v):
        n = getattr(Engine, name + "_value")(v)
        n = n if name == "hw_precision" else bool(n)
        again = any(c[0] == name for c in self.calls)
        self.calls.append((name, n))
        if again and name == self.refuse:
            raise _ffi.ReidHipError(-1, "refused")
        setattr(self, name, n)
    return setter


for _s in hc.SETTINGS:
    setattr(_Rec, "set_" + _s, _recording_setter(_s))
ALL_ON = dict(precision="f16x3", siblings=True, ema=True, f16=True, sib_f16=True)
ENTER = [("hw_precision", 2), ("hw_siblings", True), ("hw_ema", True), ("hw_f16", True), ("hw_sib_f16", True)]
LEAVE = [("hw_sib_f16", False), ("hw_f16", False), ("hw_ema", False), ("hw_siblings", False), ("hw_precision", -1)]


def _state(rec):
    return [getattr(rec, s) for s in hc.SETTINGS]


def test_the_table_names_the_five_settings_in_scope_order():
    assert tuple(s.name for s in HW_SETTINGS) == hc.SETTINGS


def test_hw_scope_enters_in_table_order_and_leaves_in_reverse():
    rec = _Rec()
    with Engine.hw_scope(rec, **ALL_ON) as inside:
        assert inside is rec and rec.calls == ENTER and _state(rec) == [2, True, True, True, True]
    assert rec.calls == ENTER + LEAVE and _state(rec) == [-1, False, False, False, False]


def test_hw_scope_leaves_none_alone():
    rec = _Rec()
    with Engine.hw_scope(rec):
        assert rec.calls == []
    with Engine.hw_scope(rec, siblings=None, ema=True, f16=None, sib_f16=True, precision=None):
        assert rec.calls == [("hw_ema", True), ("hw_sib_f16", True)]
    assert rec.calls == [("hw_ema", True), ("hw_sib_f16", True), ("hw_sib_f16", False), ("hw_ema", False)]


def test_hw_scope_restores_after_an_exception_and_when_entering_fails():
    rec = _Rec()
    with pytest.raises(KeyError):
        with Engine.hw_scope(rec, **ALL_ON):
            raise KeyError("x")
    assert rec.calls == ENTER + LEAVE and _state(rec) == [-1, False, False, False, False]
    rec = _Rec()
    with pytest.raises(ValueError, match="hw_ema"):                        # the third setting refuses its value: the first two come back
        with Engine.hw_scope(rec, precision="f32", siblings=True, ema=2, f16=True):
            raise AssertionError("entered")
    assert rec.calls == [("hw_precision", 0), ("hw_siblings", True), ("hw_siblings", False), ("hw_precision", -1)]


def test_hw_scope_makes_no_setter_call_for_a_value_that_is_back_already():
    rec = _Rec(hw_precision=2, hw_f16=True)
    with Engine.hw_scope(rec, precision="f16x3", siblings=True, f16=True):
        pass
    assert rec.calls == [("hw_precision", 2), ("hw_siblings", True), ("hw_f16", True), ("hw_siblings", False)]
    assert _state(rec) == [2, False, False, True, False]


@pytest.mark.parametrize("name", hc.SETTINGS)
def test_only_hw_precision_swallows_a_refused_restore(name):
    """A ReidHipError from the restoring setter: hw_precision stays where it is, silently; any other setting's error leaves the scope.
    Either way every other setting comes back."""
    rec = _Rec(refuse=name)
    if name == "hw_precision":
        with Engine.hw_scope(rec, **ALL_ON):
            pass
    else:
        with pytest.raises(_ffi.ReidHipError):
            with Engine.hw_scope(rec, **ALL_ON):
                pass
    assert rec.calls == ENTER + LEAVE
    assert _state(rec) == [(2 if s == "hw_precision" else True) if s == name else (-1 if s == "hw_precision" else False) for s in hc.SETTINGS]


def test_hw_precision_swallows_that_error_only():
    class _Other(_Rec):
        def set_hw_precision(self, v):
            if self.calls:
                raise KeyError("another error")
            _Rec.set_hw_precision(self, v)
    rec = _Other()
    with pytest.raises(KeyError):
        with Engine.hw_scope(rec, precision=2):
            pass
