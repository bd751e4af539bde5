"""tests/_knob_cases.py on a machine without a GPU: the covering array covers, stays small and does not change between two builds;
DEFAULTS is what struct zk_ctx starts with; a knob added to the binding fails here until it is tabled."""
import os
import re

from tests import _knob_cases as KC
from zotmer_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOT_TABLED = {"comm_chunk", "comm_self_loop"}          # the exchange's knobs: tests/_rccl_one_rank.py


def test_every_level_pair_is_in_a_row():
    rows = KC.pairwise_rows()
    names = [f[0] for f in KC.FACTORS]
    assert all(list(r) == names for r in rows)
    assert all(r[n] in lv for r in rows for n, lv in KC.FACTORS)
    pairs = KC.level_pairs()
    assert len(pairs) == sum(len(a[1]) * len(b[1]) for i, a in enumerate(KC.FACTORS) for b in KC.FACTORS[i + 1:]) == len(set(pairs))
    missing = [(names[i], a, names[j], b) for i, a, j, b in pairs if not any(r[names[i]] == a and r[names[j]] == b for r in rows)]
    assert not missing, missing[:10]


def test_array_is_small():
    sizes = sorted(len(lv) for _, lv in KC.FACTORS)
    assert sizes[-1] * sizes[-2] <= len(KC.pairwise_rows()) <= 96


def test_array_is_the_same_on_two_builds():
    first = [dict(r) for r in KC.pairwise_rows()]
    KC.pairwise_rows.cache_clear()
    again = KC.pairwise_rows()
    assert [dict(r) for r in again] == first and again is not first
    assert [dict(r) for r in KC.pairwise_rows(seed=2)] != first          # (the seed is read)


def test_defaults_are_the_initialisers_of_zk_ctx():
    text = open(os.path.join(ROOT, "zotmer_amd", "csrc", "internal.hpp")).read()
    body = text[text.index("struct zk_ctx {"):]
    body = body[:body.index("\n};")]
    inits = {m.group(1): int(m.group(2)) for m in re.finditer(r"^\s*int (\w+) = (-?\d+);", body, re.M)}
    for name, value in KC.DEFAULTS.items():
        assert inits.get(name) == value, (name, value, inits.get(name))
    assert KC.DEFAULTS["tag_words"] == native.DEFAULT_TAG_WORDS


def test_every_knob_of_the_binding_is_tabled():
    assert set(native.Context.TUNE_IDS) - NOT_TABLED == set(KC.DEFAULTS)
    factors = {f[0] for f in KC.FACTORS}
    assert set(KC.DEFAULTS) - {"kway"} == factors - set(KC.INPUT_FACTORS)
    for name, levels in KC.FACTORS:
        assert len(set(levels)) == len(levels) >= 2
        if name in KC.DEFAULTS:
            assert KC.DEFAULTS[name] in levels, name          # (the default of every knob is one of its levels)


def test_knobs_restores_every_default():
    class Ctx:
        def __init__(self):
            self.calls = []

        def tune(self, **kw):
            self.calls.append(kw)
    c = Ctx()
    try:
        with KC.knobs(c, sort_variant=5, dedupe_bits=16):
            assert c.calls == [dict(sort_variant=5, dedupe_bits=16)]
            raise KeyError("inside")
    except KeyError:
        pass
    assert c.calls[1:] == [KC.DEFAULTS]
    row = KC.pairwise_rows()[0]
    assert set(KC.knobs_of(row)) == set(KC.DEFAULTS) - {"kway"} and not set(KC.knobs_of(row)) & set(KC.INPUT_FACTORS)
