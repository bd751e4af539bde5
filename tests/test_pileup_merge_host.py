"""zk_pileup_merge and zk_narrow_counts without a device: the header and the binding agree, the numpy restatement the GPU tests
compare with (tests/_pileup_merge_cases.py) equals a dictionary on small random lists, the lists the GPU tests are made of are
what they claim to be, and Pileup.add_device is Pileup.add of the downloads."""
import os
import re

import numpy as np

from tests import _pileup_merge_cases as M
from zotmer_amd import native
from zotmer_amd.library import alufinder as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_binding_agree():
    text = open(os.path.join(ROOT, "include", "zotk.h")).read()
    assert int(re.search(r"#define ZK_PILEUP_MERGE_TILE (\d+)", text).group(1)) == native.PILEUP_MERGE_TILE
    assert int(re.search(r"#define ZK_PROF_PILEUP_MERGE (\d+)", text).group(1)) == native.Context.PROF_TAGS["pileup_merge"] == 50
    for name, n_args in (("zk_pileup_merge", 15), ("zk_narrow_counts", 5)):
        decl = re.search(r"int %s\(([^;]*)\);" % name, text)
        assert decl and len(decl.group(1).split(",")) == n_args == len(native.SIGNATURES[name][1])
    for f in ("pileup_merge_into", "pileup_merge", "narrow_counts"):
        assert callable(getattr(native.Context, f))
    assert sorted(native.Context.PROF_TAGS.values()) == list(range(1, 51))


def is_ascending(lst):
    c, x = lst[0].astype(object), lst[1].astype(object)
    keys = list(zip(c.tolist(), x.tolist()))
    return all(a < b for a, b in zip(keys, keys[1:]))


def test_restatement_against_a_dictionary():
    rng = np.random.default_rng(5)
    uni = M.universe(16)
    assert is_ascending(uni) and len(uni[0]) == 128
    for trial in range(60):
        na, nb = int(rng.integers(0, 40)), int(rng.integers(0, 40))
        bits = (32, 64)[trial & 1]
        a, b = M.layout(uni, M.LAYOUTS[trial % len(M.LAYOUTS)], na, nb, rng, bits)
        assert is_ascending(a) and is_ascending(b) and b[2].dtype.itemsize * 8 == bits
        c, x, n = M.merge_lists(a, b)
        assert c.dtype == np.uint32 and x.dtype == np.uint64 and n.dtype == np.uint64
        assert list(zip(c.tolist(), x.tolist(), n.tolist())) == M.merge_by_dict(a, b)
    # counts wrap modulo 2^64, and a carry leaves the low word
    one = (np.array([7], np.uint32), np.array([1 << 63], np.uint64))
    c, x, n = M.merge_lists(one + (np.array([(1 << 64) - 1], np.uint64),), one + (np.array([2], np.uint64),))
    assert n.tolist() == [1]
    c, x, n = M.merge_lists(one + (np.array([1], np.uint64),), one + (np.array([0xFFFFFFFF], np.uint32),))
    assert n.tolist() == [1 << 32]
    assert [len(v) for v in M.merge_lists(([], [], []), ([], [], []))] == [0, 0, 0]


def test_the_order_is_coordinate_then_kmer_both_unsigned():
    a = (np.array([1], np.uint32), np.array([1 << 63], np.uint64), np.array([1], np.uint64))
    b = (np.array([2, 1 << 31], np.uint32), np.array([0, 5], np.uint64), np.array([1, 1], np.uint64))
    c, x, _ = M.merge_lists(a, b)
    assert c.tolist() == [1, 2, 1 << 31] and x.tolist() == [1 << 63, 0, 5]


def test_layouts_and_boundaries_are_what_they_claim():
    rng = np.random.default_rng(9)
    uni = M.universe(64)
    key = lambda lst: set(zip(lst[0].tolist(), lst[1].tolist()))
    a, b = M.layout(uni, "disjoint", 50, 60, rng, 32)
    assert not key(a) & key(b) and (len(a[0]), len(b[0])) == (50, 60)
    a, b = M.layout(uni, "subset", 50, 60, rng, 32)
    assert key(b) <= key(a) and len(b[0]) == 50
    a, b = M.layout(uni, "equal", 50, 9, rng, 64)
    assert key(a) == key(b)
    a, b = M.layout(uni, "interleaved", 60, 50, rng, 32)
    assert len(key(a) & key(b)) == 16
    a, b = M.layout(uni, "a_below_b", 5, 6, rng, 32)
    assert max(key(a)) < min(key(b))
    a, b = M.layout(uni, "b_below_a", 5, 6, rng, 32)
    assert max(key(b)) < min(key(a))
    T = 16
    for shift in (-1, 0, 1):
        a, b = M.boundary_pairs(uni, T, 4, shift, rng, 32)
        assert is_ascending(a) and is_ascending(b) and len(a[0]) + len(b[0]) == 4 * T + shift
        # the merged order, A before B on ties
        tagged = sorted([(c, x, 0) for c, x in zip(a[0].tolist(), a[1].tolist())] + [(c, x, 1) for c, x in zip(b[0].tolist(), b[1].tolist())])
        for t in (1, 2, 3):
            p = t * T + shift
            assert tagged[p - 1][:2] == tagged[p][:2] and (tagged[p - 1][2], tagged[p][2]) == (0, 1)
    lists = M.random_lists(5, 100, 300, 3)
    assert all(is_ascending(l) and l[2].dtype == np.uint32 for l in lists)


class Down:
    """stands in for a DeviceArray"""

    def __init__(self, a):
        self.a, self.n = a, len(a)

    def to_host(self):
        return self.a.copy()


def test_pileup_add_device_is_add_of_the_downloads():
    lists = M.random_lists(6, 200, 500, 11)
    p, q = A.Pileup(merge_at=300), A.Pileup(merge_at=300)
    for c, x, n in lists:
        p.add(c, x, n)
        q.add_device(Down(c), Down(x), Down(n))
    q.add_device(Down(np.empty(0, np.uint32)), Down(np.empty(0, np.uint64)), Down(np.empty(0, np.uint32)))
    assert (p.merges, p.pairs) == (q.merges, q.pairs) and p.merges >= 2
    for u, v in zip(p.result(), q.result()):
        assert u.dtype == v.dtype and np.array_equal(u, v)
    want = ([], [], [])
    for l in lists:
        want = M.merge_lists(want, l)
    for u, v in zip(p.result(), want):
        assert np.array_equal(u, v)
