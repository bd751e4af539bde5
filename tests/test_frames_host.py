"""tests/_frames.py checked on the CPU against a NumPy stand-in of the device array (the lead arithmetic, and that outside_intact sees
one changed element on either side of the payload), and once on the GPU: a stray zk_copy into the lead or the tail of a frame,
inside the allocation, must be seen."""
import numpy as np
import pytest

from tests import _frames as F


class HostArray:
    """what _frames needs of native.DeviceArray, over a NumPy array (views share the memory, as device views do)"""

    def __init__(self, mem):
        self.mem, self.dtype, self.n = mem, mem.dtype, len(mem)

    def view(self, n, offset=0):
        assert 0 <= offset and offset + n <= self.n
        return HostArray(self.mem[offset:offset + n])

    def to_host(self):
        return self.mem.copy()


class HostCtx:
    def upload(self, arr):
        return HostArray(np.array(arr, copy=True))


def test_address_residues():
    """the table of the placements, for a 256-byte aligned allocation"""
    assert F.BASE_ALIGN % 128 == 0
    assert [F.residue(k, "P0") for k in F.KINDS] == [0, 0, 0, 0]
    assert [F.residue(k, "P0", True) for k in F.KINDS] == [0, 0, 0, 0]
    # P1: natural alignment only; the streams that need 16 bytes get exactly 16
    assert (F.residue("u64", "P1"), F.residue("u32", "P1"), F.residue("byte", "P1"), F.residue("stream16", "P1")) == (8, 4, 1, 16)
    # P2: the last place before a 128-byte line
    assert (F.residue("u64", "P2"), F.residue("u32", "P2"), F.residue("byte", "P2"), F.residue("stream16", "P2")) == (120, 124, 127, 112)
    for k in ("u64", "u32", "byte"):
        assert F.residue(k, "P2") + F.ITEMSIZE[k] == 128 and F.residue(k, "P2", True) == F.residue(k, "P2")
    # P3: inputs and outputs on different leads
    assert (F.lead_of("u64", "P3"), F.lead_of("u64", "P3", True)) == (1, 3)
    assert F.residue("u32", "P3", modulus=16) == 8 and F.residue("u32", "P3", True, modulus=16) == 8
    assert F.residue("byte", "P3", modulus=16) == 7 and F.residue("byte", "P3", True, modulus=16) == 7
    assert F.residue("stream16", "P3") == 48
    for k in ("u64", "u32", "byte"):
        assert F.lead_of(k, "P3") != F.lead_of(k, "P3", True)
    for k in F.KINDS:
        for p in F.PLACEMENTS:
            for out in (False, True):
                assert F.residue(k, p, out) % F.ITEMSIZE[k] == 0                     # never less than the element's own alignment
                assert F.residue("stream16", p, out, modulus=16) == 0


@pytest.mark.parametrize("dtype", [np.uint64, np.uint32, np.uint8])
@pytest.mark.parametrize("lead", [0, 1, 15, 127])
def test_outside_intact_sees_one_element(dtype, lead):
    ctx = HostCtx()
    data = np.arange(1, 38, dtype=dtype)
    f = F.Frame(ctx, data, lead)
    assert f.arr.n == len(data) and len(f.whole.mem) == lead + len(data) + F.TAIL
    assert np.array_equal(f.result(), data) and f.outside_intact() and f.unchanged()
    assert f.whole.mem[-1] == F.guard_word(dtype) and (lead == 0 or f.whole.mem[0] == F.guard_word(dtype))
    # writes inside the payload, through the view: outside_intact passes, unchanged does not
    f.arr.mem[0] = 99
    f.arr.mem[-1] = 98
    assert f.outside_intact() and not f.unchanged()
    # a result shorter than the array: the elements behind it must still be guard
    o = F.Frame.output(ctx, dtype, 37, lead)
    assert o.outside_intact(0) and o.outside_intact(5)
    o.arr.mem[:5] = 7
    assert o.outside_intact(5) and not o.outside_intact(4)
    o.arr.mem[5] = 7                                    # the first element after the result
    assert not o.outside_intact(5) and o.outside_intact(6)
    # one element just after the payload
    g = F.Frame(ctx, data, lead)
    g.whole.mem[lead + len(data)] ^= 1
    assert not g.outside_intact() and np.array_equal(g.result(), data)
    # one element just before it
    if lead:
        h = F.Frame(ctx, data, lead)
        h.whole.mem[lead - 1] ^= 1
        assert not h.outside_intact() and not h.unchanged() and np.array_equal(h.result(), data)
        h.whole.mem[lead - 1] ^= 1
        h.whole.mem[0] ^= 1                             # ... and the very first one of the allocation
        assert not h.outside_intact()


def test_guard_is_the_capacity_tests_word():
    from tests import _core_cases as cc
    assert F.GUARD == cc.GUARD
    for dt in (np.uint64, np.uint32, np.uint8):
        assert F.guard_word(dt) == cc.guard(1, dt)[0]


def test_every_view_case_builds():
    """the case builders of tests/_view_cases.py touch no device: their own assertions hold and every oracle expectation
    builds on a machine without a GPU; each array of a call has a kind the placements know, each output a capacity that holds it"""
    from tests import _view_cases as V
    names = [n for n, _ in V.CASES]
    assert len(set(names)) == len(names)
    for name, build in V.CASES:
        specs = V.flat(build())
        assert specs, name
        if name.endswith("-tiny"):          # every tiny length is there: no case may drop one quietly
            assert len(specs) >= len(V.TINY), name
        for spec in specs:
            for a in spec.arrays:
                assert a.kind in F.KINDS and a.role in ("in", "out", "io", "scratch", "slab"), name
                if a.role == "out":
                    assert a.cap >= len(a.want), name
                if a.role == "io":
                    assert len(a.want) == len(a.data) and a.want.dtype == a.data.dtype, name
    for entry, (name, which) in V.SIXTEEN.items():
        spec = V.flat(dict(V.CASES)[name]())[0]
        assert all(spec.arrays[i].kind == "stream16" for i in which), entry
    # every array that must be 16-byte aligned somewhere is in the rule's table
    marked = {(n.split("-")[0]) for n, b in V.CASES for sp in V.flat(b()) for a in sp.arrays if a.kind == "stream16"}
    assert marked == {v[0].split("-")[0] for v in V.SIXTEEN.values()}


@pytest.mark.gpu
def test_stray_device_write_is_seen():
    """8 bytes copied onto the last lead word of a frame, or onto its first tail word -- both inside the allocation -- make
    outside_intact fail; a copy into the payload does not"""
    from zotmer_amd import native
    with native.Context(0) as ctx:
        data = np.arange(100, 141, dtype=np.uint64)
        src = ctx.upload(np.array([0x1122334455667788], dtype=np.uint64))
        for where, intact in ((-1, False), (len(data), False), (0, True), (len(data) - 1, True)):
            f = F.Frame(ctx, data, 15)
            assert f.outside_intact() and f.unchanged() and np.array_equal(f.result(), data)
            ctx._check(ctx.lib.zk_copy(ctx.h, f.arr.ptr + 8 * where, src.ptr, 8))
            ctx.sync()
            assert f.outside_intact() is intact, where
            assert not f.unchanged()
