"""Frames: a device array placed at an element offset inside a larger allocation that is otherwise filled with a guard word.

Production callers hand the entry points views of slabs (library/engine.py, library/strand.py, parallel.py), not the first element
of an allocation.  A Frame allocates lead + n + tail elements, fills ALL of them with the guard word of tests/test_gpu_capacity.py
cut to the element size, and puts the payload at element `lead`; `.arr` is the view the entry is called with.  Afterwards
`result(n)` reads the first n elements of the view back and `outside_intact(n)` compares every element of the allocation outside
[lead, lead + n) with the guard: the lead as well as the tail.  Every view lies well inside its allocation, so a kernel that stores
whole 16-, 64- or 128-byte units, rounds a pointer down, or writes a few words in front of its output fails a comparison; it cannot
fault the device.

The placements (element leads; zk_alloc memory is 256-byte aligned, so the lead fixes the address modulo 128):
    P0  the control: lead 0
    P1  natural alignment only: one element (streams that need 16 bytes: 16 bytes)
    P2  the last place before a 128-byte line: u64 lead 15 (address = 120 mod 128), u32 lead 31 (= 124), bytes 127, streams 112
    P3  mixed phases, inputs and outputs on different leads: u64 inputs 1, u64 outputs 3; u32 inputs 2, outputs 6 (both = 8 mod
        16); bytes 7 and 23 (both = 7 mod 16); streams 48

A plain module: the context only has to offer upload(array) -> an object with .view(n, offset) and .to_host(), which
tests/test_frames_host.py stands in for with NumPy."""
import numpy as np

GUARD = 0xABCDABCDABCDABCD          # tests/_core_cases.py
TAIL = 64
BASE_ALIGN = 256                    # zk_alloc (native.py: upload_stream)

PLACEMENTS = ("P0", "P1", "P2", "P3")
KINDS = ("u64", "u32", "byte", "stream16")
ITEMSIZE = {"u64": 8, "u32": 4, "byte": 1, "stream16": 1}

# kind -> placement -> (lead of an input, lead of an output), in elements
LEADS = {
    "u64": {"P0": (0, 0), "P1": (1, 1), "P2": (15, 15), "P3": (1, 3)},
    "u32": {"P0": (0, 0), "P1": (1, 1), "P2": (31, 31), "P3": (2, 6)},
    "byte": {"P0": (0, 0), "P1": (1, 1), "P2": (127, 127), "P3": (7, 23)},
    "stream16": {"P0": (0, 0), "P1": (16, 16), "P2": (112, 112), "P3": (48, 48)},
}


def lead_of(kind, placement, output=False):
    return LEADS[kind][placement][1 if output else 0]


def residue(kind, placement, output=False, modulus=128):
    """the address of the view modulo `modulus`, for a 256-byte aligned allocation"""
    assert BASE_ALIGN % modulus == 0
    return (lead_of(kind, placement, output) * ITEMSIZE[kind]) % modulus


def guard_word(dtype):
    dt = np.dtype(dtype)
    return dt.type(GUARD & ((1 << (8 * dt.itemsize)) - 1))


class Frame:
    """Frame(ctx, host_array, lead, tail=64): the payload at element `lead` of a guarded allocation.  payload=False: an output, the
    whole allocation is guard and host_array only gives the type and the length."""

    def __init__(self, ctx, host_array, lead, tail=TAIL, payload=True):
        a = np.ascontiguousarray(host_array)
        self.lead, self.n, self.tail, self.dtype = int(lead), int(a.size), int(tail), a.dtype
        self.start = np.full(self.lead + self.n + self.tail, guard_word(a.dtype), dtype=a.dtype)
        if payload:
            self.start[self.lead:self.lead + self.n] = a
        self.whole = ctx.upload(self.start)
        self.arr = self.whole.view(self.n, self.lead)

    @classmethod
    def output(cls, ctx, dtype, n, lead, tail=TAIL):
        return cls(ctx, np.empty(int(n), dtype=dtype), lead, tail, payload=False)

    def result(self, n=None):
        n = self.n if n is None else int(n)
        assert 0 <= n <= self.n + self.tail
        return self.whole.to_host()[self.lead:self.lead + n]

    def outside_intact(self, n=None):
        """every element of the allocation outside [lead, lead + n) still holds the guard (n: the payload's length by default)"""
        n = self.n if n is None else int(n)
        got = self.whole.to_host()
        g = guard_word(self.dtype)
        return bool(np.all(got[:self.lead] == g) and np.all(got[self.lead + n:] == g))

    def unchanged(self):
        """the whole allocation, payload and guard, holds what was uploaded"""
        return bool(np.array_equal(self.whole.to_host(), self.start))
