"""The view cases of tests/test_gpu_views.py: what a call's arrays are (Arr, Spec), how they are placed in frames and checked
(run, check), and one builder per entry and variant (CASES).  A plain module: the builders touch no device, so
tests/test_frames_host.py builds every case on a machine without a GPU, and tests/_borrowed_stream_gpu.py runs some of them on a
borrowed stream."""
import ctypes as C
import functools
import random

import numpy as np

from oracle import zkoracle as zo
from tests import _capture_restatement as R
from tests import _contigs_links as CL
from tests import _contigs_restatement as CR
from tests import _core_cases as cc
from tests import _disass_restatement as DR
from tests import _frames as F
from tests import _spectrum_host as H
from tests import _strand_restatement as SR
from zotmer_amd import native, synth

OK, EINVAL = native.ZK_OK, native.ZK_EINVAL
U64, U32, U8 = np.uint64, np.uint32, np.uint8
N = cc.N
M64 = (1 << 64) - 1
TINY = (1, 3, 5)
u64p = C.POINTER(C.c_uint64)

DEFAULT_KNOBS = dict(short_sort=0, side_div=8, early_collapse=1, tile_sort=1, dedupe_bits=0, tag_words=native.DEFAULT_TAG_WORDS,
                     strand_blocks=1, stream_pass=1, packed_pairs=1, wide_tiles=1, kway=1)


def bytes_of(b):
    return np.frombuffer(bytes(b), dtype=U8)


# ---- a call's arrays ---------------------------------------------------------------------------------------------------------------

class Arr:
    """one device array of a call.  role: "in" (must come back unchanged), "out" (want = the oracle's result; cap = the capacity
    the entry is given, the result's length unless stated), "io" (in place: data in, want = what the array holds afterwards, in
    full), "scratch" (an input the entry may destroy: only the guard is checked), "slab" (data = several inputs, views of ONE
    allocation at different phases, as library/engine.py makes them)"""

    def __init__(self, role, kind, data=None, want=None, cap=None, unordered=False):
        self.role, self.kind, self.data, self.want, self.unordered = role, kind, data, want, unordered
        self.cap = cap if cap is not None else (len(want) if want is not None else None)


def In(kind, data): return Arr("in", kind, data=np.ascontiguousarray(data))
def Out(kind, want, cap=None, unordered=False): return Arr("out", kind, want=np.ascontiguousarray(want), cap=cap, unordered=unordered)
def IO(kind, data, want): return Arr("io", kind, data=np.ascontiguousarray(data), want=np.ascontiguousarray(want))
def Scratch(kind, data): return Arr("scratch", kind, data=np.ascontiguousarray(data))
def Slab(kind, datas): return Arr("slab", kind, data=[np.ascontiguousarray(d) for d in datas])


class Spec:
    """arrays: the Arr of a call, in the order `call` receives their views.  call(ctx, views) -> (return code, scalars[, bits]):
    scalars are compared with `scalars` (the oracle's) and with the P0 run, bits with the P0 run only.  knobs: zk_tune settings
    for the call (the defaults are restored afterwards)"""

    def __init__(self, arrays, call, scalars=(), knobs=None):
        self.arrays, self.call, self.scalars, self.knobs = arrays, call, scalars, knobs or {}


class SlabFrame:
    """several inputs in one guarded allocation: the first at the placement's input lead, each later one 3 elements of guard
    behind its predecessor (P0: right behind it), so that their phases differ"""

    def __init__(self, ctx, arr, placement):
        g = F.guard_word(arr.data[0].dtype)
        gap = 0 if placement == "P0" else 3
        parts, at, pos = [np.full(F.lead_of(arr.kind, placement), g, dtype=arr.data[0].dtype)], [], F.lead_of(arr.kind, placement)
        for d in arr.data:
            at.append(pos)
            parts += [d, np.full(gap, g, dtype=d.dtype)]
            pos += len(d) + gap
        parts.append(np.full(F.TAIL, g, dtype=arr.data[0].dtype))
        self.start = np.concatenate(parts)
        self.whole = ctx.upload(self.start)
        self.views = [self.whole.view(len(d), p) for d, p in zip(arr.data, at)]

    def unchanged(self):
        return bool(np.array_equal(self.whole.to_host(), self.start))


def run(ctx, spec, placement):
    """the call with every array at its lead of `placement`, checked against the oracle -> (outputs, scalars, bits)"""
    frames, views = [], []
    for a in spec.arrays:
        if a.role == "slab":
            f = SlabFrame(ctx, a, placement)
            views += f.views
        elif a.role == "out":
            f = F.Frame.output(ctx, a.want.dtype, a.cap, F.lead_of(a.kind, placement, True))
            views.append(f.arr)
        else:
            f = F.Frame(ctx, a.data, F.lead_of(a.kind, placement, a.role == "io"))
            views.append(f.arr)
        frames.append(f)
    try:
        ctx.tune(**spec.knobs)
        r = spec.call(ctx, views)
        ctx.sync()
    finally:
        ctx.tune(**DEFAULT_KNOBS)
    rc, scalars, bits = r[0], r[1], (r[2] if len(r) > 2 else ())
    assert rc == OK, (placement, rc, ctx.lib.zk_last_error(ctx.h))
    assert scalars == spec.scalars, (placement, scalars, spec.scalars)
    outs = []
    for i, (a, f) in enumerate(zip(spec.arrays, frames)):
        where = "array %d (%s, %s) at %s" % (i, a.role, a.kind, placement)
        if a.role in ("in", "slab"):
            assert f.unchanged(), where + ": an input, or the guard around it, was changed"
        elif a.role == "scratch":
            assert f.outside_intact(), where + ": written outside the array"
        elif a.role == "io":
            got = f.result()
            assert f.outside_intact(), where + ": written outside the array"
            assert np.array_equal(got, a.want), where + ": differs from the oracle"
            outs.append(got)
        else:
            got = f.result(len(a.want))
            if a.unordered:
                got = np.sort(got)
            assert np.array_equal(got, a.want), where + ": differs from the oracle"
            # a capacity above the result's length is the entry's work space (zk_capture_hits, zk_kmerize with a subsample)
            assert f.outside_intact(a.cap if a.cap > len(a.want) else len(a.want)), where + ": written outside the result"
            outs.append(got)
    return outs, scalars, bits


_P0 = {}


def check(ctx, name, specs, placement):
    """every Spec of a case at `placement`, and against what the same call gave at P0 on this context (run first, once)"""
    for j, spec in enumerate(specs):
        key = (name, j)
        if key not in _P0:
            _P0[key] = run(ctx, spec, "P0")
        if placement == "P0":
            continue
        outs, scalars, bits = run(ctx, spec, placement)
        outs0, scalars0, bits0 = _P0[key]
        assert scalars == scalars0 and bits == bits0, (placement, j, "differs from the run at P0", bits, bits0)
        for g, g0 in zip(outs, outs0):
            assert np.array_equal(g, g0), (placement, j, "an output differs from the run at P0")


def n_out_call(fn, before, n_outs, after=(), extra=None):
    """call for an entry whose arguments are: ctx, `before` (a function of the views), n_outs output arrays, cap, &n_out,
    `after`; -> (rc, (n_out,) + extra())"""
    def call(ctx, v):
        n = C.c_uint64(0)
        outs = v[len(v) - n_outs:]
        rc = fn(ctx)(ctx.h, *before(v), *[o.ptr for o in outs], outs[0].n, C.byref(n), *after)
        return rc, (n.value,) + (tuple(extra()) if extra else ())
    return call


def acgt_of(keys, weights=None):
    keys = np.asarray(keys, dtype=U64)
    if weights is None:
        return tuple(int(np.sum((keys & U64(3)) == U64(b))) for b in range(4))
    return tuple(int(np.asarray(weights, dtype=U64)[(keys & U64(3)) == U64(b)].sum()) for b in range(4))


CASES = []          # (id, builder): builder() -> Spec or [Spec, ...]; builders touch no device


def case(name):
    def deco(fn):
        CASES.append((name, functools.lru_cache(maxsize=None)(fn)))
        return fn
    return deco


# ---- the list producers ---------------------------------------------------------------------------------------------------------------

def encode_spec(both, t=None):
    if t is None:
        stream, one, two = cc.encode_case()
    else:
        reads = synth.read_strings(70 + t, 0, 1, 24 + t, genome=0)          # t windows of 25 bases
        stream, one, two = cc.stream_of(reads), zo.kmers_list(25, reads[0], False), zo.kmers_list(25, reads[0], True)
        assert len(one) == t
    want = two if both else one
    acgt = (C.c_uint64 * 4)()
    call = n_out_call(lambda c: c.lib.zk_encode, lambda v: (v[0].ptr, v[0].n, 25, both), 1, (acgt,), lambda: list(acgt))
    return Spec([In("stream16", bytes_of(stream)), Out("u64", want)], call, (len(want),) + acgt_of(want))


for _both in (0, 1):
    case("encode-both%d" % _both)(functools.partial(encode_spec, _both))
    case("encode-both%d-tiny" % _both)(lambda _b=_both: [encode_spec(_b, t) for t in TINY])


def subsample_spec(t=None):
    kmers, want = cc.subsample_case()
    if t is not None:
        keep = np.array([zo.sub(5, 4.2, int(x)) for x in kmers[:64]], dtype=bool)
        m = head_before(keep, t + 1)          # (up to the next k-mer kept: the rejected ones behind the t-th are in)
        kmers, want = kmers[:m], kmers[:m][keep[:m]]
        assert len(want) == t
    call = n_out_call(lambda c: c.lib.zk_subsample, lambda v: (v[0].ptr, v[0].n, 5, 4.2), 1)
    return Spec([In("u64", kmers), Out("u64", want)], call, (len(want),))


case("subsample")(subsample_spec)
case("subsample-tiny")(lambda: [subsample_spec(t) for t in TINY])


def rle_spec(in_place, t=None):
    keys, vals, cnt = cc.rle_case()
    if t is not None:
        vals, cnt = vals[:t], cnt[:t]
        keys = np.repeat(vals, cnt)
    if in_place:
        def call(ctx, v):
            n = C.c_uint64(0)
            rc = ctx.lib.zk_rle(ctx.h, v[0].ptr, v[0].n, v[0].ptr, v[1].ptr, v[1].n, C.byref(n))
            return rc, (n.value,)
        # d_uniq == d_sorted: behind the distinct values the array still holds its input (cap = the length needed)
        return Spec([IO("u64", keys, np.concatenate([vals, keys[len(vals):]])), Out("u32", cnt)], call, (len(vals),))
    call = n_out_call(lambda c: c.lib.zk_rle, lambda v: (v[0].ptr, v[0].n), 2)
    return Spec([In("u64", keys), Out("u64", vals), Out("u32", cnt)], call, (len(vals),))


for _ip in (False, True):
    case("rle-%s" % ("in_place" if _ip else "apart"))(functools.partial(rle_spec, _ip))
    case("rle-%s-tiny" % ("in_place" if _ip else "apart"))(lambda _i=_ip: [rle_spec(_i, t) for t in TINY])


def sort_count_spec(t=None):
    keys, vals, cnt = cc.rle_case()
    if t is not None:
        vals, cnt = vals[:t], cnt[:t]
        keys = np.repeat(vals, cnt)
    shuffled = np.random.default_rng(48).permutation(keys)
    call = n_out_call(lambda c: c.lib.zk_sort_count, lambda v: (v[0].ptr, v[0].n, 40), 2)
    return Spec([Scratch("u64", shuffled), Out("u64", vals), Out("u32", cnt)], call, (len(vals),))          # (the sort destroys d_keys)


case("sort_count")(sort_count_spec)
case("sort_count-tiny")(lambda: [sort_count_spec(t) for t in TINY])


def mirror_spec(K, packed, size=None):
    c, n, keys, cnt, _ = cc.mirror_case(K, size)
    assert size is None or size < GROUPED or len(c) >= GROUPED
    assert size is None or size >= GROUPED or len(keys) == (2 * size if K & 1 else 2 * size - 1)
    call = n_out_call(lambda x: x.lib.zk_mirror_expand, lambda v: (v[0].ptr, v[1].ptr, v[0].n, K), 2)
    return Spec([In("u64", c), In("u32", n), Out("u64", keys), Out("u32", cnt)], call, (len(keys),), knobs=dict(packed_pairs=packed))


GROUPED = 65536 + 5          # pipeline.hip: from 65 536 canonical entries on the mirrored words are grouped, not sorted
for _K in (25, 24):
    for _pk in (0, 1):
        case("mirror_expand-K%d-packed%d" % (_K, _pk))(functools.partial(mirror_spec, _K, _pk))
        # odd K: two entries per k-mer, 2, 6 and 10; even K: a palindrome and 0, 1 and 2 others, 1, 3 and 5
        case("mirror_expand-K%d-packed%d-tiny" % (_K, _pk))(lambda _a=_K, _b=_pk: [mirror_spec(_a, _b, t if _a & 1 else t // 2 + 1) for t in TINY])
        case("mirror_expand-K%d-packed%d-grouped" % (_K, _pk))(functools.partial(mirror_spec, _K, _pk, GROUPED + 8))


def union_spec(cdt, t=None):
    x, xc, y, yc, zs, zc = cc.union_case()
    if t is not None:          # t keys in the union: the first shared, then one list's, then the other's
        pool = zs[:t]
        inx, iny = np.arange(t) % 3 != 2, np.arange(t) % 3 != 1
        x, y = pool[inx], pool[iny]
        xc, yc = np.arange(1, len(x) + 1, dtype=U64) * U64(7), np.arange(1, len(y) + 1, dtype=U64) * U64(1000)
        zs, zc = zo.union_sum(x, xc, y, yc)
        assert len(zs) == t
    bits = 8 * np.dtype(cdt).itemsize
    acgt = (C.c_uint64 * 4)()

    def call(ctx, v):          # views: xk, yk (one slab), xc, yc (one slab), ok, oc
        n = C.c_uint64(0)
        rc = ctx.lib.zk_union_sum(ctx.h, v[0].ptr, v[2].ptr, v[0].n, v[1].ptr, v[3].ptr, v[1].n, v[4].ptr, v[5].ptr, bits, v[4].n,
                                  C.byref(n), acgt)
        return rc, (n.value,) + tuple(acgt)
    ck = "u32" if bits == 32 else "u64"
    return Spec([Slab("u64", [x, y]), Slab(ck, [xc.astype(cdt), yc.astype(cdt)]), Out("u64", zs), Out(ck, zc.astype(cdt))], call,
                (len(zs),) + acgt_of(zs, zc))


for _cdt in (np.uint32, np.uint64):
    case("union_sum-%s" % np.dtype(_cdt).name)(functools.partial(union_spec, _cdt))
    case("union_sum-%s-tiny" % np.dtype(_cdt).name)(lambda _c=_cdt: [union_spec(_c, t) for t in TINY])


def merge_spec(k, kway, t=None):
    if t is None:
        sets, zs, zc, acgt = cc.merge_case(k)
    else:          # every key in every list (k = 2)
        pool = cc.merge_case(2)[1][:t]
        sets = [(pool, np.arange(1, t + 1, dtype=U64) * U64(3 + i)) for i in range(k)]
        zs, zc, acgt = zo.merge_n(25, sets)
        assert len(zs) == t

    def call(ctx, v):
        pk = (C.c_void_p * k)(*[a.ptr for a in v[0:2 * k:2]])
        pc = (C.c_void_p * k)(*[a.ptr for a in v[1:2 * k:2]])
        ns = (C.c_uint64 * k)(*[a.n for a in v[0:2 * k:2]])
        n, got = C.c_uint64(0), (C.c_uint64 * 4)()
        rc = ctx.lib.zk_merge_n(ctx.h, k, pk, pc, ns, v[2 * k].ptr, v[2 * k + 1].ptr, 64, v[2 * k].n, C.byref(n), got)
        return rc, (n.value,) + tuple(got)
    arrays = []
    for a, b in sets:
        arrays += [In("u64", a), In("u64", b)]
    return Spec(arrays + [Out("u64", zs), Out("u64", zc)], call, (len(zs),) + tuple(int(a) for a in acgt), knobs=dict(kway=kway))


for _k in (2, 3, 5, 17):
    for _kw in (0, 2):
        case("merge_n-k%d-kway%d" % (_k, _kw))(functools.partial(merge_spec, _k, _kw))
for _kw in (0, 2):
    case("merge_n-k2-kway%d-tiny" % _kw)(lambda _w=_kw: [merge_spec(2, _w, t) for t in TINY])


def project_spec(t=None):
    ref, k, c, ek, ec = cc.project_case()
    if t is not None:          # the set's first k-mers up to the one before the (t + 1)-th that is in the reference
        m = head_before(np.isin(k, ref), t + 1)
        k, c = k[:m], c[:m]
        ek, ec = zo.project(ref, k, c)
        assert len(ek) == t
    call = n_out_call(lambda x: x.lib.zk_project, lambda v: (v[0].ptr, v[0].n, v[1].ptr, v[2].ptr, v[1].n), 2)
    return Spec([In("u64", ref), In("u64", k), In("u64", c), Out("u64", ek), Out("u64", ec)], call, (len(ek),))


case("project")(project_spec)
case("project-tiny")(lambda: [project_spec(t) for t in TINY])


def head_with(keep, t):
    """the length of the shortest prefix with t kept entries"""
    return int(np.flatnonzero(np.cumsum(keep) == t)[0]) + 1


def head_before(keep, t):
    """the length of the longest prefix with fewer than t kept entries"""
    return int(np.flatnonzero(np.cumsum(keep) == t)[0])


def sample_spec(t=None):
    k, c = cc.counted_case()
    ek, ec = zo.sample_d(0.5, 11, k, c)
    if t is not None:
        m = head_with(np.isin(k[:64], ek), t)
        k, c = k[:m], c[:m]
        ek, ec = zo.sample_d(0.5, 11, k, c)
        assert len(ek) == t
    call = n_out_call(lambda x: x.lib.zk_sample, lambda v: (v[0].ptr, v[1].ptr, v[0].n, 11, 0.5), 2)
    return Spec([In("u64", k), In("u64", c), Out("u64", ek), Out("u64", ec)], call, (len(ek),))


case("sample")(sample_spec)
case("sample-tiny")(lambda: [sample_spec(t) for t in TINY])


def project_dedupe_spec(shift, t=None):
    k, _ = cc.prefix_case()
    if t is not None:
        k = k[:head_with(np.concatenate([[True], (k[1:64] >> U64(shift)) != (k[:63] >> U64(shift))]), t)]
    want = zo.project_dedupe(k, shift)
    assert t is None or len(want) == t
    call = n_out_call(lambda x: x.lib.zk_project_dedupe, lambda v: (v[0].ptr, v[0].n, shift), 1)
    return Spec([In("u64", k), Out("u64", want)], call, (len(want),))


for _s in (0, 20):
    case("project_dedupe-shift%d" % _s)(functools.partial(project_dedupe_spec, _s))
    case("project_dedupe-shift%d-tiny" % _s)(lambda _x=_s: [project_dedupe_spec(_x, t) for t in TINY])


def trim_spec(cdt, t=None):
    k, c = cc.counted_case()
    if t is not None:
        m = head_with((c[:64] >= 3) & (c[:64] <= 7), t)
        k, c = k[:m], c[:m]
    ek, ec = zo.trim(k, c, 3, 7)
    assert t is None or len(ek) == t
    bits = 8 * np.dtype(cdt).itemsize
    ck = "u32" if bits == 32 else "u64"
    call = n_out_call(lambda x: x.lib.zk_trim, lambda v: (v[0].ptr, v[1].ptr, bits, v[0].n, 3, 7), 2)
    return Spec([In("u64", k), In(ck, c.astype(cdt)), Out("u64", ek), Out(ck, ec.astype(cdt))], call, (len(ek),))


def project_sum_spec(cdt, shift, t=None):
    k, c = cc.prefix_case()
    if t is not None:
        k = k[:head_with(np.concatenate([[True], (k[1:64] >> U64(shift)) != (k[:63] >> U64(shift))]), t)]
        c = c[:len(k)]
    wk, ws, wt = H.host_project_sum(k, c.astype(cdt), shift)
    assert t is None or len(wk) == t
    bits = 8 * np.dtype(cdt).itemsize
    total = C.c_uint64(0)
    call = n_out_call(lambda x: x.lib.zk_project_sum, lambda v: (v[0].ptr, v[1].ptr, bits, v[0].n, shift), 2, (C.byref(total),),
                      lambda: [total.value])
    return Spec([In("u64", k), In("u32" if bits == 32 else "u64", c.astype(cdt)), Out("u64", np.asarray(wk, dtype=U64)),
                 Out("u64", np.asarray(ws, dtype=U64))], call, (len(wk), int(wt)))


for _cdt in (np.uint32, np.uint64):
    _nm = np.dtype(_cdt).name
    case("trim-%s" % _nm)(functools.partial(trim_spec, _cdt))
    case("trim-%s-tiny" % _nm)(lambda _c=_cdt: [trim_spec(_c, t) for t in TINY])
    for _s in (0, 20):
        case("project_sum-%s-shift%d" % (_nm, _s))(functools.partial(project_sum_spec, _cdt, _s))
        case("project_sum-%s-shift%d-tiny" % (_nm, _s))(lambda _c=_cdt, _x=_s: [project_sum_spec(_c, _x, t) for t in TINY])


# ---- the device codec ----------------------------------------------------------------------------------------------------------------

def codec_encode_spec(form, t=None):
    v, w, v32, w32, k, wk = cc.codec_case()
    if form == "u32":
        vals = v32 if t is None else v32[:words_head(v32.astype(U64), t)]
        want = zo.codec64_encode(vals.astype(U64))
        call = n_out_call(lambda x: x.lib.zk_codec64_encode_u32_dev, lambda a: (a[0].ptr, a[0].n), 1)
        return Spec([In("u32", vals), Out("u64", want)], call, (len(want),))
    delta = int(form == "delta")
    src = k if delta else v
    vals = src if t is None else src[:words_head(zo.delta(src) if delta else src, t)]
    want = zo.codec64_encode(zo.delta(vals) if delta else vals)
    assert t is None or len(want) == t
    call = n_out_call(lambda x: x.lib.zk_codec64_encode_dev, lambda a: (a[0].ptr, a[0].n, delta), 1)
    return Spec([In("u64", vals), Out("u64", want)], call, (len(want),))


def words_head(vals, t):
    """the longest prefix of at most 64 values that encodes to t words"""
    best = None
    for m in range(1, 65):
        if len(zo.codec64_encode(vals[:m])) == t:
            best = m
    assert best is not None
    return best


def codec_decode_spec(delta, t=None):
    v, w, _, _, k, wk = cc.codec_case()
    vals = k if delta else v
    if t is not None:
        vals = vals[:t]
    words = zo.codec64_encode(zo.delta(vals) if delta else vals)
    call = n_out_call(lambda x: x.lib.zk_codec64_decode_dev, lambda a: (a[0].ptr, a[0].n, delta), 1)
    return Spec([In("u64", words), Out("u64", vals)], call, (len(vals),))


for _f in ("u64", "delta", "u32"):
    case("codec_encode-%s" % _f)(functools.partial(codec_encode_spec, _f))
    case("codec_encode-%s-tiny" % _f)(lambda _x=_f: [codec_encode_spec(_x, t) for t in TINY])
for _d in (0, 1):
    case("codec_decode-delta%d" % _d)(functools.partial(codec_decode_spec, _d))
    case("codec_decode-delta%d-tiny" % _d)(lambda _x=_d: [codec_decode_spec(_x, t) for t in TINY])


# ---- the text kernels of `zot capture` -----------------------------------------------------------------------------------------------

def line_ends_of(text):
    return np.flatnonzero(bytes_of(text) == 10).astype(U64)


def line_ends_spec(t=None):
    text = cc.capture_case()[0]
    if t is not None:
        text = text[:int(line_ends_of(text)[t - 1]) + 1 + 2]          # t lines and two bytes of the next
    want = line_ends_of(text)
    call = n_out_call(lambda x: x.lib.zk_line_ends, lambda v: (v[0].ptr, v[0].n), 1)
    return Spec([In("byte", bytes_of(text)), Out("u64", want)], call, (len(want),))


case("line_ends")(line_ends_spec)
case("line_ends-tiny")(lambda: [line_ends_spec(t) for t in TINY])


class Held:
    """a bait table built once per context (not framed: the table's memory is its own)"""

    def __init__(self):
        self.key, self.table = None, None

    def get(self, ctx, baits):
        if self.key != id(ctx):
            self.put(ctx, ctx.bait_table(ctx.upload_stream(cc.stream_of(baits)), R.READ_K))
        return self.table

    def put(self, ctx, table):
        """the table to use on this context (None: forget it)"""
        self.table, self.key = table, (id(ctx) if table is not None else None)


_capture_table = Held()


@case("capture_hits")
def capture_hits_spec():
    """the capacity is that of the pairs before deduplication, the work space of the entry: the guard is checked from there"""
    text, baits, pairs, raw, _, _ = cc.capture_case()

    def call(ctx, v):
        n = C.c_uint64(0)
        table = _capture_table.get(ctx, baits)
        rc = ctx.lib.zk_capture_hits(ctx.h, table.h, None, R.READ_K, v[0].ptr, v[1].ptr, None, None, 400, v[2].ptr, v[2].n, C.byref(n))
        return rc, (n.value,)
    return Spec([In("byte", bytes_of(text)), In("u64", line_ends_of(text)), Out("u64", pairs, cap=raw)], call, (len(pairs),))


@case("capture_hits-tiny")
def capture_hits_tiny():
    """the first reads of the same text (n_reads) that give 1, 3 and 5 pairs, in a work space for the pairs of all reads"""
    text, baits, pairs, raw, _, _ = cc.capture_case()
    out = []
    for size in TINY:
        t = next(r for r in range(1, 400) if int(np.count_nonzero((pairs & U64(0xFFFFFFFF)) < U64(r))) == size)

        def call(ctx, v, _t=t):
            n = C.c_uint64(0)
            table = _capture_table.get(ctx, baits)
            rc = ctx.lib.zk_capture_hits(ctx.h, table.h, None, R.READ_K, v[0].ptr, v[1].ptr, None, None, _t, v[2].ptr, v[2].n, C.byref(n))
            return rc, (n.value,)
        want = pairs[(pairs & U64(0xFFFFFFFF)) < U64(t)]
        assert len(want) == size
        out.append(Spec([In("byte", bytes_of(text)), In("u64", line_ends_of(text)), Out("u64", want, cap=raw)], call, (len(want),)))
    return out


def bait_build_spec(t=None):
    """zk_bait_table_build reads its stream byte by byte: the table's own arrays against the dict of capture.py:85-95"""
    K = R.READ_K
    baits = cc.capture_case()[1]
    seqs = baits if t is None else [baits[0][:K - 1 + t]]          # t windows
    table = {}
    for b, seq in enumerate(seqs):
        for x in R.kmers(K, seq, True):
            table.setdefault(x, set()).add(b)
    keys = np.array(sorted(table), dtype=U64)
    lists = [sorted(table[int(x)]) for x in keys]
    offs = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(U32)
    ids = np.concatenate(lists).astype(U32)

    def call(ctx, v):
        h = C.c_void_p()
        rc = ctx.lib.zk_bait_table_build(ctx.h, v[0].ptr, v[0].n, K, C.byref(h))
        if rc != OK:
            return rc, ()
        tb = native.BaitTable(ctx, h.value, K)
        got = tuple(a.to_host().tobytes() for a in tb.arrays())
        tb.free()
        return rc, (tb.n_keys, tb.n_ids, tb.n_records) + got
    return Spec([In("byte", bytes_of(cc.stream_of(seqs)))], call, (len(keys), len(ids), len(seqs), keys.tobytes(), offs.tobytes(), ids.tobytes()))


case("bait_table_build")(bait_build_spec)
case("bait_table_build-tiny")(lambda: [bait_build_spec(t) for t in TINY])


def capture_gather_spec(t=None):
    text, baits, pairs, _, gathered, _ = cc.capture_case()
    if t is not None:
        pairs = pairs[:t]
        recs = R.fastq_records(text.decode())
        gathered = "".join("%s\n%s\n%s\n%s\n" % recs[int(w) & 0xFFFFFFFF] for w in pairs).encode()
    want = bytes_of(gathered)
    nb = len(baits)
    bait_of = (pairs >> U64(32)).astype(np.int64)
    spans = np.zeros(2 * (nb + 1), dtype=U64)

    def call(ctx, v):
        n = C.c_uint64(0)
        rc = ctx.lib.zk_capture_gather(ctx.h, v[0].ptr, v[0].n, nb, v[1].ptr, v[2].ptr, v[2].n, v[3].ptr, v[3].n,
                                       spans.ctypes.data_as(u64p), C.byref(n))
        return rc, (n.value, tuple(int(s) for s in spans[:nb + 1]), int(spans[-1]))
    return Spec([In("u64", pairs), In("byte", bytes_of(text)), In("u64", line_ends_of(text)), Out("byte", want)], call,
                (len(want), tuple(int(np.searchsorted(bait_of, b)) for b in range(nb + 1)), len(want)))


case("capture_gather")(capture_gather_spec)
case("capture_gather-tiny")(lambda: [capture_gather_spec(t) for t in TINY])


# ---- `zot strand` -------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def strand_case():
    """FASTQ text of 300 reads of 80 to 150 bases from a genome of 9000, either strand; a third of the windows kept"""
    rng = random.Random(91)
    genome = "".join(rng.choice("ACGT") for _ in range(9000))
    comp = str.maketrans("ACGT", "TGCA")
    seqs = []
    for _ in range(300):
        n = rng.choice((80, 100, 150))
        p = rng.randrange(0, len(genome) - n)
        s = genome[p:p + n]
        if rng.random() < 0.5:
            s = s[::-1].translate(comp)
        if rng.random() < 0.1:
            q = rng.randrange(n)
            s = s[:q] + "N" + s[q + 1:]
        seqs.append(s)
    text = "".join("@r%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(seqs)).encode()
    return seqs, text


def strand_keys_spec(reverse, t=None):
    K = 21
    seqs, text = strand_case()
    T = SR.threshold(K, 0.34)[1]
    if t is not None:
        T = (1 << (2 * K)) - 1                          # every window kept: a read of K - 1 + t bases has t
        seqs = [seqs[0][:K - 1 + t]]
        text = ("@r\n%s\n+\n%s\n" % (seqs[0], "I" * len(seqs[0]))).encode()
    want = np.array(SR.tagged_keys(K, seqs, reverse, T), dtype=U64)
    assert len(want) == t if t is not None else len(want) > 2000
    call = n_out_call(lambda x: x.lib.zk_strand_keys, lambda v: (v[0].ptr, v[1].ptr, len(seqs), K, reverse, SR.SEED, T), 1)
    return Spec([In("byte", bytes_of(text)), In("u64", line_ends_of(text)), Out("u64", want, unordered=True)], call, (len(want),))


for _r in (0, 1):
    case("strand_keys-reverse%d" % _r)(functools.partial(strand_keys_spec, _r))
    case("strand_keys-reverse%d-tiny" % _r)(lambda _x=_r: [strand_keys_spec(_x, t) for t in TINY])


def strand_pairs_spec(cdt, orphans, t=None):
    K = 21
    seqs, _ = strand_case()
    T = SR.threshold(K, 0.34)[1]
    both = SR.tagged_keys(K, seqs[:150], 0, T) + SR.tagged_keys(K, seqs[150:], 1, T)
    keys, counts = np.unique(np.array(both, dtype=U64), return_counts=True)
    if t is not None:
        for m in range(1, 64):
            if len(SR.pairs_of(K, keys[:m], counts[:m], orphans)[0]) == t:
                break
        keys, counts = keys[:m], counts[:m]
    a, b, st = SR.pairs_of(K, keys, counts, orphans)
    assert len(a) == t if t is not None else len(a) > 1000
    bits = 8 * np.dtype(cdt).itemsize
    stats = native.StrandStats()

    def call(ctx, v):
        rc = ctx.lib.zk_strand_pairs(ctx.h, v[0].ptr, v[1].ptr, bits, v[0].n, K, SR.SEED, native.STRAND_ORPHANS if orphans else 0,
                                     v[2].ptr, v[3].ptr, v[2].n, C.byref(stats))
        return rc, (stats.n_pairs,)
    return Spec([In("u64", keys), In("u32" if bits == 32 else "u64", counts.astype(cdt)), Out("u64", np.array(a, dtype=U64)),
                 Out("u64", np.array(b, dtype=U64))], call, (len(a),))


for _cdt in (np.uint32, np.uint64):
    for _o in (False, True):
        _nm = "strand_pairs-%s-orphans%d" % (np.dtype(_cdt).name, _o)
        case(_nm)(functools.partial(strand_pairs_spec, _cdt, _o))
        case(_nm + "-tiny")(lambda _c=_cdt, _x=_o: [strand_pairs_spec(_c, _x, t) for t in TINY])


def format_pairs_spec(t=None):
    """library/strand.py formats a.view(m, lo): values of every decimal length"""
    rng = np.random.default_rng(92)
    n = 9000 if t is None else 1
    a = (rng.integers(0, 1 << 63, size=n, dtype=U64) * U64(2) + U64(1)) >> rng.integers(0, 64, size=n).astype(U64)
    b = rng.integers(0, 1 << 63, size=n, dtype=U64) >> rng.integers(0, 63, size=n).astype(U64)
    if t is not None:          # one pair: a line of 4, 6 and 8 bytes
        a, b = np.array([{1: 7, 3: 12, 5: 123}[t]], dtype=U64), np.array([{1: 0, 3: 45, 5: 678}[t]], dtype=U64)
    want = bytes_of("".join("%d\t%d\n" % (int(x), int(y)) for x, y in zip(a, b)).encode())
    call = n_out_call(lambda x: x.lib.zk_format_pairs, lambda v: (v[0].ptr, v[1].ptr, v[0].n), 1)
    return Spec([In("u64", a), In("u64", b), Out("byte", want)], call, (len(want),))


case("format_pairs")(format_pairs_spec)
case("format_pairs-tiny")(lambda: [format_pairs_spec(t) for t in TINY])


# ---- `zot disass`, `zot vars`, `zot contigs` -------------------------------------------------------------------------------------------

def dr_rc(K, x):
    y = 0
    for _ in range(K):
        y = (y << 2) | (3 - (x & 3))
        x >>= 2
    return y


def contig_spectra_spec(both, t=None):
    """all four outputs framed; the brute force of tests/test_gpu_disass.py: the reference's dict per record, the counted key list"""
    K, seed, p = 16, 17, (0.7 if t is None else 9.0)          # (the hash over 2^61 - 1 is below 8; tiny: every key kept, the record has its bin)
    rng = random.Random(93)
    genome = "".join(rng.choice("ACGT") for _ in range(900))
    if t is None:
        recs = []
        for _ in range(70):
            L = rng.randrange(20, 300)
            q = rng.randrange(0, len(genome) - L)
            recs.append(genome[q:q + L] if rng.random() < 0.9 else genome[q:q + L // 2] + "N" + genome[q + L // 2:q + L])
    else:
        recs = [genome[:K - 1 + t]]
    stream = ("\n".join(recs) + "\n").encode()
    words, keys, n_windows = [], {}, 0
    for r, seq in enumerate(recs):
        d = {}
        for x in DR.kmers_list(K, seq, bool(both)):
            if DR.sub(seed, p, x):
                d[x] = d.get(x, 0) + 1
        for x in DR.kmers_list(K, seq, False):
            k = min(x, dr_rc(K, x)) if both else x
            keys[k] = keys.get(k, 0) + 1
            n_windows += 1
        h = {}
        for c in d.values():
            h[c] = h.get(c, 0) + 1
        words += [((r << 32) | c, f) for c, f in sorted(h.items())]
    key_list = sorted(keys.items())
    assert t is None or len(key_list) == t
    st = native.ContigStats()

    def call(ctx, v):
        rc = ctx.lib.zk_contig_spectra(ctx.h, v[0].ptr, v[0].n, K, both, seed, p, v[1].ptr, v[2].ptr, v[1].n, v[3].ptr, v[4].ptr, v[3].n,
                                       C.byref(st))
        return rc, (st.n_records, st.n_windows, st.n_keys, st.n_bins)
    assert words and (t is None or len(words) == 1)
    return Spec([In("byte", bytes_of(stream)), Out("u64", np.array([w for w, _ in words], dtype=U64)),
                 Out("u64", np.array([f for _, f in words], dtype=U64)), Out("u64", np.array([k for k, _ in key_list], dtype=U64)),
                 Out("u32", np.array([c for _, c in key_list], dtype=U32))], call, (len(recs), n_windows, len(key_list), len(words)))


for _b in (0, 1):
    case("contig_spectra-both%d" % _b)(functools.partial(contig_spectra_spec, _b))
    case("contig_spectra-both%d-tiny" % _b)(lambda _x=_b: [contig_spectra_spec(_x, t) for t in TINY])


def vars_lists(n_ctx, seed=94):
    """(reference list, sample list): groups of every size on both sides, some sample contexts the reference lacks; sample counts
    far from the reference's shares, so that most joined groups are rows and none lies near the threshold"""
    K = 13
    rng = random.Random(seed)
    ctxs = sorted(rng.sample(range(1 << (2 * (K - 1))), n_ctx))
    ref, sam = [], []
    for c in ctxs:
        bases = sorted(rng.sample(range(4), rng.randint(2, 4)))
        if rng.random() < 0.9:
            for j, b in enumerate(bases):
                ref.append(((c << 2) | b, 1 if j else 4000))
        enriched = rng.random() < 0.6
        for j, b in enumerate(bases):
            sam.append(((c << 2) | b, (3000 if j else 5) if enriched else (1 if j else 4000)))
    return K, ref, sam


def vars_scan_spec(rbits, sbits, t=None):
    from zotmer_amd.library import varscan
    thr = -10.0
    K, ref, sam = vars_lists(3000 if t is None else 24)

    def groups(pairs):
        g, n = {}, {}
        for x, c in pairs:
            g.setdefault(x >> 2, [0, 0, 0, 0])[x & 3] = c
            n[x >> 2] = n.get(x >> 2, 0) + 1
        return g, n

    def brute(guards):
        rg, rn = groups(ref)
        sg, _ = groups(sam)
        rows, missing, mixed = [], [], 0
        for c in sorted(sg):
            if c not in rg:
                missing.append(c)
            elif rn[c] >= 2:
                mixed += 1
                st_, gt = sum(sg[c]), sum(rg[c])
                if any(varscan.candidate(sg[c][j], st_, rg[c][j], gt, thr, guards) for j in range(4)):
                    rows.append((c, sg[c], rg[c]))
        return rows, (len(sg), len(missing), missing[0] if missing else 0, mixed)
    if t is not None:          # cut the sample behind the group that makes the t-th row
        rows, _ = brute(0.0)
        last = rows[t - 1][0]
        sam = [(x, c) for x, c in sam if (x >> 2) <= last]
    rows, stats = brute(0.0)
    assert rows == brute(2.0)[0], "the data has a base inside the guard band"
    assert len(rows) == t if t is not None else len(rows) > 1000
    dt = {32: np.uint32, 64: np.uint64}
    st = native.VarsStats()

    def call(ctx, v):
        rc = ctx.lib.zk_vars_scan(ctx.h, v[0].ptr, v[1].ptr, rbits, v[0].n, v[2].ptr, v[3].ptr, sbits, v[2].n, K, thr, v[4].ptr, v[5].ptr,
                                  v[4].n, C.byref(st))
        return rc, (st.n_groups, st.n_missing, st.first_missing, st.n_mixed, st.n_rows)
    want_rows = np.array([list(sx) + list(gx) for _, sx, gx in rows], dtype=U64).reshape(-1)
    return Spec([In("u64", np.array([x for x, _ in ref], dtype=U64)), In("u%d" % rbits, np.array([c for _, c in ref], dtype=dt[rbits])),
                 In("u64", np.array([x for x, _ in sam], dtype=U64)), In("u%d" % sbits, np.array([c for _, c in sam], dtype=dt[sbits])),
                 Out("u64", np.array([c for c, _, _ in rows], dtype=U64)), Out("u64", want_rows)], call,
                stats + (len(rows),))


case("vars_scan-ref32-sam64")(functools.partial(vars_scan_spec, 32, 64))
case("vars_scan-ref64-sam32")(functools.partial(vars_scan_spec, 64, 32))
case("vars_scan-tiny")(lambda: [vars_scan_spec(32, 32, t) for t in TINY])


@functools.lru_cache(maxsize=None)
def contig_set(K, n_genome, seed):
    """the ascending k-mers of both strands of a random genome"""
    return np.array(sorted(set(CR.kmers_of(K, genome_of(n_genome, seed), True))), dtype=U64)


def genome_of(n, seed):
    rng = random.Random(seed)
    return "".join(rng.choice("ACGT") for _ in range(n))


def contig_render_spec(t=None):
    """tiny: the set of both strands of one sequence of K - 1 + t bases and one contig of t nodes (a contig's text is never
    shorter than its header and K bases)"""
    K = 15
    if t is None:
        xs = contig_set(K, 9000, 95)
        nxt, rank = CL.np_links(K, xs)
        nodes, offs = CR.walk_links([int(v) for v in nxt], [int(v) for v in rank], K, 0)
    else:          # the forward strand's t k-mers in order, as one contig (the entry takes any paths, not only the walk's)
        xs = contig_set(K, K - 1 + t, 96)
        nodes = [int(np.searchsorted(xs, U64(x))) for x in CR.kmers_of(K, genome_of(K - 1 + t, 96), False)]
        offs = [0, t]
        assert len(xs) == 2 * t and len(nodes) == t
    paths = [nodes[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]
    want = bytes_of(CR.text_of(K, [int(x) for x in xs], paths).encode())
    call = n_out_call(lambda x: x.lib.zk_contig_render, lambda v: (v[0].ptr, v[0].n, K, v[1].ptr, v[1].n, v[2].ptr, v[2].n - 1), 1)
    return Spec([In("u64", xs), In("u32", np.array(nodes, dtype=U32)), In("u64", np.array(offs, dtype=U64)), Out("byte", want)], call,
                (len(want),))


case("contig_render")(contig_render_spec)
case("contig_render-tiny")(lambda: [contig_render_spec(t) for t in TINY])


# ---- zk_kmerize: the routes the earlier tests reach at small sizes ------------------------------------------------------------------------

FLAGS = {"canonical": native.KMERIZE_CANONICAL, "both": native.KMERIZE_BOTH, "canonical_only": native.KMERIZE_CANONICAL_ONLY,
         "subsample": native.KMERIZE_CANONICAL | native.KMERIZE_SUBSAMPLE}

KMERIZE_CASES = [("deep", 25, f, {}) for f in ("canonical", "both", "canonical_only", "subsample")]          # the default plan
KMERIZE_CASES += [("flat", 25, "canonical", {})]
# the block dedupe forced: at odd K the strands are rebuilt block by block, "to a place known in advance" (strand_blocks 1), or by
# the merge-path union (0); at even K by the union of two packed lists
KMERIZE_CASES += [("deep", 25, "canonical", dict(dedupe_bits=18, strand_blocks=s)) for s in (1, 0)]
KMERIZE_CASES += [("deep", 25, "canonical_only", dict(dedupe_bits=18)), ("deep", 24, "canonical", dict(dedupe_bits=18))]
# reads that do not repeat at K = 31: the tile sort counts straight into the caller's arrays; else the passes over every bit
KMERIZE_CASES += [("flat", 31, f, dict(tile_sort=s)) for s in (1, 0) for f in ("canonical", "canonical_only")]
# pass 0: static stream ranges with 128-byte units (1, the default above), with 64-byte units, the look-back pipeline
KMERIZE_CASES += [("deep", 25, "canonical", dict(stream_pass=s)) for s in (0, 2)]
KMERIZE_CASES += [("flat", 31, "canonical", dict(stream_pass=s)) for s in (0, 2)]
KMERIZE_CASES += [("deep", 25, "canonical", dict(early_collapse=e)) for e in (0, 2)]
KMERIZE_CASES += [("deep", 25, "canonical", dict(packed_pairs=0)), ("deep", 24, "canonical", dict(packed_pairs=0))]


def facts_of(reads, K):
    """(valid windows, acgt[x & 3] over every instance of both strands)"""
    both = np.concatenate([zo.kmers_list(K, r, True) for r in reads])
    return len(both) // 2, acgt_of(both)


@functools.lru_cache(maxsize=None)
def stream_facts(inp, K):
    return facts_of(cc.kmerize_reads(inp, K), K)


def kmerize_spec(inp, K, flags, knobs, reads=None):
    if reads is None:
        wk, wc, needed = cc.kmerize_want(inp, K, flags)
        reads = cc.kmerize_reads(inp, K)
        windows, acgt = stream_facts(inp, K)
    else:
        full = zo.kmerize(K, reads)
        wk, wc, needed = full["kmers"], full["counts"], len(full["kmers"])
        windows, acgt = facts_of(tuple(reads), K)
    stream = cc.stream_of(reads)
    st = native.KmerizeStats()

    def call(ctx, v):
        rc = ctx.lib.zk_kmerize(ctx.h, v[0].ptr, v[0].n, K, FLAGS[flags], 0.5, 3, v[1].ptr, v[2].ptr, v[1].n, C.byref(st))
        return rc, (st.n_windows, st.n_instances, st.n_unique, tuple(st.acgt))
    return Spec([In("stream16", bytes_of(stream)), Out("u64", wk, cap=needed), Out("u32", wc, cap=needed)], call,
                (windows, 2 * windows, len(wk), acgt), knobs=knobs)


def kmerize_id(c):
    inp, K, flags, knobs = c
    return "-".join(["kmerize", inp, "K%d" % K, flags] + ["%s%d" % kv for kv in sorted(knobs.items())])


for _c in KMERIZE_CASES:
    case(kmerize_id(_c))(functools.partial(kmerize_spec, *_c))


@case("kmerize-tiny")
def kmerize_tiny():
    """one read of K - 1 + t bases: t windows, 2 t table entries"""
    out = []
    for t in TINY:
        reads = synth.read_strings(170 + t, 0, 1, 24 + t, genome=0)
        out += [kmerize_spec(None, 25, "canonical", {}, reads), kmerize_spec(None, 25, "canonical", dict(dedupe_bits=18), reads)]
    return out


# ---- fixed-size outputs: no cap, the frame is the only check against writing past n ---------------------------------------------------

def rand_keys(seed, n, bits=50):
    return np.random.default_rng(seed).integers(0, 1 << bits, size=n, dtype=U64)


def can_spec(in_place, t=None):
    x = rand_keys(101, t or N)
    want = np.array([zo.can(25, int(v)) for v in x], dtype=U64)
    assert not np.array_equal(want, x)
    if in_place:
        return Spec([IO("u64", x, want)], lambda ctx, v: (ctx.lib.zk_can(ctx.h, 25, v[0].ptr, v[0].n, v[0].ptr), ()))
    return Spec([In("u64", x), Out("u64", want)], lambda ctx, v: (ctx.lib.zk_can(ctx.h, 25, v[0].ptr, v[0].n, v[1].ptr), ()))


def widen_spec(t=None):
    x = np.random.default_rng(102).integers(0, 1 << 32, size=t or N, dtype=U64).astype(U32)
    return Spec([In("u32", x), Out("u64", x.astype(U64))], lambda ctx, v: (ctx.lib.zk_widen_counts(ctx.h, v[0].ptr, v[1].ptr, v[0].n), ()))


def sort_spec(pairs, K, tile_sort, wide, t=None):
    n = t or N
    keys = rand_keys(103 + K, n, 2 * K)
    knobs = dict(tile_sort=tile_sort, wide_tiles=wide)
    if not pairs:
        return Spec([IO("u64", keys, np.sort(keys))], lambda ctx, v: (ctx.lib.zk_sort_keys(ctx.h, v[0].ptr, v[0].n, 2 * K), ()), knobs=knobs)
    vals = np.arange(n, dtype=U32) * U32(2654435761)
    order = np.argsort(keys, kind="stable")
    return Spec([IO("u64", keys, keys[order]), IO("u32", vals, vals[order])],
                lambda ctx, v: (ctx.lib.zk_sort_pairs(ctx.h, v[0].ptr, v[1].ptr, v[0].n, 2 * K), ()), knobs=knobs)


def undelta_spec(t=None):
    d = rand_keys(105, t or N, 40)
    base = 0xFFFFFFFFFFFF0000          # (the sums wrap, as the library's do)
    with np.errstate(over="ignore"):
        want = np.cumsum(d, dtype=U64) + U64(base)
    return Spec([IO("u64", d, want)], lambda ctx, v: (ctx.lib.zk_undelta(ctx.h, v[0].ptr, v[0].n, base), ()))


def add_spec(t=None):
    d = rand_keys(106, t or N, 64)
    with np.errstate(over="ignore"):
        want = d + U64(0x123456789ABCDEF1)
    return Spec([IO("u64", d, want)], lambda ctx, v: (ctx.lib.zk_add_u64(ctx.h, v[0].ptr, v[0].n, 0x123456789ABCDEF1), ()))


for _nm, _fn in (("can", functools.partial(can_spec, False)), ("can-in_place", functools.partial(can_spec, True)), ("widen_counts", widen_spec),
                 ("undelta", undelta_spec), ("add_u64", add_spec)):
    case(_nm)(_fn)
    case(_nm + "-tiny")(lambda _f=_fn: [_f(t) for t in TINY])
for _p in (0, 1):
    for _K in (12, 31):
        for _ts in (0, 1):
            for _w in (0, 1):
                _fn = functools.partial(sort_spec, _p, _K, _ts, _w)
                case("sort_%s-K%d-tile_sort%d-wide%d" % ("pairs" if _p else "keys", _K, _ts, _w))(_fn)
    case("sort_%s-tiny" % ("pairs" if _p else "keys"))(lambda _x=_p: [sort_spec(_x, K, 1, 1, t) for K in (12, 31) for t in TINY])


def hash_partition_spec(world, cdt, t=None):
    n = t or N
    keys = np.sort(rand_keys(107, n))
    seed = 9
    owner = np.array([(zo.murmer(int(x), seed) * world) >> 64 for x in keys], dtype=np.int64)
    want_offs = tuple([0] + [int(v) for v in np.cumsum(np.bincount(owner, minlength=world))])
    order = np.argsort(owner, kind="stable")
    offs = (C.c_uint64 * (world + 1))()
    if cdt is None:
        return Spec([In("u64", keys), Out("u64", keys[order])],
                    lambda ctx, v: (ctx.lib.zk_hash_partition(ctx.h, v[0].ptr, None, 64, v[0].n, world, seed, v[1].ptr, None, offs), tuple(offs)),
                    want_offs)
    bits = 8 * np.dtype(cdt).itemsize
    counts = np.random.default_rng(108).integers(1, 1 << 31, size=n, dtype=U64).astype(cdt)
    ck = "u%d" % bits
    return Spec([In("u64", keys), In(ck, counts), Out("u64", keys[order]), Out(ck, counts[order])],
                lambda ctx, v: (ctx.lib.zk_hash_partition(ctx.h, v[0].ptr, v[1].ptr, bits, v[0].n, world, seed, v[2].ptr, v[3].ptr, offs),
                                tuple(offs)), want_offs)


for _w in (1, 3, 32):
    for _cdt in (None, np.uint32, np.uint64):
        _nm = "hash_partition-world%d-%s" % (_w, "keys" if _cdt is None else np.dtype(_cdt).name)
        case(_nm)(functools.partial(hash_partition_spec, _w, _cdt))
case("hash_partition-tiny")(lambda: [hash_partition_spec(3, c, t) for c in (None, np.uint32, np.uint64) for t in TINY])


def links_spec(staged, t=None):
    """staged: the closed set of a random genome, a tile's successors lie in windows that fit LDS; else 40 000 of the 65 536
    8-mers, a set so dense that the windows of a tile hold more than 5 tiles and are searched in place"""
    if staged:
        K, xs = 15, contig_set(15, 9000, 95)
    else:
        K = 8
        xs = np.sort(np.random.default_rng(109).choice(1 << 16, size=40000, replace=False)).astype(U64)
    if t is not None:
        xs = xs[:t]
    nxt, rank = CL.np_links(K, xs)
    return Spec([In("u64", xs), Out("u32", nxt), Out("u32", rank)],
                lambda ctx, v: (ctx.lib.zk_debruijn_links(ctx.h, v[0].ptr, v[0].n, K, v[1].ptr, v[2].ptr), ()))


case("debruijn_links-staged")(functools.partial(links_spec, True))
case("debruijn_links-in_place")(functools.partial(links_spec, False))
case("debruijn_links-tiny")(lambda: [links_spec(True, t) for t in TINY])


@functools.lru_cache(maxsize=None)
def index_arrays(n_keys=6000, n_records=N):
    """a k-mer index as arrays (library/index.py: S, T, U): ascending keys, CSR offsets, ascending record ids per key"""
    rng = np.random.default_rng(110)
    keys = np.sort(rng.choice(1 << 50, size=n_keys, replace=False)).astype(U64)
    lens = rng.choice([1, 1, 2, 3, 70], size=n_keys)
    lists = [np.sort(rng.choice(n_records, size=min(int(m), n_records), replace=False)) for m in lens]
    offs = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(U32)
    return keys, offs, np.concatenate(lists).astype(U32), n_records


class HeldIndex(Held):
    def get(self, ctx, *shape):
        if self.key != (id(ctx), shape):
            keys, offs, ids, nr = index_arrays(*shape)
            self.table = ctx.bait_table_from_arrays(25, ctx.upload(keys), ctx.upload(offs), ctx.upload(ids), nr)
            self.key = (id(ctx), shape)
        return self.table


_index = HeldIndex()


def index_shape(t):
    return (6000, N) if t is None else (40, t)


def bait_tally_spec(t=None):
    keys, offs, ids, nr = index_arrays(*index_shape(t))
    rng = np.random.default_rng(111)
    kmers = np.sort(np.unique(np.concatenate([rng.choice(keys, size=len(keys) // 2, replace=False),
                                              rng.choice(1 << 50, size=N if t is None else 30).astype(U64)])))
    m = np.isin(keys, kmers)
    hits = np.zeros(nr, dtype=U32)
    np.add.at(hits, ids[np.repeat(m, np.diff(offs.astype(np.int64)))], 1)
    return Spec([In("u64", kmers), Out("u32", hits)],
                lambda ctx, v: (ctx.lib.zk_bait_tally(ctx.h, _index.get(ctx, *index_shape(t)).h, v[0].ptr, v[0].n, v[1].ptr), ()))


def record_sizes_spec(t=None):
    keys, offs, ids, nr = index_arrays(*index_shape(t))
    return Spec([Out("u32", np.bincount(ids, minlength=nr).astype(U32))],
                lambda ctx, v: (ctx.lib.zk_bait_record_sizes(ctx.h, _index.get(ctx, *index_shape(t)).h, v[0].ptr), ()))


def from_arrays_spec(t=None):
    """the three input arrays on offsets; the table's own copies must equal them"""
    keys, offs, ids, nr = index_arrays(*index_shape(t))

    def call(ctx, v):
        h = C.c_void_p()
        rc = ctx.lib.zk_bait_table_from_arrays(ctx.h, 25, v[0].ptr, v[0].n, v[1].ptr, v[2].ptr, v[2].n, nr, C.byref(h))
        if rc != OK:
            return rc, ()
        table = native.BaitTable(ctx, h.value, 25)
        got = tuple(a.to_host().tobytes() for a in table.arrays())
        sizes = ctx.bait_record_sizes(table).to_host()
        table.free()
        return rc, (table.n_keys, table.n_ids, table.n_records) + got + (sizes.tobytes(),)
    return Spec([In("u64", keys), In("u32", offs), In("u32", ids)], call,
                (len(keys), len(ids), nr, keys.tobytes(), offs.tobytes(), ids.tobytes(), np.bincount(ids, minlength=nr).astype(U32).tobytes()))


for _nm, _fn in (("bait_tally", bait_tally_spec), ("bait_record_sizes", record_sizes_spec), ("bait_table_from_arrays", from_arrays_spec)):
    case(_nm)(_fn)
    case(_nm + "-tiny")(lambda _f=_fn: [_f(t) for t in TINY])


def pack_reads_spec(t=None):
    reads = synth.read_strings(9, 0, 300, 61, genome=0) + ["", "ACGT", "T" * 200] if t is None else ["ACGTN"[:t - 1]] if t < 5 else ["A", "", "G"]
    bases = bytes_of("".join(reads).encode() or b"")
    offs = np.concatenate([[0], np.cumsum([len(r) for r in reads])]).astype(U64)
    want = bytes_of(cc.stream_of(reads))          # (t bytes: t - 1 bases and the newline; 5: three reads, one of them empty)
    assert t is None or len(want) == t
    return Spec([In("byte", bases if len(bases) else np.zeros(1, dtype=U8)), In("u64", offs), Out("byte", want)],
                lambda ctx, v: (ctx.lib.zk_pack_reads(ctx.h, v[0].ptr, v[1].ptr, v[1].n - 1, v[2].ptr), ()))


def capture_filter_spec(t=None):
    """reads without a hit are blanked; the baits are the k-mers of both strands of every other read.  tiny: streams of 1, 3 and
    5 bytes at K = 2"""
    K = 25 if t is None else 2
    reads = synth.read_strings(7, 0, 195, 150, genome=0) + ["ACGT", ""] if t is None else {1: [""], 3: ["AC"], 5: ["AC", "G"]}[t]
    baits = np.unique(np.concatenate([zo.kmers_list(K, r, True) for r in (reads[::2] if t is None else ["AC"])]))
    bset = set(int(b) for b in baits)
    out, kept = [], 0
    for r in reads:
        hit = any(int(x) in bset for x in zo.kmers_list(K, r, False))
        kept += hit
        out.append(r if hit else "N" * len(r))
    nr, nk = C.c_uint64(0), C.c_uint64(0)

    def call(ctx, v):
        rc = ctx.lib.zk_capture_filter(ctx.h, v[0].ptr, v[0].n, K, v[1].ptr, v[1].n, v[2].ptr, C.byref(nr), C.byref(nk))
        return rc, (nr.value, nk.value)
    assert t is None or len(cc.stream_of(out)) == t
    return Spec([In("stream16", bytes_of(cc.stream_of(reads))), In("u64", baits), Out("byte", bytes_of(cc.stream_of(out)))], call,
                (len(reads), kept))


def fastq_mask_np(text, phase):
    t = bytes_of(text)
    nl = t == 10
    line = phase + np.cumsum(nl) - nl
    return np.where((line % 4 == 1) & ~nl, t, U8(10)).astype(U8), int(nl.sum())


def fastq_mask_spec(phase, t=None):
    """both arrays need 16 bytes"""
    text = synth.fastq_text(11, 0, 120, 97, genome=0, n_thr=synth.frac32(0.02)).encode()
    text = text[len(b"@r0\n") * (phase > 0):] if phase < 2 else text[text.index(b"+"):]
    if t is not None:
        text = b"ACGTA"[:t - 1] + b"\n"          # t bytes: a sequence line (one line precedes it)
        phase = 1
    assert phase in (0, 1, 2)
    want, n_nl = fastq_mask_np(text, phase)
    assert t is None or (len(want) == t and want.tobytes() == text)
    n = C.c_uint64(0)

    def call(ctx, v):
        rc = ctx.lib.zk_fastq_mask(ctx.h, v[0].ptr, v[0].n, phase, v[1].ptr, C.byref(n))
        return rc, (n.value,)
    return Spec([In("stream16", bytes_of(text)), Arr("out", "stream16", want=want)], call, (n_nl,))


def synth_keys_spec(t=None):
    args = (5, 1000, t or N, 50, 7, 3, 40000)
    want = synth.set_keys_raw(args[0], args[1], args[2], args[3], mul=args[4], add=args[5], mod=args[6])
    return Spec([Out("u64", want)], lambda ctx, v: (ctx.lib.zk_synth_keys(ctx.h, *args, v[0].ptr), ()))


def synth_counts_spec(t=None):
    keys = synth.set_keys(5, 0, t or N, 50)
    return Spec([In("u64", keys), Out("u64", synth.set_counts(5, keys))],
                lambda ctx, v: (ctx.lib.zk_synth_counts(ctx.h, 5, v[0].ptr, v[0].n, v[1].ptr), ()))


def synth_reads_spec(t=None):
    count, L = (163, 150) if t is None else (1, max(t - 1, 1))          # (L >= 1: the shortest stream has 2 bytes; then 3 and 5)
    kw = dict(genome=5000, sub_thr=synth.frac32(0.005), n_thr=synth.frac32(0.01)) if t is None else dict(genome=0)
    want = synth.base_stream(3, 77, count, L, **kw)
    return Spec([Out("byte", want)], lambda ctx, v: (ctx.lib.zk_synth_reads(ctx.h, 3, 77, count, L, kw.get("genome", 0), kw.get("sub_thr", 0),
                                                                          kw.get("n_thr", 0), v[0].ptr), ()))


def copy_spec(t=None):
    """odd byte counts between odd byte offsets: dst[3 : 3 + m] = src[5 : 5 + m]"""
    m = 2 * ((t or N) // 2) + 1
    src = np.random.default_rng(112).integers(0, 256, size=m + 11, dtype=np.int64).astype(U8)
    dst = np.full(m + 9, 0x5A, dtype=U8)
    want = dst.copy()
    want[3:3 + m] = src[5:5 + m]
    return Spec([In("byte", src), IO("byte", dst, want)], lambda ctx, v: (ctx.lib.zk_copy(ctx.h, v[1].ptr + 3, v[0].ptr + 5, m), ()))


for _nm, _fn in (("pack_reads", pack_reads_spec), ("capture_filter", capture_filter_spec), ("synth_keys", synth_keys_spec),
                 ("synth_counts", synth_counts_spec), ("synth_reads", synth_reads_spec), ("copy", copy_spec)):
    case(_nm)(_fn)
    case(_nm + "-tiny")(lambda _f=_fn: [_f(t) for t in TINY])
for _ph in (0, 1, 2):
    case("fastq_mask-phase%d" % _ph)(functools.partial(fastq_mask_spec, _ph))
case("fastq_mask-tiny")(lambda: [fastq_mask_spec(0, t) for t in TINY])


# ---- the reducers: inputs on offsets, the scalars the oracle's, the inputs untouched ------------------------------------------------------

def reducer(name, build):
    case(name)(build)
    case(name + "-tiny")(lambda: [build(t) for t in TINY])


def split_spec(t=None):
    x, _, y, _, zs, _ = cc.union_case()
    if t is not None:
        x, y = zs[:t][np.arange(t) % 3 != 2], zs[:t][np.arange(t) % 3 != 1]
    both = len(np.intersect1d(x, y))
    abc = (C.c_uint64 * 3)()
    return Spec([Slab("u64", [x, y])], lambda ctx, v: (ctx.lib.zk_split(ctx.h, v[0].ptr, v[0].n, v[1].ptr, v[1].n, abc), tuple(abc)),
                (both, len(x) - both, len(y) - both))


def spectrum_spec(t=None):
    """the integers equal the oracle's; the two doubles equal the run at P0 bit for bit (the header promises the same bits for the
    same call); their distance to the oracle is the business of tests/test_gpu_dist_spectrum.py"""
    x, xc, y, yc, zs, _ = cc.union_case()
    if t is not None:
        ix, iy = np.arange(t) % 3 != 2, np.arange(t) % 3 != 1
        x, y, xc, yc = zs[:t][ix], zs[:t][iy], xc[:int(ix.sum())], yc[:int(iy.sum())]
    w = H.host_spectrum_sums(x, xc, y, yc)
    r = native.Spectrum()

    def call(ctx, v):
        rc = ctx.lib.zk_spectrum_sums(ctx.h, v[0].ptr, v[2].ptr, v[0].n, v[1].ptr, v[3].ptr, v[1].n, float(w["cx"]), float(w["cy"]), C.byref(r))
        return (rc, (r.n_shared, r.s_min, r.x_shared, r.y_shared, int(r.s_xy_lo) | (int(r.s_xy_hi) << 64)),
                (np.float64(r.s_sqrt).tobytes(), np.float64(r.s_js).tobytes()))
    return Spec([Slab("u64", [x, y]), Slab("u64", [xc, yc])], call, (w["n_shared"], w["S_min"], w["X_shared"], w["Y_shared"], w["S_xy"]))


def lower_bound_spec(t=None):
    keys = np.sort(rand_keys(113, t or N))
    q = np.concatenate([np.array([0, M64], dtype=U64), keys[::max(1, len(keys) // 50)], keys[::max(1, len(keys) // 50)] + U64(1)])
    pos = np.zeros(len(q), dtype=U64)
    return Spec([In("u64", keys)],
                lambda ctx, v: (ctx.lib.zk_lower_bound(ctx.h, v[0].ptr, v[0].n, q.ctypes.data_as(u64p), len(q), pos.ctypes.data_as(u64p)),
                                tuple(int(p) for p in pos)), tuple(int(p) for p in np.searchsorted(keys, q, side="left")))


def first_descent_spec(t=None):
    keys = np.sort(rand_keys(114, t or N))
    r = C.c_uint64(0)
    call = lambda ctx, v: (ctx.lib.zk_first_descent(ctx.h, v[0].ptr, v[0].n, C.byref(r)), (r.value,))
    specs = [Spec([In("u64", keys)], call, (len(keys),))]
    if len(keys) > 1:          # a descent at the last element, seen only by the thread that holds the array's end
        bad = keys.copy()
        bad[-1] = bad[-2]
        specs.append(Spec([In("u64", bad)], call, (len(keys) - 1,)))
    return specs


def checksums_of(keys, weights):
    kl, w = [int(v) for v in keys], [int(v) for v in weights]
    return (sum(w) & M64, sum(a * b for a, b in zip(kl, w)) & M64, sum(zo.murmer(a, 0) * b for a, b in zip(kl, w)) & M64)


def checksum_spec(t=None):
    keys = rand_keys(115, t or N)
    counts = np.random.default_rng(116).integers(0, 1 << 32, size=len(keys), dtype=U64).astype(U32)
    s = (C.c_uint64 * 3)()
    return [Spec([In("u64", keys), In("u32", counts)], lambda ctx, v: (ctx.lib.zk_checksum(ctx.h, v[0].ptr, v[1].ptr, v[0].n, s), tuple(s)),
                 checksums_of(keys, counts)),
            Spec([In("u64", keys)], lambda ctx, v: (ctx.lib.zk_checksum(ctx.h, v[0].ptr, None, v[0].n, s), tuple(s)),
                 checksums_of(keys, [1] * len(keys)))]


def checksum_counts_spec(t=None):
    keys = rand_keys(117, t or N)
    out = []
    for cdt in (np.uint32, np.uint64):
        bits = 8 * np.dtype(cdt).itemsize
        counts = np.random.default_rng(118).integers(0, 1 << (bits - 1), size=len(keys), dtype=U64).astype(cdt)
        s = (C.c_uint64 * 3)()
        out.append(Spec([In("u64", keys), In("u%d" % bits, counts)],
                        lambda ctx, v, _b=bits, _s=s: (ctx.lib.zk_checksum_counts(ctx.h, v[0].ptr, v[1].ptr, _b, v[0].n, _s), tuple(_s)),
                        checksums_of(keys, counts)))
    return out


def stream_checksum_spec(t=None):
    K = 25
    reads = synth.read_strings(5, 0, 150, 131, genome=0, n_thr=synth.frac32(0.02)) + ["", "A", "acgun" * 30] if t is None else \
        synth.read_strings(5, 0, 1, 24 + t, genome=0)
    xs = np.concatenate([zo.kmers_list(K, r, True) for r in reads] + [np.zeros(0, dtype=U64)])
    want = (len(xs), int(xs.sum(dtype=U64)), sum(zo.murmer(int(x), 0) for x in xs) & M64) + acgt_of(xs)
    s = (C.c_uint64 * 7)()
    return Spec([In("stream16", bytes_of(cc.stream_of(reads)))],
                lambda ctx, v: (ctx.lib.zk_stream_checksum(ctx.h, v[0].ptr, v[0].n, K, s), tuple(s)), want)


def hist_spec(cdt, t=None):
    counts = cc.hist_case()
    if t is not None:
        counts = counts[np.isin(counts, np.unique(counts)[-t:])]          # the t largest values: t bins, some beyond the dense range
    wv, wf = zo.hist(counts)
    assert t is None or len(wv) == t
    bits = 8 * np.dtype(cdt).itemsize
    vals, freq = np.zeros(len(wv), dtype=U64), np.zeros(len(wv), dtype=U64)
    n = C.c_uint64(0)

    def call(ctx, v):
        rc = ctx.lib.zk_hist(ctx.h, v[0].ptr, bits, v[0].n, vals.ctypes.data_as(u64p), freq.ctypes.data_as(u64p), len(vals), C.byref(n))
        return rc, (n.value, vals.tobytes(), freq.tobytes())
    return Spec([In("u%d" % bits, counts.astype(cdt))], call, (len(wv), np.asarray(wv, dtype=U64).tobytes(), np.asarray(wf, dtype=U64).tobytes()))


def count_spectrum_spec(t=None):
    """the dict rule of `zot disass` over a counted canonical key list: a palindrome one entry of twice the count if sub(c), else
    [sub(c)] + [sub(rc c)] entries of the count"""
    K, seed, p = 12, 17, 0.7
    rng = np.random.default_rng(119)
    x = rng.integers(0, 1 << (2 * K), size=t or N, dtype=U64)
    h = rng.integers(0, 1 << K, size=(t or N) // 50 + 1, dtype=U64)
    x[:len(h)] = (h << U64(K)) | cc.revcomp(h, K // 2)
    keys = np.unique(np.minimum(x, cc.revcomp(x, K)))
    counts = rng.integers(1, 40, size=len(keys), dtype=U64).astype(U32)
    hist = {}
    for c, n in zip(keys.tolist(), counts.tolist()):
        r = dr_rc(K, c)
        value, entries = (2 * n, int(DR.sub(seed, p, c))) if r == c else (n, int(DR.sub(seed, p, c)) + int(DR.sub(seed, p, r)))
        if entries:
            hist[value] = hist.get(value, 0) + entries
    want = sorted(hist.items())
    vals, freq = np.zeros(len(want) + 1, dtype=U64), np.zeros(len(want) + 1, dtype=U64)
    n_bins = C.c_uint64(0)

    def call(ctx, v):
        rc = ctx.lib.zk_count_spectrum(ctx.h, v[0].ptr, v[1].ptr, 32, v[0].n, K, 1, seed, p, vals.ctypes.data_as(u64p),
                                       freq.ctypes.data_as(u64p), len(vals), C.byref(n_bins))
        return rc, (tuple(zip(vals[:n_bins.value].tolist(), freq[:n_bins.value].tolist())),)
    return Spec([In("u64", keys), In("u32", counts)], call, (tuple(want),))


def probe_scan_spec(t=None):
    K = 25
    keys = np.sort(rand_keys(120, t or N))
    wins = [(25, int(keys[0])), (25, int(keys[-1]) ^ 1), (20, int(keys[len(keys) // 2]) >> 10), (1, 2), (7, int(keys[-1]) >> 36)]
    arr = (native.ProbeWindow * len(wins))(*[native.ProbeWindow(v, J, 0) for J, v in wins])
    want = []
    for J, v in wins:
        z = (keys >> U64(2 * (K - J))) ^ U64(v)
        d = np.array([bin(int((a | (a >> 1)) & 0x5555555555555555)).count("1") for a in z.tolist()])
        want += [int(np.sum(d == e)) for e in range(3)]
    tallies = np.zeros(3 * len(wins), dtype=U64)
    return Spec([In("u64", keys)],
                lambda ctx, v: (ctx.lib.zk_probe_scan(ctx.h, v[0].ptr, v[0].n, K, arr, len(wins), tallies.ctypes.data_as(u64p)),
                                tuple(int(x) for x in tallies)), tuple(want))


def last_newline_spec(t=None):
    text = cc.capture_case()[0][:N if t is None else 200]
    cut = C.c_uint64(0)
    specs = []
    for n in ((len(text), len(text) - 37, 3) if t is None else (t + 30,)):
        want = text[:n].rfind(b"\n") + 1
        specs.append(Spec([In("byte", bytes_of(text))],
                          lambda ctx, v, _n=n: (ctx.lib.zk_last_newline(ctx.h, v[0].ptr, _n, C.byref(cut)), (cut.value,)), (want,)))
    return specs


for _nm, _fn in (("split", split_spec), ("spectrum_sums", spectrum_spec), ("lower_bound", lower_bound_spec), ("first_descent", first_descent_spec),
                 ("checksum", checksum_spec), ("checksum_counts", checksum_counts_spec), ("stream_checksum", stream_checksum_spec),
                 ("hist-uint32", functools.partial(hist_spec, np.uint32)), ("hist-uint64", functools.partial(hist_spec, np.uint64)),
                 ("count_spectrum", count_spectrum_spec), ("probe_scan", probe_scan_spec), ("last_newline", last_newline_spec)):
    reducer(_nm, _fn)


def flat(specs):
    out = []
    for s in specs if isinstance(specs, list) else [specs]:
        out += flat(s) if isinstance(s, list) else [s]
    return out


# the entries that need a 16-byte aligned stream (include/zotk.h)
SIXTEEN = {          # entry -> (a case, the arrays of its Spec that must be 16-byte aligned)
    "zk_encode": ("encode-both1", (0,)),
    "zk_capture_filter": ("capture_filter", (0,)),
    "zk_kmerize": ("kmerize-deep-K25-canonical", (0,)),
    "zk_stream_checksum": ("stream_checksum", (0,)),
    "zk_fastq_mask-text": ("fastq_mask-phase0", (0,)),
    "zk_fastq_mask-stream": ("fastq_mask-phase0", (1,)),
}
