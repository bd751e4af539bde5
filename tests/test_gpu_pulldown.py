"""`zot pulldown` on the device: zk_pulldown_hits against the restatement of the reference's semantics
(tests/_pulldown_restatement.py) on every fixture case, the veto path of zk_capture_hits against it, the capacity contract of
the new entry, and the command end to end against the reference's fixtures (tests/golden/p1_pulldown.json)."""
import contextlib
import ctypes as C
import functools
import hashlib
import io
import json
import os
import tempfile
import zipfile

import numpy as np
import pytest

from tests import _pulldown_restatement as R
from tests._pulldown_cases import make_cases

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "p1_pulldown.json")
INPUTS = {c["name"]: c for c in make_cases()}
CASES = [dict(INPUTS[g["name"]], gold=g) for g in json.load(open(GOLD))]
IDS = [c["name"] for c in CASES]
ONE_PAIR = [c for c in CASES if len(c["inputs"]) == 2]
GUARD = 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as ge
    ge.build()
    from zotmer_amd.library import engine
    yield engine.context()
    engine.close()


@functools.lru_cache(maxsize=None)
def expected(name):
    """the restatement on a case of one file pair, computed once -> (pairs u64 ascending, hist u64[n_records + 1], vetoed, reads)"""
    case = INPUTS[name]
    names, idx, anti = R.tables(case["baits"], case["up"])
    hits, _, _ = R.walk(idx, anti, *case["inputs"])
    pairs = sorted((b << 32) | r for r, h in enumerate(hits) if h is not None for b in h)
    hist = np.zeros(len(names) + 1, np.uint64)
    for h in hits:
        if h is not None:
            hist[len(h)] += 1
    return np.array(pairs, np.uint64), hist, sum(h is None for h in hits), len(hits)


class Batch:
    """a case of one file pair on the device: both tables, both texts with their line ends"""

    def __init__(self, ctx, case):
        from zotmer_amd.library import capture
        self.table = capture.build_table(ctx, [(nm, s.encode()) for nm, s in R.fasta_records(case["baits"])], 25)
        up = [(nm, s.encode()) for nm, s in R.fasta_records(case["up"] or "")]
        self.veto = capture.build_table(ctx, up, 25) if up else None
        self.texts = [ctx.upload_stream(t.encode()) for t in case["inputs"]]
        self.lines = [ctx.line_ends(t) for t in self.texts]
        self.n_reads = min(l.n // 4 for l in self.lines)

    def free(self):
        self.table.free()
        if self.veto is not None:
            self.veto.free()


@pytest.mark.parametrize("case", ONE_PAIR, ids=[c["name"] for c in ONE_PAIR])
def test_pulldown_hits_against_the_restatement(ctx, case):
    want_pairs, want_hist, want_vetoed, n = expected(case["name"])
    b = Batch(ctx, case)
    try:
        assert b.n_reads == n
        pairs, hist, vetoed = ctx.pulldown_hits(b.table, 25, b.texts[0], b.lines[0], n, b.texts[1], b.lines[1], veto=b.veto)
        assert np.array_equal(pairs.to_host(), want_pairs)
        assert hist.dtype == np.uint64 and np.array_equal(hist, want_hist)
        assert vetoed == want_vetoed
        assert int(hist.sum()) + vetoed == n
        # the veto path of zk_capture_hits, which `zot capture` never takes: the same pairs
        got = ctx.capture_hits(b.table, 25, b.texts[0], b.lines[0], n, b.texts[1], b.lines[1], veto=b.veto)
        assert np.array_equal(got.to_host(), want_pairs)
    finally:
        b.free()


def test_the_veto_counts_for_something():
    """the cases above would pass with a veto that never fires only if no case had one"""
    assert expected("paired_U")[2] > 0 and expected("edges_U")[2] == 5 and expected("emptybaits_U")[2] == 5
    assert len(expected("paired_U")[0]) < len(expected("paired")[0])
    assert expected("many")[1][1500] == 1


def raw_call(ctx, b, pairs, cap, hist, hist_cap):
    n, nv = C.c_uint64(0), C.c_uint64(0)
    rc = ctx.lib.zk_pulldown_hits(ctx.h, b.table.h, b.veto.h if b.veto is not None else None, 25, b.texts[0].ptr, b.lines[0].ptr, b.texts[1].ptr,
                                  b.lines[1].ptr, b.n_reads, pairs.ptr if pairs is not None else None, cap, C.byref(n), hist.ptr, hist_cap,
                                  C.byref(nv))
    return rc, n.value, nv.value


def test_capacity_contract(ctx):
    from zotmer_amd import native
    want_pairs, want_hist, want_vetoed, n_reads = expected("paired_U")
    b = Batch(ctx, INPUTS["paired_U"])
    try:
        nb = b.table.n_records + 1
        hist = ctx.upload(np.full(nb + 4, GUARD, np.uint64))
        rc, raw, _ = raw_call(ctx, b, None, 0, hist, nb)                      # cap = 0 sizes the output
        assert rc == native.ZK_ENOSPC and raw >= len(want_pairs) > 0
        for cap in (raw - 1, raw, raw + 5):
            pairs = ctx.upload(np.full(raw + 16, GUARD, np.uint64))
            hist = ctx.upload(np.full(nb + 4, GUARD, np.uint64))
            rc, n, nv = raw_call(ctx, b, pairs, cap, hist, nb)
            got = pairs.to_host()
            assert np.all(got[cap:] == GUARD), cap                             # nothing at or beyond cap
            assert np.all(hist.to_host()[nb:] == GUARD)                        # nothing at or beyond n_records + 1
            if cap < raw:
                assert rc == native.ZK_ENOSPC and n == raw
                continue
            assert rc == native.ZK_OK and n == len(want_pairs) and nv == want_vetoed
            assert np.array_equal(got[:n], want_pairs)
            assert np.array_equal(hist.to_host()[:nb], want_hist)
        # hist_cap: n_records is refused before anything is written, n_records + 1 is enough
        pairs = ctx.upload(np.full(raw + 16, GUARD, np.uint64))
        hist = ctx.upload(np.full(nb + 4, GUARD, np.uint64))
        rc, _, _ = raw_call(ctx, b, pairs, raw, hist, nb - 1)
        assert rc == native.ZK_EINVAL
        assert np.all(hist.to_host() == GUARD) and np.all(pairs.to_host() == GUARD)
        rc, n, nv = raw_call(ctx, b, pairs, raw, hist, nb)                     # the context stays usable
        assert rc == native.ZK_OK and np.array_equal(hist.to_host()[:nb], want_hist) and np.all(hist.to_host()[nb:] == GUARD)
    finally:
        b.free()


def test_first_call_on_an_empty_workspace(ctx):
    """The marks and counters are taken from the arena before the lookup says how much the sort needs: on a workspace too
    small for both, the arena grows and the lookup runs a second time.  The result is the same either way."""
    want_pairs, want_hist, want_vetoed, n = expected("paired_U")
    b = Batch(ctx, INPUTS["paired_U"])
    try:
        for lookups in (2, 1):
            if lookups == 2:
                ctx.release_workspace()
            ctx.profile(True)
            pairs, hist, vetoed = ctx.pulldown_hits(b.table, 25, b.texts[0], b.lines[0], n, b.texts[1], b.lines[1], veto=b.veto)
            prof = ctx.profile_read()
            ctx.profile(False)
            assert prof["capture_hits"]["launches"] == lookups and prof["pulldown_tally"]["launches"] == 2
            assert np.array_equal(pairs.to_host(), want_pairs) and np.array_equal(hist, want_hist) and vetoed == want_vetoed
    finally:
        ctx.profile(False)
        b.free()


def test_no_reads_gives_zeros(ctx):
    b = Batch(ctx, INPUTS["emptyreads"])
    try:
        nb = b.table.n_records + 1
        hist = ctx.upload(np.full(nb + 2, GUARD, np.uint64))
        rc, n, nv = raw_call(ctx, b, None, 0, hist, nb)
        assert (rc, n, nv) == (0, 0, 0)
        assert np.array_equal(hist.to_host(), np.array([0] * nb + [GUARD] * 2, np.uint64))
    finally:
        b.free()


# ---- the command ---------------------------------------------------------------------------------------------

def write_case(d, case):
    d.mkdir(parents=True, exist_ok=True)
    (d / "baits.fa").write_bytes(case["baits"].encode())
    args = ["pulldown", "-p"]
    if case["up"] is not None:
        (d / "up.fa").write_bytes(case["up"].encode())
        args += ["-U", "up.fa"]
    fns = []
    for i, text in enumerate(case["inputs"]):
        (d / ("in%d.fastq" % i)).write_bytes(text.encode())
        fns.append("in%d.fastq" % i)
    return args + ["baits.fa", "out.zip"] + fns


def zot(args):
    from zotmer_amd import cli
    out, err = io.StringIO(), io.StringIO()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        code = cli.main_inner(args)
    return code, out.getvalue(), err.getvalue()


def members(path):
    with zipfile.ZipFile(path) as z:
        assert all(i.compress_type == zipfile.ZIP_DEFLATED for i in z.infolist())
        return [(i.filename, z.read(i)) for i in z.infolist()]


def digests(ms):
    return [(nm, hashlib.sha256(b).hexdigest(), len(b)) for nm, b in ms]


def gold_members(g):
    return [(nm, g["digests"][i]["sha256"], g["digests"][i]["size"]) for nm, i in g["members"]]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_command_against_the_reference(ctx, tmp_path, monkeypatch, case):
    monkeypatch.chdir(tmp_path)
    code, out, err = zot(write_case(tmp_path, case))
    assert code == 0 and err == ""                        # unequal files: nothing on stderr
    assert out == case["gold"]["stdout"]
    got = digests(members("out.zip"))
    if case["name"] == "two_pairs":
        # the archive is opened once: the first file pair's members are those of its own case, then come the reference's
        first = gold_members(next(c for c in CASES if c["name"] == "edges_U")["gold"])
        assert got[:len(first)] == first
        got = got[len(first):]
    assert got == gold_members(case["gold"])


def test_absolute_input_paths(ctx, tmp_path):
    case = INPUTS["unequal_5_3"]
    args = write_case(tmp_path, case)
    full = [str(tmp_path / a) for a in args[2:]]
    code, out, _ = zot(args[:2] + full)
    assert code == 0 and out == "2\t3\n"
    names = [nm for nm, _ in members(full[1])]
    assert names[0] == "e0/" + full[2].lstrip("/") and names[1] == "e0/" + full[3].lstrip("/")


def test_batch_size_does_not_matter(ctx, tmp_path, monkeypatch):
    from zotmer_amd.library import capture, pulldown
    case = next(c for c in CASES if c["name"] == "paired_U")
    monkeypatch.chdir(tmp_path)
    args = write_case(tmp_path, case)
    recs, up = capture.bait_records("baits.fa"), capture.bait_records("up.fa")
    table, veto = capture.build_table(ctx, recs, 25), capture.build_table(ctx, up, 25)
    names = [nm.decode() for nm, _ in recs]
    res = []
    try:
        for batch in (4096, 64 << 20):                     # ~14 batches per mate, cut at different records of either; one batch
            out = io.StringIO()
            hist, vetoed = pulldown.pulldown(ctx, table, veto, names, args[-2:], "b%d.zip" % batch, batch, out=out)
            res.append((out.getvalue(), members("b%d.zip" % batch), vetoed))
    finally:
        table.free()
        veto.free()
    assert res[0] == res[1]
    assert res[0][0] == case["gold"]["stdout"] and digests(res[0][1]) == gold_members(case["gold"])
    assert res[0][2] == expected("paired_U")[2]


def test_temp_files_are_gone(ctx, tmp_path, monkeypatch):
    from zotmer_amd.library import capture, pulldown
    case = next(c for c in CASES if c["name"] == "edges_U")
    monkeypatch.chdir(tmp_path)
    args = write_case(tmp_path, case)
    tmp = tmp_path / "tmp"
    tmp.mkdir()
    monkeypatch.setattr(tempfile, "tempdir", str(tmp))
    seen = []
    write = pulldown.Archive.write

    def spy(self, mate, host_bytes, byte_spans):
        write(self, mate, host_bytes, byte_spans)
        seen.append((os.path.dirname(self.tmpdir), len(os.listdir(self.tmpdir))))
    monkeypatch.setattr(pulldown.Archive, "write", spy)
    code, out, _ = zot(args)
    assert code == 0 and out == case["gold"]["stdout"]
    assert seen == [(str(tmp), 4), (str(tmp), 8)]          # the temp files were there, under tempfile's directory
    assert os.listdir(tmp) == []
    # a run that raises in the middle of a file pair, with temp files written: a record longer than the batch comes late
    del seen[:]
    for m in range(2):
        with open("in%d.fastq" % m, "a") as f:
            f.write("@long/%d\n%s\n+\n%s\n" % (m + 1, "ACGT" * 1500, "I" * 6000))
    recs, up = capture.bait_records("baits.fa"), capture.bait_records("up.fa")
    table, veto = capture.build_table(ctx, recs, 25), capture.build_table(ctx, up, 25)
    try:
        with pytest.raises(IOError, match="longer than the batch size"):
            pulldown.pulldown(ctx, table, veto, [nm.decode() for nm, _ in recs], ["in0.fastq", "in1.fastq"], "bad.zip", 4096, out=io.StringIO())
    finally:
        table.free()
        veto.free()
    assert seen and seen[-1][0] == str(tmp) and seen[-1][1] > 0
    assert os.listdir(tmp) == []
