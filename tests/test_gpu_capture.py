"""`zot capture` on the device against the reference's fixtures (tests/golden/c1_capture.json), against the restatement of
its semantics (tests/_capture_restatement.py) on random cases, and against the independent zk_capture_filter at full size."""
import bz2
import contextlib
import gzip
import hashlib
import io
import json
import os
import random

import numpy as np
import pytest

from tests import _capture_restatement as R
from tests._capture_cases import make_cases

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c1_capture.json")
INPUTS = {c["name"]: c for c in make_cases()}
CASES = [dict(c, baits=INPUTS[c["name"]]["baits"], inputs=INPUTS[c["name"]]["inputs"]) for c in json.load(open(GOLD))]


@pytest.fixture(scope="module")
def ctx():
    import __graft_entry__ as ge
    ge.build()
    from zotmer_amd.library import engine
    yield engine.context()
    engine.close()


def write_case(d, case, compress=None):
    d.mkdir(parents=True, exist_ok=True)
    (d / "out").mkdir(exist_ok=True)
    fa = d / "baits.fa"
    fa.write_bytes(case["baits"].encode())
    paths = []
    for i, text in enumerate(case["inputs"]):
        data = text.encode()
        if compress == "gz":
            p = d / ("in%d.fastq.gz" % i)
            p.write_bytes(gzip.compress(data))
        elif compress == "bz2":
            p = d / ("in%d.fastq.bz2" % i)
            p.write_bytes(bz2.compress(data))
        else:
            p = d / ("in%d.fastq" % i)
            p.write_bytes(data)
        paths.append(str(p))
    return str(fa), paths


def zot(args):
    from zotmer_amd import cli
    err = io.StringIO()
    with contextlib.redirect_stderr(err):
        code = cli.main_inner(args)
    return code, err.getvalue()


def run_case(ctx, d, case, extra=(), compress=None, z=False):
    fa, paths = write_case(d, case, compress)
    args = ["capture", "-k", str(case["k"]), "-P", str(d / "out")] + list(extra)
    if case.get("paired"):
        args.append("-p")
    if z:
        args.append("-z")
    code, err = zot(args + [fa] + paths)
    assert code == 0
    files = {}
    for fn in sorted(os.listdir(d / "out")):
        b = (d / "out" / fn).read_bytes()
        if z:
            assert fn.endswith(".gz")
            fn, b = fn[:-3], gzip.decompress(b)
        files[fn] = b
    return files, err.replace(str(d / "out"), "<P>")


def matches(files, err, case):
    assert err == case["stderr"]
    assert sorted(files) == sorted(case["files"])
    for fn, want in case["files"].items():
        assert (hashlib.sha256(files[fn]).hexdigest(), len(files[fn])) == (want["sha256"], want["size"]), fn


IDS = [c["name"] for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fixture(ctx, tmp_path, case):
    files, err = run_case(ctx, tmp_path, case)
    matches(files, err, case)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_batch_size_does_not_matter(ctx, tmp_path, case):
    files, err = run_case(ctx, tmp_path / "m1", case, extra=["-m", "1"])
    matches(files, err, case)
    # batches of a few records: the mates of -p are cut at different bytes, and carried tails hold parts of records
    from zotmer_amd.library import capture
    for batch in (700, 1531):
        d = tmp_path / ("b%d" % batch)
        fa, paths = write_case(d, case)
        recs = capture.bait_records(fa)
        table = capture.build_table(ctx, recs, case["k"])
        sink = capture.Sink([nm for nm, _ in recs], str(d / "out"), case.get("paired", False), False)
        capture.capture_inputs(ctx, table, paths, case.get("paired", False), sink, batch)
        table.free()
        buf = io.StringIO()
        sink.end(buf)
        got = {fn: (d / "out" / fn).read_bytes() for fn in os.listdir(d / "out")}
        matches(got, buf.getvalue().replace(str(d / "out"), "<P>"), case)


def test_append_doubles_every_file(ctx, tmp_path):
    case = next(c for c in CASES if c["name"] == "paired")
    files1, _ = run_case(ctx, tmp_path, case)
    files2, err = run_case(ctx, tmp_path, case)
    assert sorted(files2) == sorted(files1) and files1
    for fn in files1:
        assert files2[fn] == files1[fn] + files1[fn]


@pytest.mark.parametrize("name", ["k24", "paired"])
def test_gzip_output(ctx, tmp_path, name):
    case = next(c for c in CASES if c["name"] == name)
    files, err = run_case(ctx, tmp_path, case, z=True)
    assert err == case["stderr"].replace(".fastq:", ".fastq.gz:")
    matches(files, case["stderr"], case)


@pytest.mark.parametrize("compress", ["gz", "bz2"])
def test_compressed_inputs(ctx, tmp_path, compress):
    for name in ("two_files", "paired"):
        case = next(c for c in CASES if c["name"] == name)
        files, err = run_case(ctx, tmp_path / name, case, compress=compress)
        matches(files, err, case)


def test_mate_2_shorter_warns_and_stops(ctx, tmp_path):
    case = dict(next(c for c in CASES if c["name"] == "paired"))
    m2 = case["inputs"][1].split("\n")
    case["inputs"] = [case["inputs"][0], "\n".join(m2[:4 * 150]) + "\n"]
    want_files, want_err, warnings = R.capture(case["baits"], case["inputs"], case["k"], True)
    assert warnings == ["warning: files had unequal length"]
    files, err = run_case(ctx, tmp_path, case, extra=["-m", "1"])
    assert err == "warning: files had unequal length\n" + want_err
    assert files == want_files


def test_same_name_baits_share_a_file(ctx, tmp_path):
    case = dict(next(c for c in CASES if c["name"] == "k25"))
    case["baits"] = case["baits"].replace(">b1\n", ">b0\n")
    want_files, want_err, _ = R.capture(case["baits"], case["inputs"], case["k"])
    files, err = run_case(ctx, tmp_path, case)
    assert err == want_err
    assert sorted(files) == sorted(want_files)
    for fn in files:
        assert len(files[fn]) == len(want_files[fn]) and sorted(files[fn].split(b"\n")) == sorted(want_files[fn].split(b"\n"))


def _genome(seed, G):
    from zotmer_amd import synth
    return "".join("ACGT"[int(v)] for v in (synth.rnd(seed, 1, np.arange(G, dtype=np.uint64)) & np.uint64(3)))


@pytest.mark.parametrize("K", [1, 12, 24, 25, 31, 32])
def test_random_cases_against_the_restatement(ctx, tmp_path, K):
    from zotmer_amd import synth
    rng = random.Random(1000 + K)
    G = 200000
    g = _genome(7, G)
    baits = []
    for i in range(2000):
        p = rng.randrange(0, G - 150)
        s = g[p:p + rng.randrange(20, 150)]
        if i % 7 == 0:
            s = "A" * rng.randrange(1, 14) + s
        baits.append(">bait%d%s\n%s\n" % (i % 1900, " x" if i % 5 == 0 else "", s))
    reads = synth.read_strings(7, 0, 50000, 100, genome=G, sub_thr=synth.frac32(0.01), n_thr=synth.frac32(0.001))
    for i in range(0, len(reads), 11):
        reads[i] = "A" * 14 + reads[i][14:]
    fq = "".join("@q%d\n%s\n+\n%s\n" % (i, s, "I" * len(s)) for i, s in enumerate(reads))
    case = dict(baits="".join(baits), inputs=[fq], k=K)
    want_files, want_err, _ = R.capture(case["baits"], case["inputs"], K)
    files, err = run_case(ctx, tmp_path, case, extra=["-m", "1"])
    assert err == want_err
    assert sorted(files) == sorted(want_files)
    for fn in files:
        # a duplicate name: the baits sharing a file are written one after the other per batch
        assert sorted(files[fn].split(b"\n")) == sorted(want_files[fn].split(b"\n")), fn


def test_full_size_union_equals_capture_filter(ctx, tmp_path):
    """~5 M reads: the union of what `zot capture -k 25` captured over all baits is exactly the set of reads the
    independent zk_capture_filter keeps with the union bait set, and the per-bait counts add up to the pairs written."""
    from zotmer_amd import synth
    from zotmer_amd.library import capture
    G, N, L = 4000000, 5000000, 150
    g = _genome(11, G)
    rng = random.Random(5)
    baits = []
    for i in range(100):
        p = rng.randrange(0, G - 1000)
        baits.append(("bait%d" % i, g[p:p + 1000]))
    fa = tmp_path / "baits.fa"
    fa.write_text("".join(">%s\n%s\n" % b for b in baits))
    kw = dict(genome=G, sub_thr=synth.frac32(0.005), n_thr=synth.frac32(0.0005))
    d = ctx.synth_reads(11, 0, N, L, **kw)
    m = d.to_host().reshape(N, L + 1)[:, :L]
    rec = np.empty((N, 3 + L + 3 + L + 1), dtype=np.uint8)        # '@q\n' seq '\n+\n' seq '\n'  (the read index is its order)
    rec[:, 0:3] = np.frombuffer(b"@q\n", np.uint8)
    rec[:, 3:3 + L] = m
    rec[:, 3 + L:6 + L] = np.frombuffer(b"\n+\n", np.uint8)
    rec[:, 6 + L:6 + 2 * L] = m
    rec[:, -1] = ord("\n")
    fq = tmp_path / "reads.fastq"
    fq.write_bytes(rec.tobytes())
    del rec
    (tmp_path / "out").mkdir()
    code, err = zot(["capture", "-k", "25", "-P", str(tmp_path / "out"), str(fa), str(fq)])
    assert code == 0
    counts = [int(line.rsplit(": ", 1)[1]) for line in err.strip().split("\n")]
    captured = []
    total = 0
    for i in range(len(baits)):
        p = tmp_path / "out" / ("bait%d.fastq" % i)
        if not counts[i]:
            assert not p.exists()
            continue
        seqs = p.read_bytes().split(b"\n")[1::4]
        assert len(seqs) == counts[i]
        total += counts[i]
        captured.append(seqs)
    assert total == sum(counts) and total > 10000
    # the independent path: zk_capture_filter over the base stream with the sorted both-strand bait 25-mers
    ks = []
    for _, s in baits:
        ks.extend(R.kmers(25, s, True))
    bk = ctx.upload(np.unique(np.array(ks, dtype=np.uint64)))
    out, n_reads, n_kept = ctx.capture_filter(d, 25, bk)
    rows = out.to_host().reshape(N, L + 1)[:, :L]
    kept = ~np.all(rows == ord("N"), axis=1)            # a read without a hit is blanked to all 'N'
    del rows
    assert n_reads == N and n_kept == int(kept.sum())
    got_seqs = set()
    for seqs in captured:
        got_seqs.update(seqs)
    assert got_seqs == {m[i].tobytes() for i in np.nonzero(kept)[0]}
