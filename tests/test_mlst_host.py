"""The host side of `zot mlst`, no GPU: the reference's older container as zotmer_amd/library/legacy.py reads and writes it
(block layout at the sizes where it changes, byte for byte against what the reference's writer wrote: tests/golden/m1_mlst.json,
made by tests/golden/make_golden_mlst.py), the meta's unpickler, and the restatement of the reference's route
(tests/_mlst_restatement.py) against every array and line of the fixture."""
import base64
import io
import json
import os
import pickle
import struct
import sys
import zipfile

import numpy as np
import pytest

from tests import _mlst_restatement as R
from tests._mlst_cases import make_cases
from zotmer_amd.library import legacy, mlst

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "m1_mlst.json")
INPUTS = {c["name"]: c for c in make_cases()}
CASES = [dict(INPUTS[c["name"]], **c) for c in json.load(open(GOLD))]
IDS = [c["name"] for c in CASES]
B = legacy.BLOCK_ITEMS
MEMBERS = lambda c: {"%d-mers" % c["K"]: (8, "S"), "offsets": (4, "T"), "postings": (2, "U"), "lens": (4, "lens")}


def test_the_fixture_covers_the_cases():
    assert sorted(IDS) == sorted(INPUTS) and {c["K"] for c in CASES} == {11, 27, 31}
    assert os.path.getsize(GOLD) < 200 * 1024


# ---- the vectors --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("width", [8, 4, 2])
@pytest.mark.parametrize("n", [0, 1, B - 1, B, B + 1, 2 * B])
def test_vector_round_trip(n, width):
    rng = np.random.default_rng(n + width)
    v = rng.integers(0, 1 << (8 * width - 1), size=n, dtype=np.uint64).astype("u%d" % width)
    if n:
        v[-1] = (1 << (8 * width)) - 1
    data = legacy.pack_vector(v, width)
    blocks = n // B + 1                      # writeGeneric always writes a last block (vectors.py:85-88)
    assert len(data) == 8 * blocks + width * n
    if n % B == 0:
        assert data[-8:] == struct.pack("<Q", 0)          # ... an empty one at the exact multiples and for no items
    if n >= B:
        assert data[:8] == struct.pack("<Q", B * width)
    got = legacy.unpack_vector(data, width, n, "m")
    assert got.dtype.itemsize == width and got.dtype.kind == "u" and np.array_equal(got, v)
    # the reader stops after n items: without the trailing empty block the member reads the same
    if n and n % B == 0:
        assert np.array_equal(legacy.unpack_vector(data[:-8], width, n, "m"), v)


def test_vector_items_are_little_endian():
    assert legacy.pack_vector([0x0102], 2) == struct.pack("<Q", 2) + b"\x02\x01"
    assert legacy.pack_vector([1], 8) == struct.pack("<Q", 8) + b"\x01" + b"\0" * 7
    assert legacy.unpack_vector(struct.pack("<Q", 4) + b"\x04\x03\x02\x01", 4, 1).tolist() == [0x01020304]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_member_bytes_of_the_reference(case):
    for name, (width, field) in MEMBERS(case).items():
        want = base64.b64decode(case["members"][name])
        assert legacy.pack_vector(case[field], width) == want, name
        assert legacy.unpack_vector(want, width, len(case[field]), name).tolist() == case[field]


# ---- the meta -----------------------------------------------------------------------------------------------------------

def test_python2_protocol0_meta_loads():
    # cPickle.dumps({'K': 11, 'kmers': '11-mers', 'names': ['a b', 'c'], '11-mers-N': 134L}) as Python 2 writes it
    data = (b"(dp1\nS'K'\np2\nI11\nsS'kmers'\np3\nS'11-mers'\np4\nsS'names'\np5\n(lp6\nS'a b'\np7\naS'c'\np8\nasS'11-mers-N'\np9\nL134L\ns.")
    assert legacy.load_meta(data) == {"K": 11, "kmers": "11-mers", "names": ["a b", "c"], "11-mers-N": 134}
    # a name outside ASCII comes through as latin-1
    assert legacy.load_meta(b"(dp1\nS'n'\np2\nS'\\xe9'\np3\ns.") == {"n": "\xe9"}


def test_written_meta_is_protocol_2():
    meta = {"K": 27, "names": ["x y"], "lens": 1}
    data = legacy.dump_meta(meta)
    assert data[:2] == b"\x80\x02" and legacy.load_meta(data) == meta


@pytest.mark.parametrize("payload", [b"cos\nsystem\n(S'true'\ntR.", b"c_mlst_probe_module\nthing\n.", pickle.dumps(io.BytesIO, protocol=2),
                                     pickle.dumps({"K": complex(1, 2)}, protocol=2)])
def test_meta_with_a_global_is_refused(payload):
    before = set(sys.modules)
    with pytest.raises(legacy.LegacyError, match="only dict, str, int and list"):
        legacy.load_meta(payload)
    assert set(sys.modules) == before and "_mlst_probe_module" not in sys.modules


def test_meta_that_is_no_dict_or_no_pickle():
    with pytest.raises(legacy.LegacyError):
        legacy.load_meta(pickle.dumps([1, 2], protocol=2))
    with pytest.raises(legacy.LegacyError):
        legacy.load_meta(b"not a pickle")


# ---- the index file -----------------------------------------------------------------------------------------------------

def write_case(path, case, **over):
    f = dict(case, **over)
    mlst.write_index_arrays(str(path), f["K"], f["S"], f["T"], f["U"], f["lens"], f["names"])
    return str(path)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_index_file_round_trip(tmp_path, case):
    p = write_case(tmp_path / "a.idx", case)
    with zipfile.ZipFile(p) as z:
        infos = {i.filename: i for i in z.infolist()}
        assert [i.filename for i in z.infolist()] == ["%d-mers" % case["K"], "offsets", "postings", "lens", "__meta__"]
        assert infos["__meta__"].compress_type == zipfile.ZIP_STORED
        assert all(i.compress_type == zipfile.ZIP_DEFLATED for n, i in infos.items() if n != "__meta__")
        for name in MEMBERS(case):
            assert z.read(name) == base64.b64decode(case["members"][name])
        nm = "%d-mers" % case["K"]
        assert legacy.load_meta(z.read("__meta__")) == {"kmers": nm, "K": case["K"], nm + "-N": len(case["S"]), "T": len(case["T"]),
                                                       "U": len(case["U"]), "lens": len(case["lens"]), "names": case["names"]}
    got = mlst.read_index_arrays(p)
    assert got["K"] == case["K"] and got["names"] == case["names"]
    assert [got[a].tolist() for a in ("keys", "offs", "ids", "lens")] == [case[b] for b in ("S", "T", "U", "lens")]
    assert got["keys"].dtype == np.uint64 and got["ids"].dtype == np.uint32


def rebuild(path, src, change):
    """copy a container, passing every member's bytes through change(name, bytes) (None drops the member)"""
    with zipfile.ZipFile(src) as zin, zipfile.ZipFile(str(path), "w") as zout:
        for i in zin.infolist():
            data = change(i.filename, zin.read(i.filename))
            if data is not None:
                zout.writestr(i.filename, data, compress_type=i.compress_type)
    return str(path)


@pytest.mark.parametrize("member", ["offsets", "postings", "lens", "11-mers"])
def test_truncated_and_missing_members_are_named(tmp_path, member):
    src = write_case(tmp_path / "a.idx", CASES[0])
    assert CASES[0]["K"] == 11
    for cut in (3, 9, 21):
        p = rebuild(tmp_path / ("cut%d.idx" % cut), src, lambda n, d: d[:-cut] if n == member else d)
        with pytest.raises(IOError, match=repr(member)) as e:
            mlst.read_index_arrays(p)
        assert "truncated" in str(e.value)
    p = rebuild(tmp_path / "gone.idx", src, lambda n, d: None if n == member else d)
    with pytest.raises(IOError, match="%r is missing" % member):
        mlst.read_index_arrays(p)


def test_not_an_index(tmp_path):
    p = tmp_path / "x.idx"
    p.write_bytes(b"plain text")
    with pytest.raises(IOError):
        mlst.read_index_arrays(str(p))
    src = write_case(tmp_path / "a.idx", CASES[0])
    q = rebuild(tmp_path / "meta.idx", src, lambda n, d: legacy.dump_meta({"K": 11}) if n == "__meta__" else d)
    with pytest.raises(IOError, match="not a k-mer index"):
        mlst.read_index_arrays(q)


def test_more_than_65536_records_use_postings32(tmp_path):
    n_rec = B + 1
    keys = np.arange(10, 10 + n_rec, dtype=np.uint64)
    offs = np.arange(n_rec + 1, dtype=np.uint32)
    ids = np.arange(n_rec, dtype=np.uint32)[::-1].copy()          # record 65 536 is in the list of the first key
    lens = np.ones(n_rec, dtype=np.uint32)
    names = ["r%d" % i for i in range(n_rec)]
    p = str(tmp_path / "wide.idx")
    mlst.write_index_arrays(p, 13, keys, offs, ids, lens, names)
    with zipfile.ZipFile(p) as z:
        assert "postings32" in z.namelist() and "postings" not in z.namelist()
        assert legacy.load_meta(z.read("__meta__"))["U32"] is True
        assert len(z.read("postings32")) == 2 * 8 + 4 * n_rec
    got = mlst.read_index_arrays(p)
    assert np.array_equal(got["ids"], ids) and got["ids"].max() == B and got["names"] == names
    assert np.array_equal(got["keys"], keys) and np.array_equal(got["offs"], offs) and np.array_equal(got["lens"], lens)
    # 65 536 records still fit 16 bits
    mlst.write_index_arrays(p, 13, keys[:B], offs[:B + 1], ids[1:], lens[:B], names[:B])
    with zipfile.ZipFile(p) as z:
        assert "postings" in z.namelist() and "U32" not in legacy.load_meta(z.read("__meta__"))
    assert np.array_equal(mlst.read_index_arrays(p)["ids"], ids[1:])


# ---- the restatement ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_reproduces_the_fixture(case):
    idx = R.build_index(case["K"], [t for _, t in case["files"]])
    for f in ("K", "names", "lens", "S", "T", "U"):
        assert idx[f] == case[f], f
    assert sorted(case["stdout"]) == sorted(s[0] for s in case["samples"])
    for name, xs, expect in case["samples"]:
        inp = "set_%s_%s" % (case["name"], name)
        assert R.stdout(idx, inp, xs) == case["stdout"][name], name
        called = {int(l.split("\t")[1]) for l in case["stdout"][name].splitlines()}
        assert {case["records"][t] for t in expect["called"]} <= called
        assert not {case["records"][t] for t in expect["not_called"]} & called
        assert case["records"]["tiny"] in called          # a record shorter than K is called for every sample


# ---- the command, before it reaches the device --------------------------------------------------------------------------

def run(args):
    import contextlib
    from zotmer_amd import cli
    out, err = io.StringIO(), io.StringIO()
    code = None
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        try:
            code = cli.main_inner(args)
        except SystemExit as e:
            code = e.code
    return code, out.getvalue(), err.getvalue()


@pytest.mark.parametrize("args", [["mlst"], ["mlst", "only.idx"], ["mlst", "-K", "0", "-X", "a.idx", "a.fa"], ["mlst", "-XK", "33", "a.idx", "a.fa"],
                                  ["mlst", "-K", "x", "-X", "a.idx", "a.fa"], ["mlst", "-Q", "a.idx", "a.fa"]])
def test_bad_arguments_end_before_the_device(args, monkeypatch):
    from zotmer_amd.library import engine
    monkeypatch.setattr(engine, "context", lambda: pytest.fail("the device was touched"))
    code, out, err = run(args)
    assert code == 1 and out == "" and "zot mlst" in err


def test_missing_index_and_several_processes(tmp_path, monkeypatch):
    from zotmer_amd.library import engine
    monkeypatch.setattr(engine, "context", lambda: pytest.fail("the device was touched"))
    code, out, err = run(["mlst", str(tmp_path / "none.idx"), "a.k27"])
    assert code == 1 and out == "" and "none.idx" in err
    monkeypatch.setenv("WORLD_SIZE", "2")
    code, out, err = run(["mlst", "-X", str(tmp_path / "a.idx"), "a.fa"])
    assert code not in (0, None) and "single GPU" in str(code) + err


def test_help_prints_the_deviations():
    code, out, _ = run(["help", "mlst"])
    assert code == 0 and "zot mlst [-XK K] <alleles> <input>..." in out
    for word in ("postings32", "status 1", "1 .. 32", "single GPU"):
        assert word in out, word
