#!/usr/bin/env python3
"""
Capture golden vectors of `zot mlst` from the reference (drtconway/zotmer).

Runs ONLY where a checkout of the reference is at hand: its commands/mlst.py, library/index.py, library/file.py,
library/container/{__init__,std,vectors}.py and library/{basics,bits,misc,sparse}.py are copied to a throw-away directory
outside the repository and passed through the stdlib's lib2to3, with two further edits that Python 3 needs: tostring() /
fromstring( -> tobytes() / frombytes( in container/vectors.py, and open(self.tfn, 'w') -> 'wb' in container/__init__.py.
docopt and the two modules that read k-mer sets (library/kmers.py, library/files.py) are stubbed, so that the command sees
the k-mers of tests/_mlst_cases.py (the seeded generator of the inputs) without a set file.  buildIndex, index and mlst.main
are the reference's own, driven in-process; the whole container code of the reference runs (nothing had to be captured through
a stub).

What is committed is data only: tests/golden/m1_mlst.json holds per case K, the names, lens, S, T and U as the reference's
index() loads them from the file its buildIndex wrote, the decompressed bytes of each member of that file as the reference's
writer wrote them (base64), and the reference's stdout per sample (the input named "set_<case>_<sample>").

The run also checks
  * that the cases hold what the fixture is for (see `check_classes`) and that the reference calls what the generator expects;
  * that the index written by zotmer_amd/library/legacy.py from the same arrays is loaded by the reference's index() as equal
    to its own, and that legacy.py reproduces the reference's member bytes and reads the reference's file;
  * that the restatement (tests/_mlst_restatement.py) reproduces every array and every line;
  * that an input of another K dies with a TypeError in the reference (mlst.py:41).

Usage:  python3 tests/golden/make_golden_mlst.py <reference checkout>      (rewrites tests/golden/m1_mlst.json)
"""
import base64
import contextlib
import importlib
import io
import json
import os
import shutil
import subprocess
import sys
import tempfile
import zipfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import _mlst_restatement as R  # noqa: E402
from tests._mlst_cases import make_cases  # noqa: E402
from zotmer_amd.library import legacy, mlst as product  # noqa: E402

KMERS_STUB = '''_sets = {}


class kmers:
    def __init__(self, path, mode):
        self.path, self.meta = path, {"K": _sets[path][0]}

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False
'''
FILES_STUB = '''def readKmers(z):
    from zotmer.library.kmers import _sets
    return _sets[z.path][1]
'''


def edit(path, pairs):
    s = open(path).read()
    for a, b in pairs:
        assert a in s, (path, a)
        s = s.replace(a, b)
    with open(path, "w") as f:
        f.write(s)


def build_derived(ref, work):
    os.makedirs(work + "/stubs")
    shutil.copytree(ref + "/zotmer", work + "/zotmer")
    subprocess.check_call(["chmod", "-R", "u+w", work])
    files = [work + "/zotmer/library/%s.py" % m for m in ("basics", "bits", "misc", "sparse", "file", "index")]
    files += [work + "/zotmer/library/container/%s.py" % m for m in ("__init__", "std", "vectors")]
    files += [work + "/zotmer/commands/mlst.py"]
    subprocess.check_call([sys.executable, "-W", "ignore", "-m", "lib2to3", "-w", "-n"] + files,
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    edit(work + "/zotmer/library/container/vectors.py", [("tostring()", "tobytes()"), ("fromstring(", "frombytes(")])
    edit(work + "/zotmer/library/container/__init__.py", [("open(self.tfn, 'w')", "open(self.tfn, 'wb')")])
    with open(work + "/stubs/docopt.py", "w") as f:
        f.write("_next = {}\n\ndef docopt(doc, argv=None, **kw):\n    return dict(_next)\n")
    with open(work + "/zotmer/library/kmers.py", "w") as f:
        f.write(KMERS_STUB)
    with open(work + "/zotmer/library/files.py", "w") as f:
        f.write(FILES_STUB)
    os.environ["TMPDIR"] = work                    # file.tmpfile: the writers' temporary files
    sys.path.insert(0, work + "/stubs")
    sys.path.insert(0, work)


def run_main(opts):
    """the reference's mlst.main -> (stdout, stderr, exit status)"""
    import docopt
    docopt._next = opts
    mod = importlib.import_module("zotmer.commands.mlst")
    out, err, code = io.StringIO(), io.StringIO(), 0
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        try:
            mod.main(["mlst"])
        except SystemExit as e:
            code = e.code
    return out.getvalue(), err.getvalue(), code


def loaded(idx):
    """what KmerIndex holds, as plain lists"""
    return dict(K=int(idx.K), names=list(idx.names), lens=list(idx.lens), S=list(idx.S.xs), T=list(idx.T), U=list(idx.U))


def check_classes(case, got, lines_of):
    """the classes of records and samples the fixture is for; AssertionError if one is missing"""
    rec, K = case["records"], case["K"]
    seqs = {nm: s for text in (t for _, t in case["files"]) for nm, s in R.read_fasta(text)}
    by_tag = {tag: seqs[got["names"][i]] for tag, i in rec.items()}
    assert len(case["files"]) == 2 and all(t.count(">") >= 2 for _, t in case["files"])
    a1, a2, a3 = by_tag["abc_1"], by_tag["abc_2"], by_tag["abc_3"]
    assert len(a1) == len(a2) == len(a3) and all(sum(x != y for x, y in zip(a1, b)) == 1 for b in (a2, a3))
    assert by_tag["abc_1_again"] == a1
    assert by_tag["sub_short"] in by_tag["sub_long"] and len(by_tag["sub_short"]) >= K
    assert len(by_tag["tiny"]) < K and got["lens"][rec["tiny"]] == 0
    assert "N" in by_tag["with_n"] and 0 < got["lens"][rec["with_n"]] < 2 * (len(by_tag["with_n"]) - K + 1)
    assert by_tag["lower_u"].islower() and "u" in by_tag["lower_u"] and got["lens"][rec["lower_u"]] > 0
    assert any(("\n" + by_tag["multi_line"][:17] + "\n") in t for _, t in case["files"])
    assert " " in got["names"][rec["lower_u"]] and got["names"][rec["lower_u"]] == got["names"][rec["lower_u"]].strip()
    names = [s[0] for s in case["samples"]]
    assert {"one_per_locus", "all_but_one", "forward_only", "nothing", "superset"} <= set(names)
    for nm, xs, expect in case["samples"]:
        called = set(lines_of[nm])
        assert {rec[t] for t in expect["called"]} <= called, (case["name"], nm)
        assert not {rec[t] for t in expect["not_called"]} & called, (case["name"], nm)
        assert rec["tiny"] in called                                       # also for the empty sample
    assert not dict((s[0], s[1]) for s in case["samples"])["nothing"]
    assert set(lines_of["superset"]) == set(rec.values())
    assert {rec["abc_1"], rec["abc_1_again"], rec["sub_long"], rec["sub_short"]} <= set(lines_of["twins_and_substring"])


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    work = tempfile.mkdtemp(prefix="zot3_mlst_")
    try:
        build_derived(sys.argv[1], work)
        from zotmer.library import kmers as kmers_stub
        ref_index = importlib.import_module("zotmer.library.index")
        out, Ks = [], set()
        for case in make_cases():
            K, name = case["K"], case["name"]
            Ks.add(K)
            paths = []
            for fn, text in case["files"]:
                paths.append(os.path.join(work, fn))
                with open(paths[-1], "w") as f:
                    f.write(text)
            idx_path = os.path.join(work, name + ".idx")
            text, err, code = run_main({"-X": True, "-K": str(K), "<alleles>": idx_path, "<input>": paths})
            assert (text, err, code) == ("", "", 0), (text, err, code)
            got = loaded(ref_index.index(idx_path))
            assert got["K"] == K and got["T"][0] == 0 and got["T"][-1] == len(got["U"]) and len(got["T"]) == len(got["S"]) + 1
            # the members as the reference's writer wrote them
            with zipfile.ZipFile(idx_path) as z:
                members = {n: z.read(n) for n in z.namelist() if n != "__meta__"}
            assert sorted(members) == sorted(["%d-mers" % K, "offsets", "postings", "lens"])
            widths = {"%d-mers" % K: (8, "S"), "offsets": (4, "T"), "postings": (2, "U"), "lens": (4, "lens")}
            for n, (w, field) in widths.items():
                assert legacy.pack_vector(got[field], w) == members[n], (name, n)
                assert len(members[n]) == 8 + w * len(got[field])
            # the product's reader on the reference's file, the reference's reader on the product's file
            mine = product.read_index_arrays(idx_path)
            assert mine["K"] == K and mine["names"] == got["names"]
            assert all(mine[a].tolist() == got[b] for a, b in (("keys", "S"), ("offs", "T"), ("ids", "U"), ("lens", "lens")))
            own_path = os.path.join(work, name + ".own.idx")
            product.write_index_arrays(own_path, K, got["S"], got["T"], got["U"], got["lens"], got["names"])
            assert loaded(ref_index.index(own_path)) == got, name
            # the restatement
            rs = R.build_index(K, [t for _, t in case["files"]])
            assert rs == got, name
            # the samples
            stdout, lines_of = {}, {}
            for nm, xs, _ in case["samples"]:
                inp = "set_%s_%s" % (name, nm)
                kmers_stub._sets[inp] = (K, xs)
                text, err, code = run_main({"-X": False, "-K": None, "<alleles>": idx_path, "<input>": [inp]})
                assert err == "" and code == 0, (err, code)
                again, _, _ = run_main({"-X": False, "-K": None, "<alleles>": own_path, "<input>": [inp]})
                assert again == text and R.stdout(rs, inp, xs) == text, (name, nm)
                stdout[nm] = text
                lines_of[nm] = [int(l.split("\t")[1]) for l in text.splitlines()]
                assert all(l.split("\t")[0] == inp for l in text.splitlines())
            check_classes(case, got, lines_of)
            # an input of another K: the reference dies while formatting its message (mlst.py:41)
            kmers_stub._sets["other_k"] = (K + 1, [])
            try:
                run_main({"-X": False, "-K": None, "<alleles>": idx_path, "<input>": ["other_k"]})
                raise AssertionError("the reference took an input of another K")
            except TypeError:
                pass
            out.append(dict(got, name=name, members={n: base64.b64encode(b).decode() for n, b in sorted(members.items())}, stdout=stdout))
            print(name, K, "records", len(got["names"]), "S", len(got["S"]), "U", len(got["U"]), "lens", got["lens"])
            print("   members", {n: len(b) for n, b in sorted(members.items())})
        assert Ks == {11, 27, 31}
        with open(os.path.join(HERE, "m1_mlst.json"), "w") as f:
            json.dump(out, f, indent=None, sort_keys=True, separators=(",", ":"))
            f.write("\n")
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
