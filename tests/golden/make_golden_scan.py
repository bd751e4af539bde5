#!/usr/bin/env python3
"""
Capture golden vectors of `zot scan` from the reference (drtconway/zotmer).

Runs ONLY where a checkout of the reference is at hand: its commands/scan.py and library/{basics,bits,misc,sparse,stats,file,
exceptions}.py are copied to a throw-away directory outside the repository and passed through the stdlib's lib2to3; nothing
else is edited.  Stand-ins, because the originals cannot run here:
  * docopt (not installed): returns the options the maker sets;
  * library/kmers.py and library/files.py: a sample is the (meta `acgt`, k-mer list) pair of tests/_scan_cases.py, no set file;
  * library/container/casket.py: keeps the members that scan hands to add_content in memory and serves them back through
    open() -- the converted casket mixes text and bytes under Python 3;
  * the name `array` in scan's module: array.array with the tostring / fromstring that Python 3.9 removed.
scan.main, resolveAll, succ, null, logGammaPInt, chi2 and everything under them are the reference's own, driven in-process: once
with -X per case, once to scan all of the case's samples in one call.

What is committed is data only: tests/golden/s1_scan.json holds per case the bytes the reference handed to the container for
S, T, U and V (hex), the parsed __meta__, and the stdout lines per input.

The run also checks that the restatement (tests/_scan_restatement.py) reproduces the members, the meta data and every line as
text, and prints which branches the cases reached: a line printed, a record with no line, more than one fragment, a link.
Ambiguity codes did not appear: within a fragment consecutive k-mers agree on every base they share, so a position gets
votes for one base only, and fragments are only ever combined by the linking step.  A record whose sample copy has three
substitutions close together prints the sample's bases; with the substitutions spread out it falls into fragments with
uncovered positions between them and prints nothing.
The linking step did not fire: the record "poly A head" (25 A's, then CG) gives a fragment whose first k-mer has the value 6,
below the size of the sample, but a link also needs a fragment whose last k-mer has exactly one successor in the sample and
that successor at exactly that rank; it was not pursued further.

Usage:  python3 tests/golden/make_golden_scan.py <reference checkout>      (rewrites tests/golden/s1_scan.json)
"""
import array
import contextlib
import importlib
import io
import json
import os
import shutil
import subprocess
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import _scan_restatement as R  # noqa: E402
from tests._scan_cases import golden_cases  # noqa: E402

KMERS_STUB = '''import sys

_sets = {}
_opened = []


class kmers:
    def __init__(self, path, mode):
        _opened.append((path, sys.stdout.tell()))
        self.path, self.meta = path, {"acgt": _sets[path][0]}

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False
'''
FILES_STUB = '''def readKmers(z):
    from zotmer.library.kmers import _sets
    return iter(_sets[z.path][1])
'''
CASKET_STUB = '''import io

_files = {}


class casket:
    def __init__(self, fn, mode="r"):
        if mode == "w":
            _files[fn] = []
        self.members = _files[fn]

    def add_content(self, name, data):
        self.members.append((name, data))

    def open(self, name):
        data = [d for n, d in self.members if n == name][-1]
        return io.StringIO(data) if isinstance(data, str) else io.BytesIO(data)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False
'''


class Array(array.array):
    def tostring(self):
        return self.tobytes()

    def fromstring(self, data):
        self.frombytes(data)


def build_derived(ref, work):
    os.makedirs(work + "/stubs")
    shutil.copytree(ref + "/zotmer", work + "/zotmer")
    subprocess.check_call(["chmod", "-R", "u+w", work])
    files = [work + "/zotmer/library/%s.py" % m for m in ("basics", "bits", "misc", "sparse", "stats", "file", "exceptions")]
    files += [work + "/zotmer/commands/scan.py"]
    subprocess.check_call([sys.executable, "-W", "ignore", "-m", "lib2to3", "-w", "-n"] + [f for f in files if os.path.exists(f)],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with open(work + "/stubs/docopt.py", "w") as f:
        f.write("_next = {}\n\ndef docopt(doc, argv=None, **kw):\n    return dict(_next)\n")
    for name, text in (("library/kmers.py", KMERS_STUB), ("library/files.py", FILES_STUB), ("library/container/casket.py", CASKET_STUB),
                       ("library/container/__init__.py", "")):
        with open(work + "/zotmer/" + name, "w") as f:
            f.write(text)
    sys.path.insert(0, work + "/stubs")
    sys.path.insert(0, work)


def run_main(mod, opts):
    import docopt
    docopt._next = opts
    out = io.StringIO()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(io.StringIO()):
        mod.main(["scan"])
    return out.getvalue()


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    work = tempfile.mkdtemp(prefix="zot3_scan_")
    try:
        build_derived(sys.argv[1], work)
        from zotmer.library import kmers as kmers_stub
        from zotmer.library.container import casket as casket_stub
        mod = importlib.import_module("zotmer.commands.scan")
        mod.array = types.SimpleNamespace(array=Array)
        out, events = [], {}
        for case in golden_cases():
            name = case["name"]
            paths = []
            for k, recs in enumerate(case["fasta"]):
                paths.append("%s/%s_%d.fa" % (work, name, k))
                with open(paths[-1], "w") as f:
                    for nm, seq in recs:
                        f.write(">%s\n" % nm)
                        for at in range(0, len(seq), 60):
                            f.write(seq[at:at + 60] + "\n")
            genes = work + "/" + name + ".genes"
            assert run_main(mod, {"-X": True, "-A": False, "<genes>": genes, "<input>": paths}) == ""
            members = dict(casket_stub._files[genes])
            assert [n for n, _ in casket_stub._files[genes]] == ["__meta__", "S", "T", "U", "V"]
            meta = json.loads(members["__meta__"])
            assert meta["K"] == 27

            records = [r for recs in case["fasta"] for r in recs]
            rmeta, S, T, U, V = R.index_build(records)
            assert rmeta == meta, name
            for nm, code, vals in (("S", "Q", S), ("T", "I", T), ("U", "I", U), ("V", "i", V)):
                assert array.array(code, vals).tobytes() == members[nm], (name, nm)
            assert array.array("L").itemsize == 8

            for nm, acgt, X in case["samples"]:
                kmers_stub._sets[nm] = (acgt, X)
            del kmers_stub._opened[:]
            inputs = [nm for nm, _, _ in case["samples"]]
            text = run_main(mod, {"-X": False, "-A": False, "<genes>": genes, "<input>": inputs})
            starts = [at for _, at in kmers_stub._opened] + [len(text)]
            assert [p for p, _ in kmers_stub._opened] == inputs
            stdout = {nm: text[starts[k]:starts[k + 1]].splitlines() for k, nm in enumerate(inputs)}
            want = R.scan_lines(records, [(acgt, X) for _, acgt, X in case["samples"]], events=events)
            for nm, lines in zip(inputs, want):
                assert stdout[nm] == lines, (name, nm, stdout[nm], lines)
            for rec, (gene, in_sample) in case.get("changed", {}).items():
                # a record whose sample copy has substitutions prints the SAMPLE's bases (no ambiguity codes: see the header)
                (ln,) = [l for v in stdout.values() for l in v if l.split("\t")[6] == rec]
                assert ln.split("\t")[7] == in_sample != gene, rec
            out.append(dict(name=name, inputs=inputs, meta=meta, members={n: members[n].hex() for n in "STUV"}, stdout=stdout))
            print(name, "records", len(meta["nms"]), "S", len(S), "entries", len(U), "lines", {k: len(v) for k, v in stdout.items()})
        print("branches reached:", dict(sorted(events.items())), "| link fired:", bool(events.get("link")))
        assert events.get("line") and events.get("no line")
        with open(os.path.join(HERE, "s1_scan.json"), "w") as f:
            json.dump(out, f, indent=None, sort_keys=True, separators=(",", ":"))
            f.write("\n")
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
