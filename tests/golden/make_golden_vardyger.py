#!/usr/bin/env python3
"""
Capture golden vectors of `zot vardyger` from the reference (drtconway/zotmer).

Runs ONLY where a checkout of the reference is at hand: its zotmer/ tree is copied to a throw-away directory outside the
repository, the trace loop of commands/vardyger.py and the `continue` behind it (lines 395-401: `for (x,y) in rngs:` ... `continue`,
which keep main from ever reaching its caller) are cut out of that copy, and commands/vardyger.py and library/*.py are passed
through the stdlib's lib2to3; nothing else is edited.  docopt (absent) is stubbed by a parser of this one usage, tqdm by a class
that does nothing; yaml is PyYAML itself.

It was the reference's own main that ran: on every case of tests/_vardyger_cases.py its stdout (per sequence the coverage line of
line 376, then the table's lines) and its stderr (the phantom warnings) are recorded.  What is committed is data only:
tests/golden/v1_vardyger.json holds per case K, the options, digests of the inputs, and those lines.

The run also asserts that the restatement (tests/_vardyger_restatement.py) reproduces all of it -- the coverage lines in order, the
rows without their number and the warnings as sorted lists (the reference's order is that of its dicts and sets) -- that no
strict path was chosen among equals, and that the cases hold what they should.

Usage:  python3 tests/golden/make_golden_vardyger.py <reference checkout>      (rewrites tests/golden/v1_vardyger.json)
"""
import contextlib
import glob
import importlib
import io
import json
import os
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import _vardyger_restatement as R  # noqa: E402
from tests._vardyger_cases import digest, fixture_cases, write_case  # noqa: E402

DOCOPT = '''
def docopt(doc, argv=None, **kw):
    opts = {"-A": False, "-a": False, "-k": "24", "-m": "10", "-s": False, "-v": False}
    pos, i = [], 0
    while i < len(argv):
        a = argv[i]
        if a in ("-A", "-a", "-s", "-v"):
            opts[a] = True
        elif a in ("-k", "-m"):
            i += 1
            opts[a] = argv[i]
        else:
            pos.append(a)
        i += 1
    opts["<sequences>"], opts["<input>"] = pos[0], pos[1:]
    return opts
'''
TQDM = '''
class tqdm(object):
    def __init__(self, *a, **kw):
        pass
    def update(self, *a, **kw):
        pass
    def set_postfix(self, *a, **kw):
        pass
    def close(self):
        pass
'''


def build_derived(ref, work):
    os.makedirs(work + "/stubs")
    shutil.copytree(ref + "/zotmer", work + "/zotmer")
    subprocess.check_call(["chmod", "-R", "u+w", work])
    cmd = work + "/zotmer/commands/vardyger.py"
    with open(cmd) as f:
        lines = f.read().split("\n")
    first = lines.index("        for (x,y) in rngs:")
    last = lines.index("        continue", first)
    assert (first, last) == (394, 400) and lines[last + 2].strip() == "fst = {}", (first, last)
    with open(cmd, "w") as f:
        f.write("\n".join(lines[:first] + lines[last + 1:]))
    files = sorted(glob.glob(work + "/zotmer/library/*.py")) + [cmd]
    subprocess.check_call([sys.executable, "-W", "ignore", "-m", "lib2to3", "-w", "-n"] + files, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    for name, text in (("docopt", DOCOPT), ("tqdm", TQDM)):
        with open(work + "/stubs/%s.py" % name, "w") as f:
            f.write(text)
    sys.path.insert(0, work + "/stubs")
    sys.path.insert(0, work)


def split_stdout(lines):
    """-> (coverage lines, table lines without the header, whether the header stood before the first row)"""
    cover = [l for l in lines if l == "" or set(l) <= set(".X")]
    rest = [l for l in lines if not (l == "" or set(l) <= set(".X"))]
    if not rest:
        return cover, [], True
    return cover, rest[1:], rest[0] == R.HEADER


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    work = tempfile.mkdtemp(prefix="zot3_vardyger_")
    try:
        build_derived(sys.argv[1], work)
        mod = importlib.import_module("zotmer.commands.vardyger")
        out = []
        rows_of = {}
        for case in fixture_cases():
            args = write_case(case, work + "/" + case["name"])
            so, se = io.StringIO(), io.StringIO()
            with contextlib.redirect_stdout(so), contextlib.redirect_stderr(se):
                mod.main(args)
            stdout, stderr = so.getvalue().split("\n")[:-1], se.getvalue().split("\n")[:-1]
            cover, rows, header_ok = split_stdout(stdout)
            assert header_ok, case["name"]
            assert [r.split("\t")[0] for r in rows] == [str(i + 1) for i in range(len(rows))], case["name"]

            index = R.Index(case["K"], list(R.read_fasta(case["fasta"])))
            reads = [s for t in case["inputs"] for s in R.read_fastq(t)]
            o = case["opts"]
            ties = []
            mine_cover, mine_rows = R.call(index, R.count_reads(index, reads), int(o[o.index("-m") + 1]) if "-m" in o else 10, "-a" in o, "-s" in o,
                                           ties)
            assert mine_cover == cover, case["name"]
            assert sorted(R.ordered(mine_rows)) == sorted(r.split("\t", 1)[1] for r in rows), case["name"]
            assert sorted(index.warnings) == sorted(stderr), case["name"]
            assert not ties, (case["name"], ties)
            rows_of[case["name"]] = [r.split("\t") for r in rows]
            out.append(dict(name=case["name"], K=case["K"], opts=case["opts"],
                            params=dict(fasta=digest([case["fasta"]]), inputs=digest(case["inputs"]), reads=len(reads)), stdout=stdout, stderr=stderr))
            print(case["name"], "reads", len(reads), "rows", len(rows), "warnings", len(stderr), [r.split("\t")[-1] for r in rows])
        hg = lambda name: [r[-1] for r in rows_of[name]]
        assert hg("u30") == ["GENE1:c.201_230dup"] == hg("u30_strict"), hg("u30")
        assert hg("u31") == [] and hg("u31_all") == ["GENE1:c.201_231dup"]
        assert sorted(hg("u13_all_rolled3")) == ["GENE1:c.%d_%ddup" % (p, p + 12) for p in (200, 201, 202)] and hg("u12_all") == []
        assert len(hg("u48_k32_rolled2")) == 2 and hg("u45_k30_strict") == ["GENE1:c.201_245dup"]
        assert hg("snp_copy") == ["GENE1:c.201_260dup"] == hg("snp_copy_strict")
        assert hg("gap") == ["GENE1:c.201_350dup"] and hg("gap_strict") == []
        assert len(hg("two_depths")) > len(hg("two_depths_m30")) >= 1
        assert {h.split(":")[0] for h in hg("shared")} == {"GENE1", "SHARED"}
        assert any(c["stderr"] for c in out if c["name"] == "phantom") and hg("phantom")
        assert hg("dressed_two_files")
        with open(os.path.join(HERE, "v1_vardyger.json"), "w") as f:
            json.dump(out, f, indent=None, sort_keys=True, separators=(",", ":"))
            f.write("\n")
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
