#!/usr/bin/env python3
"""
Capture golden vectors of `zot fizzle` from the reference (drtconway/zotmer).

Runs ONLY where a checkout of the reference is at hand: its zotmer/ tree is copied to a throw-away directory outside the
repository and commands/fizzle.py and library/*.py are passed through the stdlib's lib2to3; nothing else is edited.  docopt is
stubbed; yaml is PyYAML itself.  The derived module's openFile is replaced by a text-mode open (gzip by suffix): under Python 3
the reference's `gunzip -c` pipe yields bytes, which its readFasta cannot strip and compare.  Its `sig` is replaced by a constant:
recHits' debugging print hashes a list of tuples with it, which multiplies a tuple by 2^63 and dies, under Python 2 as under 3;
the value is only printed.  The reference's main dies in an experiment before it reaches the scan, so what runs here are its
module-level functions, on every case of tests/_fizzle_cases.py:
  * prepareBedFileGene and prepareBedFileGeneTx on the case's gene lists and refGene table (the BED text and stderr);
  * indexBedFiles over the BED of the first, through its own SequenceFactory, written by yaml.safe_dump_all as its main would;
  * recHits (its print swallowed) on both records of every read pair, the windows cut by the reference's kmersWithPosLists and
    the index being the restatement's (the reference builds its own inside main, behind the dead branch).

What is committed is data only: tests/golden/z1_fizzle.json holds per case K, digests of the inputs, the two BED texts and
their warnings, the index text, and per record recHits' answer and hit count.

The run also checks that the restatement (tests/_fizzle_restatement.py) reproduces all of them, window for window, and that the
cases hold what they should: tuples of two and of three exons, records that take one and two turns of the threshold loop, a record
that stays empty, a record with an empty component beside one that answers, answers that name two genes, and an exon that -T
reports.  The scan's table and the -T report cannot come from the reference; the restatement stands for them.

Usage:  python3 tests/golden/make_golden_fizzle.py <reference checkout>      (rewrites tests/golden/z1_fizzle.json)
"""
import contextlib
import glob
import gzip
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

from tests import _fizzle_restatement as R  # noqa: E402
from tests._fizzle_cases import case_digests, fixture_cases, write_case  # noqa: E402


def build_derived(ref, work):
    os.makedirs(work + "/stubs")
    shutil.copytree(ref + "/zotmer", work + "/zotmer")
    subprocess.check_call(["chmod", "-R", "u+w", work])
    files = sorted(glob.glob(work + "/zotmer/library/*.py")) + [work + "/zotmer/commands/fizzle.py"]
    subprocess.check_call([sys.executable, "-W", "ignore", "-m", "lib2to3", "-w", "-n"] + files,
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with open(work + "/stubs/docopt.py", "w") as f:
        f.write("def docopt(doc, argv=None, **kw):\n    raise AssertionError('never called')\n")
    sys.path.insert(0, work + "/stubs")
    sys.path.insert(0, work)


def open_text(fn, mode="r"):
    return gzip.open(fn, mode + "t", encoding="latin-1") if fn.endswith(".gz") else open(fn, mode, encoding="latin-1")


def read(path):
    with open(path, newline="") as f:
        return f.read()


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    work = tempfile.mkdtemp(prefix="zot3_fizzle_")
    try:
        build_derived(sys.argv[1], work)
        mod = importlib.import_module("zotmer.commands.fizzle")
        basics = importlib.import_module("zotmer.library.basics")
        import yaml
        mod.openFile = open_text
        mod.sig = lambda xs: 0
        out = []
        seen = dict(two=0, three=0, one_turn=0, two_turns=0, empty=0, beside=0, two_genes=0, genomic=0, merged=0, warned=0)
        for case in fixture_cases():
            K = case["K"]
            p = write_case(case, work + "/" + case["name"])
            got = {}
            for key, fn, lst in (("bed", mod.prepareBedFileGene, p["gene_list"]), ("bed_tx", mod.prepareBedFileGeneTx, p["tx_list"])):
                err = io.StringIO()
                with contextlib.redirect_stderr(err):
                    fn(lst, p["ref_gene"], work + "/out.bed")
                got[key], got[key + "_err"] = read(work + "/out.bed"), err.getvalue()
            assert (got["bed"], got["bed_err"]) == R.prepare_gene(case["gene_list"], case["ref_gene"]), case["name"]
            assert (got["bed_tx"], got["bed_tx_err"]) == R.prepare_gene_tx(case["tx_list"], case["ref_gene"]), case["name"]
            seen["warned"] += "multiple chromosomes" in got["bed_err"] and "no annotated" in got["bed_err"] and "not found" in got["bed_tx_err"]
            seen["merged"] += got["bed"].count("GA/") < got["bed_tx"].count("GA/")
            with open(work + "/in.bed", "w") as f:
                f.write(got["bed"])
            got["index"] = yaml.safe_dump_all(mod.indexBedFiles(work + "/in.bed", mod.SequenceFactory(p["home"])), default_flow_style=False)
            items = R.index_bed(got["bed"], lambda ch: case["chroms"][ch])
            assert got["index"] == yaml.safe_dump_all(items, default_flow_style=False), case["name"]
            ref = list(yaml.load_all(got["index"], Loader=yaml.BaseLoader))
            assert ref == R.as_loaded(items), case["name"]

            idx, lens = R.tuple_index(K, ref)
            seen["two"] += any(len(t) == 2 for t in idx.values())
            seen["three"] += any(len(t) == 3 for t in idx.values())
            records = []
            pairs = list(zip(R.read_fastq(case["reads"][0]), R.read_fastq(case["reads"][1])))
            for s1, s2 in pairs:
                lf, lr = basics.kmersWithPosLists(K, s1)
                rf, rr = basics.kmersWithPosLists(K, s2)
                mine = R.records_of(K, s1, s2)
                for xps, xs in zip((lf + rr, lr + rf), mine):
                    assert [x for x, _ in xps] == xs, case["name"]
                    with contextlib.redirect_stdout(io.StringIO()):
                        res, n = mod.recHits(idx, xps)
                    drops = []
                    sdx = R.sdx_of(idx, xs)
                    assert (dict(res), n) == R.rec_hits_sdx(sdx, drops), (case["name"], s1, s2)
                    records.append([n, sorted([list(k), v] for k, v in dict(res).items())])
                    seen["one_turn"] += len(drops) == 1 and len(res) > 0
                    seen["two_turns"] += len(drops) == 2 and len(res) > 0
                    seen["empty"] += n > 0 and len(res) == 0
                    seen["beside"] += len(drops) == 0 and len(res) > 0 and sum(dict(res).values()) < n
                    seen["two_genes"] += len({ref[i]["gene"] for k in dict(res) for i in k}) >= 2
            seen["genomic"] += "GB/02" in R.crosstalk(K, ref, lambda ch: case["chroms"][ch])["aliasing-genomic"]
            out.append(dict(name=case["name"], K=K, params=case_digests(case), pairs=len(pairs), records=records, **got))
            print(case["name"], "pairs", len(pairs), "exons", len(ref), "tuples", len(set(idx.values())))
        print(seen)
        assert all(seen.values()), seen
        with open(os.path.join(HERE, "z1_fizzle.json"), "w") as f:
            json.dump(out, f, indent=None, sort_keys=True, separators=(",", ":"))
            f.write("\n")
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
