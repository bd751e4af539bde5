#!/usr/bin/env python3
"""
Capture golden vectors of `zot stop` from the reference (drtconway/zotmer).

Runs ONLY where a checkout of the reference is at hand: its zotmer/ tree is copied to a throw-away directory outside the
repository and commands/stop.py and library/{basics,bits,misc,file}.py are passed through the stdlib's lib2to3; nothing else is edited.
docopt, yaml and zotmer.library.prot (which the reference does not have: its stop.py dies on import; nucToAa3 is never called)
are stubbed.  The reference's OWN main runs on every case of tests/_stop_cases.py, with two hooks around it:
  * readFastq is wrapped to count the reads, so that the ordinal g of the read being processed is known;
  * random.random returns u(seed, g) = (rnd(seed, T_STOP, g) >> 11) / 2^53, the draw this project defines (zotmer_amd/synth.py)
    -- an exact double, which the reference's `v < pv; v -= pv` walk turns into a frame.
What main prints is recorded, sorted.

What is committed is data only: tests/golden/s1_stop.json holds per case K, the seed, digests of the inputs, the number of
lines whose nearest k-mer is tied, and the lines.

The run also checks
  * that the restatement (tests/_stop_restatement.py) reproduces the first four columns and the name of every line, and the
    nearest k-mer wherever the minimum is untied;
  * that at most one line in ten of every case is tied;
  * that some case has known lines and some novel lines, negative offsets, hits in both orientations, and a read with two or
    more frames whose draw picks a frame other than the first.

Usage:  python3 tests/golden/make_golden_stop.py <reference checkout>      (rewrites tests/golden/s1_stop.json)
"""
import contextlib
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

from tests import _stop_restatement as R  # noqa: E402
from tests._stop_cases import digest, fixture_cases, write_case  # noqa: E402
from zotmer_amd import synth  # noqa: E402


def build_derived(ref, work):
    os.makedirs(work + "/stubs")
    shutil.copytree(ref + "/zotmer", work + "/zotmer")
    subprocess.check_call(["chmod", "-R", "u+w", work])
    files = [work + "/zotmer/library/%s.py" % m for m in ("basics", "bits", "misc", "file")] + [work + "/zotmer/commands/stop.py"]
    subprocess.check_call([sys.executable, "-W", "ignore", "-m", "lib2to3", "-w", "-n"] + files,
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with open(work + "/stubs/docopt.py", "w") as f:
        f.write("_next = {}\n\ndef docopt(doc, argv=None, **kw):\n    return dict(_next)\n")
    with open(work + "/stubs/yaml.py", "w") as f:
        f.write("")
    with open(work + "/zotmer/library/prot.py", "w") as f:
        f.write("def nucToAa3(x):\n    raise AssertionError('never called')\n")
    sys.path.insert(0, work + "/stubs")
    sys.path.insert(0, work)


class Draw:
    """stands in for the module `random` inside the reference's stop.py"""

    def __init__(self):
        self.seed_value, self.g, self.calls = None, -1, 0

    def seed(self, v):
        assert v == 17

    def random(self):
        self.calls += 1
        return synth.stop_fraction(self.seed_value, self.g) / 9007199254740992.0


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    work = tempfile.mkdtemp(prefix="zot3_stop_")
    try:
        build_derived(sys.argv[1], work)
        mod = importlib.import_module("zotmer.commands.stop")
        import docopt
        draw = Draw()
        mod.random = draw
        read_fastq = mod.readFastq

        def counting(f):
            for rd in read_fastq(f):
                draw.g += 1
                yield rd
        mod.readFastq = counting

        out, seen = [], dict(known=0, novel=0, negative=0, fwd=0, rev=0, later_frame=0)
        for case in fixture_cases():
            K, S = case["K"], case["S"]
            args = write_case(case, work + "/" + case["name"])
            docopt._next = {"-k": str(K), "-r": args[5], "-v": False, "<input>": args[6:]}
            draw.seed_value, draw.g = S, -1
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                mod.main(["stop"])
            key = lambda line: (line.split("\t")[:4], line.split("\t")[5])
            got = sorted(buf.getvalue().split("\n")[:-1], key=key)

            index = R.Index(K, R.read_fasta(case["fasta"]))
            reads = [s for t in case["inputs"] for s in R.read_fastq(t)]
            assert draw.g + 1 == len(reads), case["name"]
            rows = R.rows(index, R.count_stops(index, reads, S))
            mine = sorted(((R.line_of(K, r), r[6]) for r in rows), key=lambda m: key(m[0]))
            assert len(mine) == len(got), (case["name"], len(mine), len(got))
            tied = 0
            for (line, is_tied), ref_line in zip(mine, got):
                a, b = line.split("\t"), ref_line.split("\t")
                assert a[:4] == b[:4] and a[5] == b[5], (case["name"], line, ref_line)
                if is_tied:
                    tied += 1
                else:
                    assert a[4] == b[4], (case["name"], line, ref_line)
            assert 10 * tied <= len(got), (case["name"], tied, len(got))
            for g, seq in enumerate(reads):
                frames, _ = R.frames_of(index, seq)
                if not frames:
                    continue
                order = sorted(frames)
                drawn = R.pick(frames, synth.stop_draw(S, g, sum(frames.values())))
                seen["negative"] += drawn[1] < 0
                seen["rev" if drawn[2] else "fwd"] += 1
                seen["later_frame"] += len(order) > 1 and drawn != order[0]
            seen["known"] += sum(l.startswith("known") for l in got)
            seen["novel"] += sum(l.startswith("novel") for l in got)
            out.append(dict(name=case["name"], K=K, S=S, params=dict(fasta=digest([case["fasta"]]), inputs=digest(case["inputs"]),
                                                                      reads=len(reads)), tied=tied, lines=sorted(got)))
            print(case["name"], "reads", len(reads), "lines", len(got), "tied", tied)
        print(seen)
        assert all(seen.values()), seen
        with open(os.path.join(HERE, "s1_stop.json"), "w") as f:
            json.dump(out, f, indent=None, sort_keys=True, separators=(",", ":"))
            f.write("\n")
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
