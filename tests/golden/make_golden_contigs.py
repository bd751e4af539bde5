#!/usr/bin/env python3
"""
Capture golden vectors of `zot contigs` from the reference (drtconway/zotmer).

Runs ONLY where a checkout of the reference is at hand: its commands/contigs.py and library/{basics,bits,sparse,bitvec}.py are
copied to a throw-away directory outside the repository and passed through the stdlib's lib2to3; nothing else is edited.  docopt
and the two modules that read k-mer sets (library/kmers.py, library/files.py) are stubbed, so that the command sees the k-mer
lists of tests/_contigs_cases.py (the seeded generator of the inputs) without a set file.  contigs.main, succ, sparse, bitvec
and everything under them are the reference's own, driven in-process.

What is committed is data only: tests/golden/k1_contigs.json holds per case K, -l, the generator's parameters (with the number
of k-mers and a digest of them) and the reference's stdout.

The run also checks
  * that the restatement (tests/_contigs_restatement.py) reproduces every case byte for byte;
  * that every case with output prints at least 3 contigs, and that across the cases printed paths end for all three reasons:
    no successor, several successors, a seen successor;
  * that at least one case prints other bytes when the restatement leaves the marks at rank(rc x) out (the walk depends on them);
  * that the set which is not closed under reverse complement has n % 64 != 0 and marks that fall at n, that the same kind of
    set with n % 64 == 0 kills the reference with IndexError, and that K = 4 kills it with ValueError (a negative shift count).

Usage:  python3 tests/golden/make_golden_contigs.py <reference checkout>      (rewrites tests/golden/k1_contigs.json)
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

from tests import _contigs_restatement as R  # noqa: E402
from tests._contigs_cases import closed, genome, make_cases  # noqa: E402

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
    for x in _sets[z.path][1]:
        yield x
'''


def build_derived(ref, work):
    os.makedirs(work + "/stubs")
    shutil.copytree(ref + "/zotmer", work + "/zotmer")
    subprocess.check_call(["chmod", "-R", "u+w", work])
    files = [work + "/zotmer/library/%s.py" % m for m in ("basics", "bits", "sparse", "bitvec")]
    files += [work + "/zotmer/commands/contigs.py"]
    subprocess.check_call([sys.executable, "-W", "ignore", "-m", "lib2to3", "-w", "-n"] + files,
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with open(work + "/stubs/docopt.py", "w") as f:
        f.write("_next = {}\n\ndef docopt(doc, argv=None, **kw):\n    return dict(_next)\n")
    with open(work + "/zotmer/library/kmers.py", "w") as f:
        f.write(KMERS_STUB)
    with open(work + "/zotmer/library/files.py", "w") as f:
        f.write(FILES_STUB)
    sys.path.insert(0, work + "/stubs")
    sys.path.insert(0, work)


def run_main(opts):
    """the reference's contigs.main -> (stdout, the exception it died with or None)"""
    import docopt
    docopt._next = opts
    mod = importlib.import_module("zotmer.commands.contigs")
    out, died = io.StringIO(), None
    with contextlib.redirect_stdout(out):
        try:
            mod.main(["contigs"])
        except (IndexError, ValueError) as e:
            died = e
    return out.getvalue(), died


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    work = tempfile.mkdtemp(prefix="zot3_contigs_")
    try:
        build_derived(sys.argv[1], work)
        from zotmer.library import kmers as kmers_stub
        out, reasons, order_matters, Ks = [], set(), False, set()
        for case in make_cases():
            K, name, l = case["K"], case["name"], case["l"]
            Ks.add(K)
            kmers_stub._sets[name] = (K, case["kmers"])
            text, died = run_main({"-l": None if l is None else str(l), "<input>": [name]})
            assert died is None, (name, died)
            ends, dropped = [], []
            paths = R.walk(K, case["kmers"], 2 * K if l is None else l, ends=ends, dropped=dropped)
            assert R.text_of(K, case["kmers"], paths) == text, name
            assert text == "" or text.count(">") >= 3, (name, text.count(">"))
            reasons |= set(ends)
            order_matters = order_matters or R.stdout_text(K, case["kmers"], l, rc_marks=False) != text
            if name == "not_closed":
                assert not closed(K, case["kmers"]) and len(case["kmers"]) % 64 != 0 and dropped and text
            elif name == "l_above_all":
                assert text == ""
            else:
                assert closed(K, case["kmers"]) and text
            if name == "poly_a":
                assert 0 in case["kmers"] and 4 ** K - 1 in case["kmers"]
            if name == "palindromes_k12":
                assert K % 2 == 0 and any(R.rc(K, x) == x for x in case["kmers"])
            out.append(dict(name=name, K=K, l=l, params=case["params"], stdout=text))
            print(name, K, "n", len(case["kmers"]), "contigs", text.count(">"), "ends", sorted(set(ends)), "dropped marks", len(dropped))
        assert reasons == {R.DEAD_END, R.BRANCH, R.SEEN} and order_matters and Ks >= {11, 16, 25, 31, 32}

        # two inputs in one call print both, in order
        a, b = make_cases()[0], make_cases()[1]
        text, died = run_main({"-l": None, "<input>": [a["name"], b["name"]]})
        assert died is None and text == out[0]["stdout"] + out[1]["stdout"]

        # not closed, n a multiple of 64: IndexError (a mark one past the bit vector's last word)
        xs = [x for i, x in enumerate(R.kmers_of(15, genome(103))) if i % 3 != 2][:-40]
        xs = xs[:len(xs) - len(xs) % 64]
        kmers_stub._sets["nc64"] = (15, xs)
        text, died = run_main({"-l": "17", "<input>": ["nc64"]})
        assert isinstance(died, IndexError), died
        # K < 5: sparse.__init__ shifts by 2K - 10
        kmers_stub._sets["k4"] = (4, R.kmers_of(4, genome(1)[:40]))
        text, died = run_main({"-l": None, "<input>": ["k4"]})
        assert isinstance(died, ValueError) and text == "", died
        print("not closed with n % 64 == 0: IndexError; K = 4:", type(died).__name__)

        with open(os.path.join(HERE, "k1_contigs.json"), "w") as f:
            json.dump(out, f, indent=None, sort_keys=True, separators=(",", ":"))
            f.write("\n")
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
