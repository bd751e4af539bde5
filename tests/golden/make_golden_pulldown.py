#!/usr/bin/env python3
"""
Capture golden vectors of `zot pulldown` from the reference (drtconway/zotmer at /root/reference).

Runs ONLY in the development container, as tests/golden/make_golden_capture.py does: the reference's own
commands/pulldown.py (with library/{basics,bits,file}.py) is copied to a throw-away directory under /tmp and passed through
the stdlib's lib2to3; docopt is stubbed, and so are library/kmers.py and library/files.py, which pulldown.py imports and
never uses.  The command is driven in-process from the case's directory, with the inputs under the relative names
'in<i>.fastq', and its stdout captured.  What is committed is data only: tests/golden/p1_pulldown.json holds, per case of
tests/_pulldown_cases.py (the seeded generator of the inputs), whether -U was given, the stdout text, and the archive's
members in archive order as [name, index into the case's `digests`], where a digest is the SHA-256 and the size of a
member's uncompressed bytes (many members share one).  The archive's own bytes are never kept: they hold timestamps.
For a case of several file pairs the reference's archive holds the last pair's members only.

Usage:  python3 tests/golden/make_golden_pulldown.py        (rewrites tests/golden/p1_pulldown.json)
"""
import contextlib
import hashlib
import importlib
import io
import json
import os
import shutil
import subprocess
import sys
import zipfile

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
WORK = "/tmp/zot3_pulldown"
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests._pulldown_cases import make_cases  # noqa: E402


def build_derived():
    shutil.rmtree(WORK, ignore_errors=True)
    os.makedirs(WORK + "/stubs")
    shutil.copytree(REF + "/zotmer", WORK + "/zotmer")
    subprocess.check_call(["chmod", "-R", "u+w", WORK])
    files = [WORK + "/zotmer/library/%s.py" % m for m in ("basics", "bits", "file")]
    files += [WORK + "/zotmer/commands/pulldown.py"]
    subprocess.check_call([sys.executable, "-W", "ignore", "-m", "lib2to3", "-w", "-n"] + files,
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with open(WORK + "/zotmer/library/kmers.py", "w") as f:
        f.write("def kmers(*a, **k):\n    raise RuntimeError('not used')\n")
    with open(WORK + "/zotmer/library/files.py", "w") as f:
        f.write("def writeKmers(*a, **k):\n    raise RuntimeError('not used')\n")
    with open(WORK + "/stubs/docopt.py", "w") as f:
        f.write("_next = {}\n\ndef docopt(doc, argv=None, **kw):\n    return dict(_next)\n")
    sys.path.insert(0, WORK + "/stubs")
    sys.path.insert(0, WORK)


def run_pulldown(case, tmp):
    """the reference's pulldown.main on the case's inputs -> (stdout text, [(member name, bytes)] in archive order)"""
    import docopt
    d = os.path.join(tmp, case["name"])
    shutil.rmtree(d, ignore_errors=True)
    os.makedirs(d)
    with open(d + "/baits.fa", "w", newline="") as f:
        f.write(case["baits"])
    if case["up"] is not None:
        with open(d + "/up.fa", "w", newline="") as f:
            f.write(case["up"])
    inputs = []
    for i, text in enumerate(case["inputs"]):
        with open(d + "/in%d.fastq" % i, "w", newline="") as f:
            f.write(text)
        inputs.append("in%d.fastq" % i)
    docopt._next = {"-p": True, "-U": "up.fa" if case["up"] is not None else None, "<baits>": "baits.fa", "<output>": "out.zip",
                    "<input>": inputs}
    mod = importlib.import_module("zotmer.commands.pulldown")
    out = io.StringIO()
    cwd = os.getcwd()
    os.chdir(d)
    try:
        with contextlib.redirect_stdout(out):
            mod.main(["pulldown"])
        members = []
        if os.path.exists("out.zip"):          # no file pair at all would leave no archive
            with zipfile.ZipFile("out.zip") as z:
                for info in z.infolist():
                    assert info.compress_type == zipfile.ZIP_DEFLATED
                    members.append((info.filename, z.read(info)))
    finally:
        os.chdir(cwd)
    return out.getvalue(), members


def main():
    build_derived()
    tmp = WORK + "/runs"
    res = []
    for case in make_cases():
        stdout, members = run_pulldown(case, tmp)
        digests, where, listed = [], {}, []
        for nm, b in members:
            dg = (hashlib.sha256(b).hexdigest(), len(b))
            if dg not in where:
                where[dg] = len(digests)
                digests.append({"sha256": dg[0], "size": dg[1]})
            listed.append([nm, where[dg]])
        res.append({"name": case["name"], "U": case["up"] is not None, "stdout": stdout, "members": listed, "digests": digests})
        print(case["name"], repr(stdout), len(members), "members")
    with open(os.path.join(HERE, "p1_pulldown.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, sort_keys=True) for r in res) + "\n]\n")


if __name__ == "__main__":
    main()
