#!/usr/bin/env python3
"""
Capture golden vectors of `zot capture` from the reference (drtconway/zotmer at /root/reference).

Runs ONLY in the development container: the reference's own commands/capture.py (with library/{basics,bits,file,reads}.py)
is copied to a throw-away directory under /tmp, passed through the stdlib's lib2to3, docopt / tqdm / yaml are stubbed, and
the command is driven in-process, as tests/golden/make_golden.py does for the other commands.  What is committed is data
only: tests/golden/c1_capture.json holds, per case of tests/_capture_cases.py (the seeded generator of the inputs), the
options, the SHA-256 and size of every output file the reference wrote, and its stderr.

Usage:  python3 tests/golden/make_golden_capture.py        (rewrites tests/golden/c1_capture.json)
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

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
WORK = "/tmp/zot3_capture"
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests._capture_cases import make_cases  # noqa: E402


def build_derived():
    shutil.rmtree(WORK, ignore_errors=True)
    os.makedirs(WORK + "/stubs")
    shutil.copytree(REF + "/zotmer", WORK + "/zotmer")
    subprocess.check_call(["chmod", "-R", "u+w", WORK])
    files = [WORK + "/zotmer/library/%s.py" % m for m in ("basics", "bits", "file", "reads")]
    files += [WORK + "/zotmer/commands/capture.py"]
    subprocess.check_call([sys.executable, "-W", "ignore", "-m", "lib2to3", "-w", "-n"] + files,
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    with open(WORK + "/stubs/docopt.py", "w") as f:
        f.write("_next = {}\n\ndef docopt(doc, argv=None, **kw):\n    return dict(_next)\n")
    with open(WORK + "/stubs/tqdm.py", "w") as f:
        f.write("def tqdm(*a, **k):\n    raise RuntimeError('not used')\n")
    with open(WORK + "/stubs/yaml.py", "w") as f:
        f.write("")
    sys.path.insert(0, WORK + "/stubs")
    sys.path.insert(0, WORK)


def run_capture(case, tmp):
    """the reference's capture.main on the case's inputs -> ({file name: bytes}, stderr text)"""
    import docopt
    d = os.path.join(tmp, case["name"])
    shutil.rmtree(d, ignore_errors=True)
    os.makedirs(d + "/out")
    with open(d + "/baits.fa", "w", newline="") as f:
        f.write(case["baits"])
    inputs = []
    for i, text in enumerate(case["inputs"]):
        p = d + "/in%d.fastq" % i
        with open(p, "w", newline="") as f:
            f.write(text)
        inputs.append(p)
    docopt._next = {"-b": str(case.get("b", 4096)), "-k": str(case["k"]), "-P": d + "/out", "-p": case.get("paired", False),
                    "-v": False, "-z": False, "<sequences>": d + "/baits.fa", "<input>": inputs}
    mod = importlib.import_module("zotmer.commands.capture")
    err = io.StringIO()
    with contextlib.redirect_stderr(err):
        mod.main(["capture"])
    files = {}
    for fn in sorted(os.listdir(d + "/out")):
        with open(os.path.join(d + "/out", fn), "rb") as f:
            files[fn] = f.read()
    return files, err.getvalue().replace(d + "/out", "<P>")


def main():
    build_derived()
    tmp = WORK + "/runs"
    out = []
    for case in make_cases():
        files, err = run_capture(case, tmp)
        rec = {k: v for k, v in case.items() if k not in ("baits", "inputs")}
        rec["files"] = {fn: {"sha256": hashlib.sha256(b).hexdigest(), "size": len(b)} for fn, b in files.items()}
        rec["stderr"] = err
        out.append(rec)
        print(case["name"], {fn: len(b) for fn, b in files.items()})
    with open(os.path.join(HERE, "c1_capture.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
