"""
The host walk of `zot contigs` -- zk_contig_walk in zotmer_amd/csrc/hostio.cpp -- built with AddressSanitizer and
UndefinedBehaviorSanitizer into a stand-alone program (tests/san/contig_walk_san_driver.cpp, `make contig_walk_san`) and run on
the CPU.  The driver hands the walk heap blocks of exactly the advertised sizes, so an access one element past an array ends the
run; the results must equal the restatement's.  Nothing here is loaded into Python or touches a GPU.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import _contigs_restatement as R
from tests._contigs_cases import make_cases
from tests._contigs_links import NO_LINK, arbitrary_links, np_links

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "san", "contig_walk_san_driver")
OK, EINVAL, ENOSPC = 0, -1, -4


@pytest.fixture(scope="module")
def driver():
    if not shutil.which("g++") or not shutil.which("make"):
        pytest.skip("g++ / make not available")
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "zotmer_amd", "csrc"), "contig_walk_san"], stdout=subprocess.DEVNULL)
    return DRIVER


def replay(driver, tmp_path, cases):
    """cases: [(next, rc, K, min_len, cap_nodes, cap_contigs)] -> [(code, n_nodes, n_contigs, nodes | None, offs | None)]"""
    words = []
    for nxt, rc, K, ml, cn, cc in cases:
        words += [len(nxt), K & 0xFFFFFFFFFFFFFFFF, ml, cn, cc] + [int(v) for v in nxt] + [int(v) for v in rc]
    src, dst = tmp_path / "cases", tmp_path / "results"
    src.write_bytes(np.array(words, dtype="<u8").tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([driver, str(src), str(dst)], capture_output=True, text=True, env=env, timeout=300)
    assert p.returncode == 0, "sanitizer or driver failure:\n" + p.stdout + p.stderr[-4000:]
    assert p.stdout.startswith("cases %d" % len(cases))
    w = np.frombuffer(dst.read_bytes(), dtype="<u8").tolist()
    out, at = [], 0
    for _ in cases:
        code, nn, nc = w[at] - (1 << 64) if w[at] >> 63 else w[at], w[at + 1], w[at + 2]
        at += 3
        nodes = offs = None
        if code == OK:
            nodes, offs = w[at:at + nn], w[at + nn:at + nn + nc + 1]
            at += nn + nc + 1
        out.append((code, nn, nc, nodes, offs))
    assert at == len(w)
    return out


def test_golden_cases_under_sanitizers(driver, tmp_path):
    cases, want = [], []
    for c in make_cases():
        K, ml = c["K"], 2 * c["K"] if c["l"] is None else c["l"]
        nxt, rank = np_links(K, c["kmers"])
        nodes, offs = R.walk_links(nxt.tolist(), rank.tolist(), K, ml)
        assert [nodes[a:b] for a, b in zip(offs, offs[1:])] == R.walk(K, c["kmers"], ml)
        cases.append((nxt, rank, K, ml, len(nodes), len(offs) - 1))          # exactly what is needed
        want.append((OK, len(nodes), len(offs) - 1, nodes, offs))
    assert replay(driver, tmp_path, cases) == want


def test_arbitrary_links_under_sanitizers(driver, tmp_path):
    cases, want = [], []
    for seed in range(200):
        nxt, rc, K, ml = arbitrary_links(seed)
        nodes, offs = R.walk_links(nxt, rc, K, ml)
        cases.append((nxt, rc, K, ml, len(nodes), len(offs) - 1))
        want.append((OK, len(nodes), len(offs) - 1, nodes, offs))
    assert replay(driver, tmp_path, cases) == want


def test_capacity_edges_and_damage_under_sanitizers(driver, tmp_path):
    cases, want = [], []
    for seed in (3, 7, 11, 12):
        nxt, rc, K, ml = arbitrary_links(seed)
        nodes, offs = R.walk_links(nxt, rc, K, ml)
        nn, nc = len(nodes), len(offs) - 1
        assert nn > 1 and nc > 1
        for cn, cc in ((nn - 1, nc), (nn, nc - 1), (0, 0), (0, nc), (nn, 0)):
            cases.append((nxt, rc, K, ml, cn, cc))
            want.append((ENOSPC, nn, nc, None, None))
        cases.append((nxt, rc, K, ml, nn + 5, nc + 5))
        want.append((OK, nn, nc, nodes, offs))
    cases.append(([], [], 5, 0, 0, 0))                                       # nothing: offs[0] = 0 in a block of one entry
    want.append((OK, 0, 0, [], [0]))
    got = replay(driver, tmp_path, cases)
    assert got == want
    # damaged arrays end with ZK_EINVAL before anything is indexed out of range
    n = 70
    chain = list(range(1, n)) + [NO_LINK]
    damaged = []
    for i, v in ((0, n), (40, n + 1000), (69, 0xFFFFFFFE)):
        bad = list(chain)
        bad[i] = v
        damaged.append((bad, [n] * n, 9, 0, n, n))
    for i, v in ((1, n + 1), (69, 0xFFFFFFFF)):
        bad = [n] * n
        bad[i] = v
        damaged.append((chain, bad, 9, 0, n, n))
    damaged.append((chain, [n] * n, 33, 0, n, n))
    assert [g[0] for g in replay(driver, tmp_path, damaged)] == [EINVAL] * len(damaged)
