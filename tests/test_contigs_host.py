"""`zot contigs` without a GPU: the restatement against the reference's fixture (tests/golden/k1_contigs.json), the host walk
(zk_contig_walk, through ctypes) against the fixture, the restatement and a direct loop on arbitrary link arrays, its refusals
and capacities, and the command before it reaches the device."""
import contextlib
import ctypes as C
import io
import json
import os

import numpy as np
import pytest

from tests import _contigs_restatement as R
from tests._contigs_cases import make_cases
from tests._contigs_links import NO_LINK, arbitrary_links, np_links

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = {c["name"]: c for c in json.load(open(os.path.join(ROOT, "tests", "golden", "k1_contigs.json")))}
CASES = make_cases()
IDS = [c["name"] for c in CASES]


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as ge
    ge.build()
    from zotmer_amd import native
    return native


def min_len(case):
    return 2 * case["K"] if case["l"] is None else case["l"]


def test_the_fixture_covers_the_cases():
    assert sorted(GOLD) == sorted(IDS) and {11, 16, 25, 31, 32} <= {c["K"] for c in CASES}
    for c in CASES:
        g = GOLD[c["name"]]
        assert (g["K"], g["l"], g["params"]) == (c["K"], c["l"], c["params"])          # the generator still makes the sets of the capture
        assert g["stdout"] == "" or g["stdout"].count(">") >= 3
    assert GOLD["l_above_all"]["stdout"] == "" and GOLD["l_1"]["l"] == 1 and len(GOLD["not_closed"]["params"]) and \
        GOLD["not_closed"]["params"]["n"] % 64 != 0


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_against_the_fixture(case):
    assert R.stdout_text(case["K"], case["kmers"], case["l"]) == GOLD[case["name"]]["stdout"]


def test_the_walk_depends_on_its_marks_and_ends_for_every_reason():
    ends, differs = set(), False
    for c in CASES:
        e = []
        t = R.stdout_text(c["K"], c["kmers"], c["l"], ends=e)
        ends |= set(e)
        differs = differs or R.stdout_text(c["K"], c["kmers"], c["l"], rc_marks=False) != t
    assert ends == {R.DEAD_END, R.BRANCH, R.SEEN} and differs


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_brute_force_links_are_the_restatements(case):
    nxt, rank = np_links(case["K"], case["kmers"])
    a, b = R.links(case["K"], case["kmers"])
    assert nxt.tolist() == a and rank.tolist() == b


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_walk_reproduces_the_fixture(native, case):
    K, xs = case["K"], case["kmers"]
    nxt, rank = np_links(K, xs)
    nodes, offs = native.contig_walk(nxt, rank, K, min_len(case))
    paths = [nodes[a:b].tolist() for a, b in zip(offs[:-1].tolist(), offs[1:].tolist())]
    assert paths == R.walk(K, xs, min_len(case))
    assert R.text_of(K, xs, paths) == GOLD[case["name"]]["stdout"]
    if case["name"] == "not_closed":
        assert int(rank.max()) == len(xs)                                  # marks at n: dropped


def test_walk_on_arbitrary_links(native):
    kept = 0
    for seed in range(200):
        nxt, rc, K, ml = arbitrary_links(seed)
        nodes, offs = native.contig_walk(nxt, rc, K, ml)
        want_nodes, want_offs = R.walk_links(nxt, rc, K, ml)
        assert nodes.tolist() == want_nodes and offs.tolist() == want_offs, seed
        kept += len(want_offs) - 1
    assert kept > 1000


def raw_walk(native, nxt, rc, K, ml, cap_nodes, cap_contigs):
    lib = native.load()
    nxt, rc = np.asarray(nxt, dtype=np.uint32), np.asarray(rc, dtype=np.uint32)
    nodes, offs = np.full(cap_nodes + 1, 0xAAAAAAAA, dtype=np.uint32), np.full(cap_contigs + 2, 0xAAAAAAAA, dtype=np.uint64)
    nn, nc = C.c_uint64(77), C.c_uint64(77)
    r = lib.zk_contig_walk(nxt.ctypes.data, rc.ctypes.data, len(nxt), K, ml, nodes.ctypes.data, cap_nodes, offs.ctypes.data, cap_contigs,
                           C.byref(nn), C.byref(nc))
    assert nodes[cap_nodes] == 0xAAAAAAAA and offs[cap_contigs + 1] == 0xAAAAAAAA          # nothing past the capacities
    return r, nn.value, nc.value, nodes, offs


def test_walk_capacities(native):
    nxt, rc, K, ml = arbitrary_links(7)
    want_nodes, want_offs = R.walk_links(nxt, rc, K, ml)
    nn, nc = len(want_nodes), len(want_offs) - 1
    assert nn > 10 and nc > 3
    r, a, b, nodes, offs = raw_walk(native, nxt, rc, K, ml, nn, nc)
    assert (r, a, b) == (native.ZK_OK, nn, nc) and nodes[:nn].tolist() == want_nodes and offs[:nc + 1].tolist() == want_offs
    for cn, cc in ((nn - 1, nc), (nn, nc - 1), (0, 0), (nn - 1, nc - 1)):
        r, a, b, _, _ = raw_walk(native, nxt, rc, K, ml, cn, cc)
        assert (r, a, b) == (native.ZK_ENOSPC, nn, nc), (cn, cc)


def test_walk_refuses_damaged_links(native):
    n = 10
    good_next, good_rc = [1, 2, 3, NO_LINK, 5, NO_LINK, 7, 8, 9, NO_LINK], [n] * n
    assert raw_walk(native, good_next, good_rc, 5, 0, n, n)[:3] == (native.ZK_OK, n, 3)
    for i, v in ((0, n), (2, n + 5), (8, 0xFFFFFFFE)):
        bad = list(good_next)
        bad[i] = v
        assert raw_walk(native, bad, good_rc, 5, 0, n, n)[0] == native.ZK_EINVAL, (i, v)
    for i, v in ((1, n + 1), (9, 0xFFFFFFFF)):
        bad = list(good_rc)
        bad[i] = v
        assert raw_walk(native, good_next, bad, 5, 0, n, n)[0] == native.ZK_EINVAL, (i, v)
    for K in (0, 33, -1):
        assert raw_walk(native, good_next, good_rc, K, 0, n, n)[0] == native.ZK_EINVAL
    with pytest.raises(native.ZotkError):
        native.contig_walk([n], [0], 5, 0)


def test_walk_of_nothing(native):
    r, nn, nc, _, offs = raw_walk(native, [], [], 5, 0, 0, 0)
    assert (r, nn, nc) == (native.ZK_OK, 0, 0) and offs[0] == 0
    nodes, offs = native.contig_walk([], [], 5, 10)
    assert len(nodes) == 0 and offs.tolist() == [0]


def test_a_short_path_keeps_its_marks(native):
    # 0 -> 1 -> 2 is too short for min_len and goes, but its marks stay: 1, 2 and rc marks 4 start nothing; 3 starts a path alone
    nxt, rc = [1, 2, NO_LINK, NO_LINK, NO_LINK], [5, 4, 5, 5, 5]
    nodes, offs = native.contig_walk(nxt, rc, 3, 6)                         # 3 nodes + 2 = 5 < 6
    assert nodes.tolist() == [] and offs.tolist() == [0]
    nodes, offs = native.contig_walk(nxt, rc, 3, 3)                         # every path is kept: 4 was marked by node 1
    assert nodes.tolist() == [0, 1, 2, 3] and offs.tolist() == [0, 3, 4]


# ---- the command, before it reaches the device ------------------------------------------------------------------------------

def run(args):
    from zotmer_amd import cli
    out, err = io.StringIO(), io.StringIO()
    code = None
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        try:
            code = cli.main_inner(args)
        except SystemExit as e:
            code = e.code
    return code, out.getvalue(), err.getvalue()


@pytest.mark.parametrize("args", [["contigs"], ["contigs", "-l"], ["contigs", "-l", "30"], ["contigs", "-l", "3.5", "a.k"],
                                  ["contigs", "-l", "many", "a.k"], ["contigs", "-x", "a.k"], ["contigs", "-l", "", "a.k"]])
def test_bad_arguments_end_before_the_device(args, monkeypatch):
    from zotmer_amd.library import engine
    monkeypatch.setattr(engine, "context", lambda: pytest.fail("the device was touched"))
    code, out, err = run(args)
    assert code == 1 and out == "" and "zot contigs [-l LEN] <input>..." in err


def test_good_arguments_parse():
    from zotmer_amd.commands import contigs as cmd
    assert cmd.parse(["a.k"]) == (None, ["a.k"])
    assert cmd.parse(["-l", "40", "a.k", "b.k"]) == (40, ["a.k", "b.k"])
    assert cmd.parse(["a.k", "-l7"]) == (7, ["a.k"])
    assert cmd.parse(["-l", "-5", "a.k"]) == (-5, ["a.k"])
    from zotmer_amd.library import debruijn
    assert [debruijn.min_length(11, l) for l in (None, 1, -5, 100)] == [22, 1, 0, 100]


def test_several_processes_are_refused(monkeypatch):
    from zotmer_amd.library import engine
    monkeypatch.setattr(engine, "context", lambda: pytest.fail("the device was touched"))
    monkeypatch.setenv("WORLD_SIZE", "2")
    code, out, err = run(["contigs", "a.k"])
    assert code not in (0, None) and "single GPU" in str(code) + err


def test_too_many_kmers_are_refused():
    from zotmer_amd.library import debruijn

    class Huge:
        n = (1 << 32) - 1
    with pytest.raises(debruijn.TooManyKmers, match="32 bits"):
        debruijn.contigs_text(None, Huge(), 25)
    assert debruijn.MAX_KMERS == (1 << 32) - 2


def test_help_prints_the_deviations():
    code, out, _ = run(["help", "contigs"])
    assert code == 0 and "zot contigs [-l LEN] <input>..." in out
    for word in ("not closed under reverse complement", "IndexError", "multiple of 64", "K < 5", "2^32 - 1", "not an integer", "single GPU"):
        assert word in out, word
    code, out, _ = run(["help"])
    assert "\tcontigs\n" in out
