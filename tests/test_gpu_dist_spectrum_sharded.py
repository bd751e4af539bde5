"""
The spectrum measures of `zot dist` through the multi-process code: eight logical ranks on one GPU
(tests/_logical_ranks_spectrum_gpu.py), and the command with one forced rank through both transports and both owners, against
the reference's printed values (tests/golden/g11_dist_spectrum.json -- admitted only where their %g text survives
(n_shared + 8) * 2**-52 * sum |term| on the two floating-point sums, so another summation order cannot change a digit).
"""
import os
import subprocess
import sys

import pytest

from tests import _golden as G
from zotmer_amd.library import vectors
from zotmer_amd.library.container import KmerSet
from zotmer_amd.library.measures import MEASURES

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CASES = G.load_json("g11_dist_spectrum")
NINE = sorted(m for m, v in MEASURES.items() if v[1])
FILES = ["g3_kmerize_genome_k12", "g3_kmerize_genome_k24", "g4_part0", "g4_part1", "g4_part2"]          # K = 12, 24, 25, 25, 25


def test_spectrum_measures_over_8_logical_ranks_on_one_gpu():
    r = subprocess.run([sys.executable, os.path.join(HERE, "_logical_ranks_spectrum_gpu.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.count("SPECTRUM-RANKS-OK") == 2, r.stdout[-6000:] + r.stderr[-3000:]


def test_dist_all_measures_through_the_distributed_code_with_one_rank(tmp_path):
    """`zot dist -M '*' 8` over five sets of three different K: the spectrum columns are the fixture's text wherever the fixture
    has the pair, the *.qual columns are those of the plain single-GPU run"""
    paths = []
    for name in FILES:
        info, km, ct, _, _ = G.load_case(name)
        p = tmp_path / (name + ".k%d" % info["K"])
        with KmerSet(str(p), "w") as z:
            vectors.write_kmers_and_counts(z, km, ct)
            z.meta.update({"K": info["K"], "kmers": "kmers", "counts": "counts"})
        paths.append(str(p))
    zot = os.path.join(ROOT, "zot")

    def run(env_extra):
        r = subprocess.run([sys.executable, zot, "dist", "-M", "*", "8"] + paths, capture_output=True, text=True, timeout=600,
                           env=dict(os.environ, **env_extra), cwd=str(tmp_path))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        rows = [l.split("\t") for l in r.stdout.splitlines()]
        assert len(rows) == 1 + 10 and all(len(x) == 2 + 17 for x in rows) and rows[0][2:] == sorted(MEASURES)
        return rows

    plain = run({})
    gold = {(c["lhs"], c["rhs"]): c["values"] for c in CASES if c["k"] == 8 and "prefix_parity" not in c}
    name_of = dict(zip(paths, FILES))
    for env in ({"ZOT_FORCE_DIST": "1"}, {"ZOT_FORCE_DIST": "1", "ZOT_OWNER": "hash", "ZOT_COMM": "torch"}):
        rows = run(env)
        head, seen = rows[0], 0
        for row, want in zip(rows[1:], plain[1:]):
            assert row[:2] == want[:2]
            assert [v for h, v in zip(head, row) if h.endswith(".qual")] == [v for h, v in zip(head, want) if h.endswith(".qual")]
            values = gold.get((name_of[row[0]], name_of[row[1]]))
            if values:
                seen += 1
                assert [v for h, v in zip(head, row) if h in NINE] == [values[m]["g"] for m in NINE], (env, row[:2])
        assert seen == 4
