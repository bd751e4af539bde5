"""
Toy inputs of `zot hgvs-gen` on the genome of tests/_spikein_cases.py: BED files whose zones start at base 0 and end at a
chromosome's last base, cover its run of N and its soft-masked stretch, repeat a name and come out of order; the cases of
tests/golden/g1_hgvsgen.json; and the eight well-separated zones of the round trip through hgvs-index, spikein and hgvs-find.
"""
from tests._spikein_cases import GENOME, SIZES

KINDS = ("sub", "del", "ins", "delins", "dup", "ani", "and")

BED = ("track name=toy\n"
       "chrA\t1000\t1400\tmid1\n"
       "chrA\t0\t40\tfirst\n"
       "chrA\t590\t640\tsoft\n"
       "chrA\t2490\t2550\tenn\n"
       "chrA\t3000\t3000\tenn\n"
       "chrA\t%d\t%d\tlast\n"
       "chrB\t%d\t%d\tlast\n"
       "chrB\t0\t9\ttiny\n"
       "chrB\t1500\t1520\tmid1\n") % (SIZES["chrA"] - 92, SIZES["chrA"] - 1, SIZES["chrB"] - 96, SIZES["chrB"] - 1)
# zones of one and two bases at the ends of the chromosomes: positions 0 and the last one, and fst == lst spellings
BED_EDGES = "chrA\t0\t1\tzero\nchrA\t3000\t3000\tone\nchrB\t%d\t%d\tlast\n" % (SIZES["chrB"] - 2, SIZES["chrB"] - 1)
BED_UNNAMED = "chrB\t100\t200\nchrA\t100\t200\tx\nchrA\t300\t400\n"

ALL = ",".join(KINDS)
GOLDEN_CASES = (
    [dict(name=k, opts=["-S", str(10 + n), "-N", "25", "-t", k], bed=BED) for n, k in enumerate(KINDS)] +
    [dict(name="all", opts=["-S", "20", "-N", "80", "-t", ALL], bed=BED),
     dict(name="weights", opts=["-S", "21", "-N", "40", "-t", "2:sub,0.5:del,ani"], bed=BED),
     dict(name="D1_I3", opts=["-S", "22", "-N", "40", "-t", "delins,and", "-D", "1", "-I", "3"], bed=BED),
     dict(name="D3_I1", opts=["-S", "23", "-N", "40", "-t", "delins,and", "-D", "3", "-I", "1"], bed=BED),
     dict(name="D1.001_I3", opts=["-S", "22", "-N", "40", "-t", "delins,and", "-D", "1.001", "-I", "3"], bed=BED),
     dict(name="D3_I1.001", opts=["-S", "23", "-N", "40", "-t", "delins,and", "-D", "3", "-I", "1.001"], bed=BED),
     dict(name="edges", opts=["-S", "25", "-N", "40", "-t", ALL], bed=BED_EDGES),
     dict(name="long", opts=["-S", "24", "-N", "30", "-t", "dup,delins,del", "-D", "60", "-I", "90", "-U", "120"], bed=BED)])

# the round trip: twelve zones of 41 bases, 400 apart, beyond the run of N; the eight variants of ROUND_SEED -- chosen on the CPU with
# the restatement, the first seed that puts them into eight different zones, so further apart than the flanks of an index, with two
# substitutions and four kinds among them -- and the one wide zone `zot spikein` cuts about 100-fold coverage of them from
ROUND_BED = "".join("chrA\t%d\t%d\tz%d\n" % (2800 + 400 * k, 2840 + 400 * k, k) for k in range(12))
ROUND_TYPES = "sub,del,ins,delins,dup"
ROUND_N = 8
ROUND_SEED = 48
ROUND_SPIKE_BED = "chrA\t2600\t7300\tall\n"
ROUND_SPIKE_N = 2400


def base_at(ch):
    seq = GENOME[ch]
    return lambda lo, hi: seq[lo:hi]
