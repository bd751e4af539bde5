"""
The spectrum measures of `zot dist` on the host: library/measures.py's SPECTRUM applied to sums computed in Python integers and
math.fsum from the golden sets must print what the reference printed (tests/golden/g11_dist_spectrum.json, written by
make_golden_dist_spectrum.py from the reference's own library/dist.py) and lie within the rounding of the reference's loops.

Bounds.  The reference adds one rounded term per counter, n = n_union non-zero ones at most (2 * n_shared for Jensen-Shannon):
its sum s carries a relative error below delta = (n + 8) * 2**-52 (n roundings of 2**-53 for the additions, a few more for the
operations inside a term; the generator used the same delta to admit a value).  Our s is exact or an fsum, divided once.  With
the handful of roundings after the sum (operands at most 2 in size) counted as delta * 1, since delta >= 8 * 2**-52:
    bray.curtis.quant = 1 - 2 s             |ours - ref| <= delta * (2 s + 1)
    kulczynski.quant  = 1 - 0.5 s           |ours - ref| <= delta * (0.5 s + 1)
    whittaker.quant   = 0.5 s               |ours - ref| <= delta * ref          (no subtraction: the error stays relative)
    chord.quant, hellinger.quant = sqrt(R), R = 2 - 2 s:   stated on the radicand, |ours**2 - ref**2| <= delta * (2 s + 2)
                                            (the second delta: the roundings of R, of the two roots and of the two squares)
    jensen.shannon    = sqrt(R), R = 0.5 s: |ours**2 - ref**2| <= delta * (0.5 * sum |term| + R); terms of both signs are
                                            added, so the sum's error is relative to sum |term|, not to s
    jaccard.ab, ochiai.ab, sorensen.ab:     u and v are quotients of exact integers in both implementations and the formulas
                                            are the same operations: equal, bit for bit.
"""
import contextlib
import io
import math

import pytest

from tests import _golden as G
from tests import _spectrum_host as H
from zotmer_amd.library import measures

CASES = G.load_json("g11_dist_spectrum")
NINE = ["bray.curtis.quant", "chord.quant", "hellinger.quant", "jaccard.ab", "jensen.shannon", "kulczynski.quant", "ochiai.ab",
        "sorensen.ab", "whittaker.quant"]


def case_id(c):
    return "%s-%s-k%d%s" % (c["lhs"], c["rhs"], c["k"], "-disjoint" if "prefix_parity" in c else "")


def case_sums(c):
    par = c.get("prefix_parity", [None, None])
    xk, xs, _ = H.golden_spectrum(c["lhs"], c["k"], par[0])
    yk, ys, _ = H.golden_spectrum(c["rhs"], c["k"], par[1])
    return H.host_spectrum_sums(xk, xs, yk, ys)


def bound_ok(name, ours, ref, s, delta):
    """-> (measured difference, bound), on the value or (roots) on the radicand; see the module docstring"""
    cx, cy = s["cx"], s["cy"]
    if name == "bray.curtis.quant":
        return abs(ours - ref), delta * (2 * (s["S_min"] / (cx + cy)) + 1)
    if name == "kulczynski.quant":
        return abs(ours - ref), delta * (0.5 * ((cx + cy) * s["S_min"] / (cx * cy)) + 1)
    if name == "whittaker.quant":
        return abs(ours - ref), delta * ref
    if name == "chord.quant":
        return abs(ours * ours - ref * ref), delta * (2 * (s["S_xy"] / (cx * cy)) + 2)
    if name == "hellinger.quant":
        return abs(ours * ours - ref * ref), delta * (2 * (s["S_sqrt"] / math.sqrt(cx * cy)) + 2)
    if name == "jensen.shannon":
        return abs(ours * ours - ref * ref), delta * (0.5 * s["js_abs"] + ref * ref)
    return abs(ours - ref), 0.0          # the *.ab measures


def test_golden_covers_the_issue():
    assert {c["k"] for c in CASES} == {1, 4, 6, 8}
    assert any(c["lhs"].endswith("k12") and c["rhs"].endswith("k24") for c in CASES)          # unequal shifts
    dis = [c for c in CASES if c["n_shared"] == 0]
    assert len(dis) == 1 and sorted(dis[0]["values"]) == [m for m in NINE if m not in ("jaccard.ab", "sorensen.ab")]
    for c in CASES:
        if c["n_shared"]:
            assert sorted(c["values"]) == NINE


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_measures_match_the_reference(c):
    s = case_sums(c)
    assert s["n_shared"] == c["n_shared"]
    delta = (c["n_union"] + 8) * 2.0 ** -52
    for name, want in sorted(c["values"].items()):
        ours, ref = measures.SPECTRUM[name](s), float.fromhex(want["hex"])
        diff, bound = bound_ok(name, ours, ref, s, delta)
        print("%-18s ours %.17g ref %.17g diff %.3g bound %.3g" % (name, ours, ref, diff, bound))
        assert "%g" % ours == want["g"], name
        assert diff <= bound, (name, ours, ref, diff, bound)


def test_tables():
    """MEASURES as tests/test_host_format.py indexes it, SPECTRUM for exactly the names it marks as vector measures"""
    assert len(measures.MEASURES) == 17
    assert sorted(measures.SPECTRUM) == sorted(m for m, v in measures.MEASURES.items() if v[1]) == NINE
    for m, (desc, vec, fn) in measures.MEASURES.items():
        assert isinstance(desc, str) and (fn is None) == vec


def test_list_output_is_unchanged():
    from zotmer_amd.commands import dist
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        dist.main(["dist", "-M", "list", "8"])
    assert buf.getvalue() == G.load_json("g5_dist")["list"]["stdout"]


def test_disjoint_spectra():
    """no k-mer in common: jaccard.ab and sorensen.ab, 0 / 0 in the reference, are their limit 1; the rest as the reference has them"""
    s = H.host_spectrum_sums([1, 3], [5, 7], [2, 4], [1, 9])
    assert s["n_shared"] == 0
    assert measures.SPECTRUM["jaccard.ab"](s) == 1.0 and measures.SPECTRUM["sorensen.ab"](s) == 1.0
    assert measures.SPECTRUM["ochiai.ab"](s) == 1.0 and measures.SPECTRUM["bray.curtis.quant"](s) == 1.0
    assert measures.SPECTRUM["chord.quant"](s) == math.sqrt(2) and measures.SPECTRUM["hellinger.quant"](s) == math.sqrt(2)
    assert measures.SPECTRUM["jensen.shannon"](s) == 0.0 and measures.SPECTRUM["kulczynski.quant"](s) == 1.0
    assert measures.SPECTRUM["whittaker.quant"](s) == 0.5 * (22 / (12 * 10))


def test_identical_spectra():
    """the clamp under the Hellinger root: S_sqrt / sqrt(cx * cy) may round to just above 1"""
    k, v = [1, 2, 3, 7], [3, 1, 4, 1]
    s = H.host_spectrum_sums(k, v, k, v)
    for m in NINE:          # (chord.quant and whittaker.quant, divided by cx * cy as the reference has them, are not 0 here)
        if m not in ("chord.quant", "whittaker.quant"):
            assert abs(measures.SPECTRUM[m](s)) < 1e-7, m
    s["S_sqrt"] = math.sqrt(s["cx"] * s["cy"]) * (1 + 2.0 ** -52)
    assert measures.SPECTRUM["hellinger.quant"](s) == 0.0


def test_empty_set_is_an_error():
    s = H.host_spectrum_sums([], [], [2, 4], [1, 9])
    for m in NINE:
        with pytest.raises(measures.EmptySpectrum):
            measures.SPECTRUM[m](s)
