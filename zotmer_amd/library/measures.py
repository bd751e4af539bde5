"""
Distances between k-mer sets from the three counts a = |X & Y|, b = |X \\ Y|, c = |Y \\ X|
(the GPU's zk_split).  Reference: zotmer/library/dist.py:17-239 (set form of each measure, formulas
from arXiv 1604.02412 table 1) and the registry in zotmer/commands/dist.py:59-92.

Each formula keeps the reference's operation order, so the doubles are the same bit for bit.
The "quant" / "ab" / jensen.shannon entries are measures over k-mer SPECTRA, vectors of 4**K counters
in the reference (the vec=True branches of zotmer/library/dist.py).  Every term of every one of them is
zero unless the k-mer occurs in both spectra, so they are functions of a few sums over the shared
k-mers (the GPU's zk_spectrum_sums) and of the two totals: SPECTRUM below.  MEASURES keeps them as
listed names without a function.
"""
import math


def _bray_curtis(a, b, c):      # dist.py:40-41 (sorensen :209-210 is the same expression)
    return float(b + c) / float(2 * a + b + c)


def _chord(a, b, c):            # dist.py:67-68 (hellinger :93-94 is the same expression)
    return math.sqrt(2 * (1 - a / math.sqrt((a + b) * (a + c))))


def _jaccard(a, b, c):          # dist.py:112-113
    return float(b + c) / float(a + b + c)


def _kulczynski(a, b, c):       # dist.py:168-172
    a, b, c = float(a), float(b), float(c)
    return 1 - 0.5 * (a / (a + b) + a / (a + c))


def _ochiai(a, b, c):           # dist.py:190-191
    return 1 - a / math.sqrt((a + b) * (a + c))


def _whittaker(a, b, c):        # dist.py:235-239
    a, b, c = float(a), float(b), float(c)
    return 0.5 * (b / (a + b) + c / (a + c) + abs(a / (a + b) - a / (a + c)))


# name -> (description, is_vector, function of (a, b, c) or None)      commands/dist.py:59-92
MEASURES = {
    "bray.curtis.quant": ("Quantative Bray.Curtis distance", True, None),
    "bray.curtis.qual": ("Qualitative Bray.Curtis distance", False, _bray_curtis),
    "chord.quant": ("Quantative Chord distance", True, None),
    "chord.qual": ("Qualitative Chord distance", False, _chord),
    "hellinger.quant": ("Quantative Hellinger distance", True, None),
    "hellinger.qual": ("Qualitative Hellinger distance", False, _chord),
    "jaccard.ab": ("Abundance.based Jaccard distance", True, None),
    "jaccard.qual": ("Qualitative Jaccard distance", False, _jaccard),
    "jensen.shannon": ("Jensen.Shannon distance", True, None),
    "kulczynski.quant": ("Quantative Kulczynski distance", True, None),
    "kulczynski.qual": ("Qualitative Kulczynski distance", False, _kulczynski),
    "ochiai.ab": ("Abundance.based Ochiai distance", True, None),
    "ochiai.qual": ("Qualitative Ochiai distance", False, _ochiai),
    "sorensen.ab": ("Abundance.based Sorensen distance", True, None),
    "sorensen.qual": ("Qualitative Sorensen distance", False, _bray_curtis),
    "whittaker.quant": ("Quantative Whittaker distance", True, None),
    "whittaker.qual": ("Qualitative Whittaker distance", False, _whittaker),
}


# ---- spectrum measures --------------------------------------------------------------------------------
# `s` is a mapping with the exact integers cx, cy (the totals of the two spectra), S_min = sum of min(x, y), X_shared / Y_shared
# = sum of x / of y over the k-mers present in both, S_xy = sum of x * y, and the doubles S_sqrt = sum of sqrt(x * y) and S_js =
# sum of the two Jensen-Shannon terms of dist.py:138-139.  The reference adds up one rounded quotient per counter; here each
# sum is exact (or, for the two doubles, accumulated once) and divided once: one rounding per operation written below.

class EmptySpectrum(ValueError):
    """a set without k-mers has no spectrum to compare (the reference divides by zero)"""


def _totals(s):
    if s["cx"] == 0 or s["cy"] == 0:
        raise EmptySpectrum("a k-mer set with no k-mers has no spectrum")
    return s["cx"], s["cy"]


def _q_bray_curtis(s):          # dist.py:29-38
    cx, cy = _totals(s)
    return 1 - 2 * (s["S_min"] / (cx + cy))


def _q_chord(s):                # dist.py:56-65
    cx, cy = _totals(s)
    return math.sqrt(2 - 2 * (s["S_xy"] / (cx * cy)))


def _q_hellinger(s):            # dist.py:82-91; identical spectra leave 2 - 2 * (1 +- rounding): clamped, the reference raises or not
    cx, cy = _totals(s)
    return math.sqrt(max(0.0, 2 - 2 * (s["S_sqrt"] / math.sqrt(cx * cy))))


def _q_kulczynski(s):           # dist.py:156-166
    cx, cy = _totals(s)
    return 1 - 0.5 * ((cx + cy) * s["S_min"] / (cx * cy))


def _q_whittaker(s):            # dist.py:224-233: the sum of |x - y| is cx + cy - 2 * S_min; the cx * cy denominator is the reference's
    cx, cy = _totals(s)
    return 0.5 * ((cx + cy - 2 * s["S_min"]) / (cx * cy))


def _uv(s):                     # dist.decompose, dist.py:267-280
    cx, cy = _totals(s)
    return float(s["X_shared"]) / float(cx), float(s["Y_shared"]) / float(cy)


def _ab_jaccard(s):             # dist.py:108-110; disjoint spectra: 0 / 0 in the reference, the limit 1 here
    u, v = _uv(s)
    if u == 0 and v == 0:
        return 1.0
    return 1 - u * v / (u + v - u * v)


def _ab_ochiai(s):              # dist.py:186-188
    u, v = _uv(s)
    return 1 - math.sqrt(u * v)


def _ab_sorensen(s):            # dist.py:205-207; disjoint spectra as jaccard.ab
    u, v = _uv(s)
    if u == 0 and v == 0:
        return 1.0
    return 1 - 2 * u * v / (u + v)


def _jensen_shannon(s):         # dist.py:127-140: only k-mers present in both spectra contribute
    _totals(s)
    return math.sqrt(0.5 * s["S_js"])


# name -> function of the sums; the nine names MEASURES marks as vector measures
SPECTRUM = {
    "bray.curtis.quant": _q_bray_curtis,
    "chord.quant": _q_chord,
    "hellinger.quant": _q_hellinger,
    "jaccard.ab": _ab_jaccard,
    "jensen.shannon": _jensen_shannon,
    "kulczynski.quant": _q_kulczynski,
    "ochiai.ab": _ab_ochiai,
    "sorensen.ab": _ab_sorensen,
    "whittaker.quant": _q_whittaker,
}

