"""How a line of `zot vars` is compared with the fixture captured on another machine (tests/golden/v1_vars.json)."""
import math


def same_number(a, b, noise):
    """a numeric column, as text: equal; or both magnitudes below 100 x noise (noise = the largest value the reference
    returned where the exact one is 0; the factor is the margin for another libm's last-bit differences over a run of adds);
    or within one unit of the second printed significant digit ('%3.2g')"""
    if a == b:
        return True
    x, y = float(a), float(b)
    if abs(x) < 100 * noise and abs(y) < 100 * noise:
        return True
    top = max(abs(x), abs(y))
    return abs(x - y) <= 10.0 ** (math.floor(math.log10(top)) - 1) * (1 + 1e-9)


def same_line(got, want, noise):
    g, w = got.split("\t"), want.split("\t")
    return len(g) == len(w) == 6 and g[:2] == w[:2] and all(same_number(a, b, noise) for a, b in zip(g[2:], w[2:]))


def same_lines(got, want, noise):
    return len(got) == len(want) and all(same_line(a, b, noise) for a, b in zip(got, want))
