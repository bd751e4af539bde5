"""The links of a k-mer list by NumPy brute force (searchsorted over the whole array), and the seeded arbitrary link arrays the
walk is tested on: shared by the host, sanitizer and GPU tests of `zot contigs`."""
import random

import numpy as np

NO_LINK = 0xFFFFFFFF


def np_rc(K, xs):
    x = np.asarray(xs, dtype=np.uint64).copy()
    y = np.zeros_like(x)
    for _ in range(K):
        y = (y << np.uint64(2)) | (np.uint64(3) - (x & np.uint64(3)))
        x >>= np.uint64(2)
    return y


def np_links(K, xs):
    """-> (next u32, rank u32) of an ascending uint64 array"""
    x = np.asarray(xs, dtype=np.uint64)
    m = np.uint64((1 << (2 * K)) - 1)
    y0 = (x << np.uint64(2)) & m
    a = np.searchsorted(x, y0, side="left")
    b = np.searchsorted(x, y0 | np.uint64(3), side="right")
    nxt = np.where(b - a == 1, a, NO_LINK).astype(np.uint32)
    rank = np.searchsorted(x, np_rc(K, x), side="left").astype(np.uint32)
    return nxt, rank


def arbitrary_links(seed):
    """(next, rc, K, min_len): any arrays the walk accepts, not the links of a k-mer set -- chains, cycles, self-loops, links
    into the middle of other chains, marks anywhere in 0 .. n"""
    rng = random.Random(seed)
    n = rng.choice([0, 1, 2, 3, 63, 64, 65, 128]) if seed % 5 == 0 else rng.randint(1, 300)
    p_link = rng.choice([0.3, 0.7, 0.95])
    nxt = [rng.randrange(n) if rng.random() < p_link else NO_LINK for _ in range(n)]
    rc = [rng.randint(0, n) for _ in range(n)]
    K = rng.randint(1, 32)
    min_len = rng.choice([0, 1, K, K + 1, K + 3, 2 * K])
    return nxt, rc, K, min_len
