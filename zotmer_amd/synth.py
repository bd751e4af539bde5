"""
Counter-based synthetic read generator.

Every base is a pure function of (seed, read index, position), built on the splitmix64
finaliser, so the numpy version here and the HIP version in csrc/synth.hip produce the
same bytes without sharing any state; tests check the two against each other.

  rnd(seed, tag, i) = mix64(mix64(seed + tag) + i)          (all arithmetic mod 2**64)

Genome-sampled mode: the genome is never stored -- base g of the genome is rnd(seed,1,g) & 3.
Read i starts at rnd(seed,2,i) % (G - L + 1) on strand rnd(seed,3,i) & 1; base j gets a
substitution when the low 32 bits of rnd(seed,4,i*L+j) fall below sub_thr and becomes 'N'
when the high 32 bits fall below n_thr (thresholds are fractions of 2**32).
Uniform mode: base = rnd(seed,6,i*L+j) & 3, with the same 'N' rule.

The device input format ("base stream") is every read followed by one '\n'.
"""
import numpy as np

_GAMMA = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)

DEFAULT_SEED = 20261004


def mix64(z):
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = z + _GAMMA
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        return z ^ (z >> np.uint64(31))


def rnd(seed, tag, i):
    with np.errstate(over="ignore"):
        base = mix64(np.uint64((int(seed) + int(tag)) & 0xFFFFFFFFFFFFFFFF))
        return mix64(base + np.asarray(i, dtype=np.uint64))


def frac32(p):
    """A probability as a threshold on a uniform 32-bit draw."""
    return int(round(p * 4294967296.0))


def reads_matrix(seed, first, count, L, genome=0, sub_thr=0, n_thr=0):
    """uint8[count, L] of ASCII bases for reads first .. first+count-1.
    genome == 0 selects uniform mode; otherwise it is the genome length G (>= L)."""
    i = np.arange(first, first + count, dtype=np.uint64)[:, None]
    j = np.arange(L, dtype=np.uint64)[None, :]
    idx = i * np.uint64(L) + j
    if genome:
        start = rnd(seed, 2, i) % np.uint64(genome - L + 1)
        strand = rnd(seed, 3, i) & np.uint64(1)
        gpos = np.where(strand == 1, start + np.uint64(L - 1) - j, start + j)
        b = rnd(seed, 1, gpos) & np.uint64(3)
        b = np.where(strand == 1, np.uint64(3) - b, b)
        e = rnd(seed, 4, idx)
        if sub_thr:
            hit = (e & np.uint64(0xFFFFFFFF)) < np.uint64(sub_thr)
            alt = (b + np.uint64(1) + rnd(seed, 5, idx) % np.uint64(3)) & np.uint64(3)
            b = np.where(hit, alt, b)
    else:
        b = rnd(seed, 6, idx) & np.uint64(3)
        e = rnd(seed, 4, idx)
    out = np.frombuffer(b"ACGT", dtype=np.uint8)[b.astype(np.intp)]
    if n_thr:
        out = np.where((e >> np.uint64(32)) < np.uint64(n_thr), np.uint8(ord("N")), out)
    return np.ascontiguousarray(out, dtype=np.uint8)


def base_stream(seed, first, count, L, **kw):
    """The device input: uint8[count*(L+1)], each read followed by '\\n'."""
    m = reads_matrix(seed, first, count, L, **kw)
    s = np.full((count, L + 1), ord("\n"), dtype=np.uint8)
    s[:, :L] = m
    return s.reshape(-1)


def read_strings(seed, first, count, L, **kw):
    m = reads_matrix(seed, first, count, L, **kw)
    return [bytes(r).decode() for r in m]


def fastq_text(seed, first, count, L, **kw):
    """FASTQ text '@r<i>\\n<seq>\\n+\\n<I*L>\\n' for the same reads."""
    q = "I" * L
    return "".join("@r%d\n%s\n+\n%s\n" % (first + k, s, q)
                   for k, s in enumerate(read_strings(seed, first, count, L, **kw)))


# ---- synthetic sorted k-mer sets (BASELINE configs 3 and 4); the HIP version is csrc/partition.hip ----------

def set_keys_raw(seed, first, count, key_bits, mul=1, add=0, mod=1 << 62):
    """Element first+i of an affine walk through a pool of `mod` random keys: rnd(seed, 7, (mul*(first+i)+add) % mod)
    masked to key_bits -- distinct pool indices while first+i < mod and gcd(mul, mod) == 1 (a draw without
    replacement).  Unsorted, may hold the odd duplicate value."""
    i = np.arange(first, first + count, dtype=np.uint64)
    with np.errstate(over="ignore"):
        j = (np.uint64(mul) * i + np.uint64(add)) % np.uint64(mod)
    mask = np.uint64((1 << key_bits) - 1) if key_bits < 64 else np.uint64(0xFFFFFFFFFFFFFFFF)
    return rnd(seed, 7, j) & mask


def set_keys(seed, first, count, key_bits, **kw):
    """The sorted distinct keys of set_keys_raw."""
    return np.unique(set_keys_raw(seed, first, count, key_bits, **kw))


def set_counts(seed, keys):
    """Geometric counts (mean 8) in integer arithmetic: successive 3-bit groups of rnd(seed, 8, key) are trials that
    stop with probability 1/8; a word whose 21 groups all fail is re-mixed (at most 8 words)."""
    h = rnd(seed, 8, np.asarray(keys, dtype=np.uint64))
    cnt = np.ones(len(h), dtype=np.uint64)
    done = np.zeros(len(h), dtype=bool)
    for _ in range(8):
        for g in range(21):
            stop = ((h >> np.uint64(3 * g)) & np.uint64(7)) == 0
            newly = stop & ~done
            done |= newly
            cnt += (~done).astype(np.uint64)
        h = mix64(h)
    return cnt


# config 3: two sets of 100 M 50-bit keys, half of them shared = two windows of one key sequence
CONFIG3 = dict(n=100_000_000, key_bits=50, seed=1, first_a=0, first_b=50_000_000)
# config 4: 64 sets of 50 M keys drawn without replacement from a shared pool of 200 M, geometric counts (mean 8);
# set s walks the pool with stride CONFIG4["mul"][s % 8] from offset 3 125 000 * s
CONFIG4 = dict(sets=64, n=50_000_000, pool=200_000_000, key_bits=50, seed=100,
               mul=[1, 3, 7, 11, 13, 17, 19, 23])


def config4_set_args(s, scale=1.0):
    """zk_synth_keys / set_keys arguments of set s of config 4 (scale < 1 shrinks pool and sets together)."""
    n, pool = int(CONFIG4["n"] * scale), int(CONFIG4["pool"] * scale)
    pool |= 1                                             # odd pool size: every stride of the table is coprime to it
    while any(pool % m == 0 for m in CONFIG4["mul"] if m > 1):
        pool += 2
    return dict(seed=CONFIG4["seed"], first=0, count=n, key_bits=CONFIG4["key_bits"], mul=CONFIG4["mul"][s % 8],
                add=(pool // 64) * s, mod=pool)


# The named configurations of BASELINE.json / SURVEY.md section 8(d).
CONFIGS = {
    # name: reads, L, K, genome, sub rate, N rate
    "config1": dict(reads=10_000, L=150, K=25, genome=100_000, sub=0.005, n=0.0005),
    "config2": dict(reads=50_000_000, L=150, K=25, genome=100_000_000, sub=0.005, n=0.0005),
    "config5": dict(reads=300_000_000, L=150, K=31, genome=3_100_000_000, sub=0.005, n=0.0005),
}


# ---- simulated read pairs (`zot spikein`); the HIP version is csrc/spikein.hip -------------------------------
# Integer-only from end to end, on Python ints, so that the host, the tests' restatement and the device agree bit for bit.
# Every draw of pair p is rnd(seed, tag, index); pairs are numbered in output order, so a run cut into any number of device
# calls gives the same bytes.
T_ZONE, T_ALLELE, T_POS, T_LEN, T_STRAND, T_ERR = 16, 17, 18, 19, 20, 21      # the device's draws
T_ANON, T_POP = 22, 23                                                         # the host's: insN / delinsN bases, the -m lottery
_MASK64 = 0xFFFFFFFFFFFFFFFF
IH_MAX = 6 * 65535            # |z| of spike_len_z never exceeds it


def mix64_int(z):
    z = (z + 0x9E3779B97F4A7C15) & _MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    return z ^ (z >> 31)


def rnd_int(seed, tag, i):
    """rnd(seed, tag, i) on Python ints"""
    return mix64_int((mix64_int((int(seed) + int(tag)) & _MASK64) + int(i)) & _MASK64)


def spike_sd_q(I, D):
    """the standard deviation I * D of the fragment length in units of 2^-16, as the device takes it"""
    return int(round(I * D * 65536))


def spike_len_z(seed, p):
    """Irwin-Hall: twelve 16-bit fields of three draws, less their mean: mean 0, standard deviation 2^16 (to 1e-9)"""
    z = -IH_MAX
    for k in range(3):
        r = rnd_int(seed, T_LEN, 3 * p + k)
        z += (r & 0xFFFF) + ((r >> 16) & 0xFFFF) + ((r >> 32) & 0xFFFF) + (r >> 48)
    return z


def spike_frag_len(seed, p, I, sd_q, L):
    """fl = max(I + floor(sd_q * z / 2^32), L + L // 2)"""
    return max(I + ((sd_q * spike_len_z(seed, p)) >> 32), L + L // 2)


def spike_flmax(I, sd_q, L):
    return max(L + L // 2, I + ((sd_q * IH_MAX) >> 32))


def spike_zone_of(seed, n, cum):
    """the zone of draw n: rnd(seed, T_ZONE, n) % T looked up in the inclusive cumulative zone lengths"""
    import bisect
    return bisect.bisect_right(cum, rnd_int(seed, T_ZONE, n) % cum[-1])


# ---- the frame draw of `zot stop`; the HIP version is csrc/stop_frames.hip -----------------------------------
T_STOP = 24


def stop_fraction(seed, g):
    """the 53-bit numerator of read g's uniform draw: u = stop_fraction / 2^53 is an exact double in [0, 1)"""
    return rnd_int(seed, T_STOP, g) >> 11


def stop_draw(seed, g, n):
    """the rank, among the n votes of read g ordered by frame, of the vote whose frame is drawn: floor(u * n)"""
    return (stop_fraction(seed, g) * int(n)) >> 53


# ---- random variants (`zot hgvs-gen`); the HIP version is csrc/hgvs_gen.hip ----------------------------------
# Variant v, numbered in output order, takes its zone from T_ZONE as a pair of `zot spikein` does, and every other draw from
# rnd(seed, tag, an index made of v): the tables below are all the host computes in floating point, once per run.
T_HG_TYPE, T_HG_POS, T_HG_LEN, T_HG_INS, T_HG_MIX, T_HG_BASES, T_HG_ALT = 25, 26, 27, 28, 29, 30, 31
HG_KINDS = ("sub", "del", "ins", "delins", "dup", "ani", "and")       # a row's kind is the index
HG_TRIES = 64                 # position draws of a substitution before the walk round the zone
HG_TABLE_MAX = 65536          # entries of a geometric table: means up to 4574


def hg_type_thresholds(probs):
    """relative probabilities of the seven kinds, in HG_KINDS order -> cumulative thresholds on a 32-bit draw, the last 2^32:
    the kind is the first whose threshold exceeds the draw"""
    total = float(sum(probs))
    out, t = [], 0.0
    for p in probs:
        t += p
        out.append(min(frac32(t / total), 1 << 32))
    last = max(i for i, p in enumerate(probs) if p > 0)
    for i in range(last, len(out)):
        out[i] = 1 << 32
    return out


def hg_geom_table(mean):
    """Q[k] = floor-product approximations of 2^32 (1 - 1/mean)^(k + 1), descending, down to the last positive entry:
    P(X > k) = Q[k - 1] / 2^32 for X = hg_geom(Q, a uniform 32-bit draw).  A mean of 1 gives the empty table.  ValueError
    for a mean below 1, one that is not finite, and one whose table would exceed HG_TABLE_MAX entries."""
    mean = float(mean)
    if not (mean >= 1.0) or mean == float("inf"):
        raise ValueError("a mean length of %r: it must be finite and at least 1" % mean)
    q0 = frac32(1.0 - 1.0 / mean)
    if q0 >= 1 << 32:
        raise ValueError("a mean length of %r is too large" % mean)
    out, q = [], q0
    while q > 0:
        if len(out) == HG_TABLE_MAX:
            raise ValueError("a mean length of %r needs a table of more than %d entries" % (mean, HG_TABLE_MAX))
        out.append(q)
        q = (q * q0) >> 32
    return out


def hg_geom(table, r32):
    """1 + the number of entries of the descending table above r32"""
    lo, hi = 0, len(table)
    while lo < hi:
        mid = (lo + hi) >> 1
        if table[mid] > r32:
            lo = mid + 1
        else:
            hi = mid
    return 1 + lo


def hg_mix_thr(D, I):
    """delins and `and`: the threshold below which a 32-bit draw gives l = 1.  The reference draws l ~ geom(pd), m ~ geom(pi)
    until l > 1 or m > 1, with pd = 1/D, pi = 1/I: P(l = 1 | kept) = pd (1 - pi) / (1 - pd pi).  ValueError when pd pi = 1."""
    pd, pi = 1.0 / float(D), 1.0 / float(I)
    if pd * pi >= 1.0:
        raise ValueError("-D 1 with -I 1 leaves delins nothing to draw: every pair (1, 1) is rejected")
    return min(frac32(pd * (1.0 - pi) / (1.0 - pd * pi)), 1 << 32)


def hg_words(table_ins):
    """W: the 64-bit words that hold the bases of the longest insertion, 1 + hg_geom's largest value, at 32 bases a word"""
    return max(1, (len(table_ins) + 2 + 31) // 32)
