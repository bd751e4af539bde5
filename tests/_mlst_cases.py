"""The inputs of the `zot mlst` fixtures (tests/golden/m1_mlst.json): FASTA texts and sample k-mer sets built by a seeded
generator, so that the fixture holds only what the reference made of them.  Read by tests/golden/make_golden_mlst.py and by
the tests.

A case is dict(name, K, files [(file name, FASTA text)], records {tag: record number}, samples [(name, ascending k-mers,
expect)]), `expect` being what the generator knows of the sample: the tags of records that must be called and of records that
must not.  The fixture writer asserts both against the reference's output."""
import random

BASES = "ACGT"
CODE = {"A": 0, "C": 1, "G": 2, "T": 3, "U": 3}


def window_kmers(K, seq, both=True):
    """the k-mers of every window of K bases AaCcGgTtUu, by the definition: the window's value and, with `both`, the value of
    its reverse complement"""
    out = []
    for i in range(len(seq) - K + 1):
        w = seq[i:i + K].upper()
        if any(ch not in CODE for ch in w):
            continue
        x = xb = 0
        for j, ch in enumerate(w):
            x = (x << 2) | CODE[ch]
            xb |= (3 - CODE[ch]) << (2 * j)
        out.append(x)
        if both:
            out.append(xb)
    return out


def _substitute(rng, seq, places):
    s = list(seq)
    for p in places:
        s[p] = rng.choice([b for b in BASES if b != s[p]])
    return "".join(s)


def _wrap(seq, width):
    return "\n".join(seq[i:i + width] for i in range(0, len(seq), width))


def _case(name, K, seed):
    rng = random.Random(seed)
    rand_seq = lambda n: "".join(rng.choice(BASES) for _ in range(n))
    L = K + 30
    recs = []           # (tag, header as written, sequence as written)

    abc = rand_seq(L)
    recs.append(("abc_1", ">abc_1", abc))
    recs.append(("abc_2", ">abc_2", _substitute(rng, abc, [L // 2])))               # one base from abc_1
    recs.append(("abc_3", ">abc_3", _substitute(rng, abc, [L // 2 + 3])))
    recs.append(("abc_1_again", ">abc_1_again", abc))                                # the same sequence twice
    long_ = rand_seq(L + 10)
    recs.append(("sub_long", ">sub_long", long_))
    recs.append(("sub_short", ">sub_short", long_[4:4 + K + 12]))                    # a substring of sub_long
    recs.append(("tiny", ">tiny", rand_seq(K - 1)))                                  # shorter than K: no k-mers
    n_seq = rand_seq(L)
    recs.append(("with_n", ">with_n", n_seq[:K + 5] + "N" + n_seq[K + 6:]))
    low = rand_seq(L)
    recs.append(("lower_u", ">  rna lower case  ", low.lower().replace("t", "u")))     # a name with blanks in it
    multi = rand_seq(L + 7)
    recs.append(("multi_line", ">multi_line", _wrap(multi, 17)))                     # over several lines
    file1 = "".join("%s\n%s\n" % (h, s) for _, h, s in recs)
    n1 = len(recs)
    xyz = rand_seq(L)
    recs.append(("xyz_1", ">xyz_1", xyz))
    recs.append(("xyz_2", ">xyz_2 second file", _substitute(rng, xyz, [7])))
    file2 = "".join("%s\n%s\n" % (h, s) for _, h, s in recs[n1:])
    records = {tag: i for i, (tag, _, _) in enumerate(recs)}
    seq_of = {tag: s.replace("\n", "") for tag, _, s in recs}
    every = sorted(set(x for s in seq_of.values() for x in window_kmers(K, s)))

    def kset(*tags):
        return sorted(set(x for t in tags for x in window_kmers(K, seq_of[t])))

    samples = []
    samples.append(("one_per_locus", kset("abc_2", "xyz_1"), dict(called=["abc_2", "xyz_1", "tiny"], not_called=["abc_1", "abc_3", "xyz_2"])))
    own = [x for x in kset("abc_2") if x not in set(kset("abc_1", "abc_3"))]
    samples.append(("all_but_one", [x for x in kset("abc_2", "xyz_1") if x != own[len(own) // 2]],
                    dict(called=["xyz_1", "tiny"], not_called=["abc_2"])))
    samples.append(("forward_only", sorted(set(window_kmers(K, seq_of["abc_3"], both=False))), dict(called=["tiny"], not_called=["abc_3"])))
    samples.append(("nothing", [], dict(called=["tiny"], not_called=[t for t in records if t != "tiny"])))
    extra = set(rng.getrandbits(2 * K) for _ in range(200))
    samples.append(("superset", sorted(set(every) | extra), dict(called=list(records), not_called=[])))
    samples.append(("twins_and_substring", kset("abc_1", "sub_long", "with_n", "lower_u", "multi_line"),
                    dict(called=["abc_1", "abc_1_again", "sub_long", "sub_short", "with_n", "lower_u", "multi_line", "tiny"],
                         not_called=["abc_2", "abc_3", "xyz_1", "xyz_2"])))
    samples.append(("substring_only", kset("sub_short"), dict(called=["sub_short", "tiny"], not_called=["sub_long"])))
    return dict(name=name, K=K, files=[(name + "_a.fa", file1), (name + "_b.fa", file2)], records=records, samples=samples)


def make_cases():
    return [_case("k11", 11, 1101), _case("k27", 27, 2701), _case("k31", 31, 3101)]
