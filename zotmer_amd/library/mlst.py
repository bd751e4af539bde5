"""
`zot mlst` on the device (zotmer/commands/mlst.py, zotmer/library/index.py): which alleles of a FASTA database have all
their k-mers in a k-mer set?

The reference builds, in Python dictionaries, S = the sorted distinct K-mers of both strands of every FASTA record, T = CSR
offsets and U = the ascending record numbers per k-mer, with lens[i] = the number of distinct k-mers of record i
(index.py:67-125), and stores them in its older container (library/legacy.py).  Per input set it starts a counter per record
at lens and takes one off for every (k-mer of the set, record listing it) pair; the records left at zero are printed
(mlst.py:45-54).  Here S, T, U are a bait table built on the device (zk_bait_table_build), lens is zk_bait_record_sizes, and
the counting is one pass of zk_bait_tally over the set (csrc/allele_tally.hip): a record is complete when its hits equal its
lens.  A record shorter than K has lens 0 and is complete for every set, as in the reference.
"""
import numpy as np

from zotmer_amd.library import legacy, seqio

DEFAULT_K = 27                      # mlst.py:27
U16_RECORDS = 1 << 16               # array('H') holds record numbers below this (index.py:110)


class BadIndex(IOError):
    pass


def fasta_records(fasta_paths):
    """the records of all files in order (index.py:76-79) -> (names, sequences as bytes)"""
    names, seqs = [], []
    for path in fasta_paths:
        for nm, seq in seqio.fasta_records(path):
            names.append(nm)
            seqs.append(seq)
    return names, seqs


def build_index(ctx, K, fasta_paths):
    """buildIndex (index.py:67-115) -> (BaitTable, names): one base stream with one '\\n' per record"""
    names, seqs = fasta_records(fasta_paths)
    stream = b"".join(s + b"\n" for s in seqs)
    table = ctx.bait_table(ctx.upload_stream(stream), K)
    assert table.n_records == len(names)
    return table, names


# ---- the file (host only) ---------------------------------------------------------------------------------------------------

def write_index_arrays(path, K, keys, offs, ids, lens, names):
    """index.py:117-125: the members '<K>-mers', 'offsets', 'postings', 'lens' and the meta.  With more than 65 536 records the
    postings are 32 bits wide, in a member 'postings32', and meta['U32'] is True (the reference cannot build such an index)."""
    nm = "%d-mers" % K
    meta = {"kmers": nm, "K": int(K), nm + "-N": int(len(keys)), "T": int(len(offs)), "U": int(len(ids)), "lens": int(len(lens)),
            "names": [str(n) for n in names]}
    wide = len(lens) > U16_RECORDS
    if wide:
        meta["U32"] = True
    legacy.write_container(path, meta, [(nm, keys, 8), ("offsets", offs, 4),
                                        ("postings32", ids, 4) if wide else ("postings", ids, 2), ("lens", lens, 4)])


def read_index_arrays(path):
    """KmerIndex.__init__ (index.py:37-47) -> dict(K, keys u64, offs u32, ids u32, lens u32, names)"""
    with legacy.Reader(path) as z:
        m = z.meta
        try:
            K, nm = int(m["K"]), m["kmers"]
            n_keys, n_offs, n_ids, n_lens, names = int(m[nm + "-N"]), int(m["T"]), int(m["U"]), int(m["lens"]), list(m["names"])
        except (KeyError, TypeError, ValueError) as e:
            raise BadIndex("%s: not a k-mer index: its meta lacks %s" % (path, e))
        if n_offs != n_keys + 1 or len(names) != n_lens:
            raise BadIndex("%s: a damaged index: %d k-mers with %d offsets, %d names with %d lens" % (path, n_keys, n_offs, len(names), n_lens))
        keys = z.vector(nm, 8, n_keys)
        offs = z.vector("offsets", 4, n_offs)
        ids = z.vector("postings32", 4, n_ids) if m.get("U32") else z.vector("postings", 2, n_ids).astype(np.uint32)
        lens = z.vector("lens", 4, n_lens)
    return dict(K=K, keys=keys, offs=offs, ids=ids, lens=lens, names=[str(n) for n in names])


# ---- the file <-> the device ------------------------------------------------------------------------------------------------

def write_index(path, table, names):
    """the table's arrays downloaded, lens from zk_bait_record_sizes"""
    ctx = table.ctx
    keys, offs, ids = (a.to_host() for a in table.arrays())
    lens = ctx.bait_record_sizes(table).to_host()
    write_index_arrays(path, table.K, keys, offs, ids, lens, names)


def upload_index(ctx, idx, path="index"):
    """arrays of read_index_arrays -> (BaitTable, names, lens on the device).  The arrays are checked on the device
    (zk_bait_table_from_arrays); an index whose lens are not the table's own record sizes is refused as damaged."""
    from zotmer_amd import native
    try:
        table = ctx.bait_table_from_arrays(idx["K"], ctx.upload(idx["keys"], np.uint64), ctx.upload(idx["offs"], np.uint32),
                                           ctx.upload(idx["ids"], np.uint32), len(idx["lens"]))
    except native.ZotkError as e:
        if e.code != native.ZK_EINVAL:
            raise
        raise BadIndex("%s: a damaged index: %s" % (path, e))
    lens = ctx.bait_record_sizes(table)
    if not np.array_equal(lens.to_host(), idx["lens"]):
        raise BadIndex("%s: a damaged index: its lens are not the numbers of k-mers that list each record" % path)
    return table, idx["names"], lens


def read_index(ctx, path):
    return upload_index(ctx, read_index_arrays(path), path)


def complete(ctx, table, lens_dev, kmers_dev):
    """the ascending record numbers whose every k-mer is in the set (mlst.py:45-54)"""
    hits = ctx.bait_tally(table, kmers_dev).to_host()
    return np.nonzero(hits == lens_dev.to_host())[0]


def lines(inp, records, names):
    """mlst.py:54"""
    return ["%s\t%d\t%s\n" % (inp, j, names[j]) for j in records]
