"""
Host side of `zot ksnp` (zotmer/commands/ksnp.py): the set's k-mers go to the device, one entry of csrc/ksnp.hip marks and
compacts the candidate-SNP k-mers (zk_ksnp_flank for the default mode, zk_ksnp_components for -H and -L), and the kept k-mers
are written as a k-mer set without counts.  DESIGN.md section 6p has the design and the measurements.
"""
import sys

MAX_KMERS = (1 << 32) - 2          # csrc/ksnp.hip: parents and directory entries are 32 bits wide

DEFAULT, HAMMING, LEVENSHTEIN = "default", "hamming", "levenshtein"


class TooManyKmers(Exception):
    pass


class NoKmers(Exception):
    pass


def check_meta(path, meta):
    """the input's metadata, before anything touches the device -> K"""
    if "kmers" not in meta:
        raise NoKmers('cannot dump "%s" as it contains no k-mers' % path)
    K = meta["K"]
    if not isinstance(K, int) or isinstance(K, bool) or not 1 <= K <= 32:
        raise NoKmers('"%s": K = %r, this build handles 1 <= K <= 32' % (path, K))
    return K


def candidates(ctx, kmers, K, mode=DEFAULT, d=0):
    """ascending k-mers on the device -> the candidate-SNP k-mers among them (a uint64 DeviceArray view, ascending)"""
    from zotmer_amd import native
    from zotmer_amd.library.timing import Phase
    if kmers.n > MAX_KMERS:
        raise TooManyKmers("%d k-mers; `zot ksnp` indexes them with 32 bits, at most %d" % (kmers.n, MAX_KMERS))
    metric = {DEFAULT: None, HAMMING: native.KSNP_HAMMING, LEVENSHTEIN: native.KSNP_LEVENSHTEIN}[mode]
    with Phase(ctx, "ksnp %s" % mode, 8 * kmers.n):
        return ctx.ksnp(kmers, K, metric, d)


def write_set(path, K, kmers_bytes=None, ctx=None, kmers_dev=None):
    """the file the reference names (ksnp.py:159-162): the `kmers` stream and meta {K, kmers}, through the container writer.
    The k-mers come as the bytes of the member (vectors.encode_kmers) or as a device array."""
    from zotmer_amd.library import vectors
    from zotmer_amd.library.container import KmerSet
    with KmerSet(path, "w") as z:
        if kmers_dev is None:
            z.add("kmers", kmers_bytes)
        elif kmers_dev.n == 0:
            z.add("kmers", b"")
        else:
            words = vectors._check_codec(ctx.codec_encode, kmers_dev, True)
            z.add_device("kmers", ctx, words)
        z.meta = {"K": K, "kmers": "kmers"}


def run(make_ctx, out_path, in_path, mode=DEFAULT, d=0):
    """make_ctx() gives the device context; it is called once the input's metadata is known to be good"""
    from zotmer_amd.library import vectors
    from zotmer_amd.library.container import KmerSet
    with KmerSet(in_path, "r") as z:
        try:
            K = check_meta(in_path, z.meta)
        except NoKmers as e:
            sys.stderr.write("%s\n" % e)
            raise SystemExit(1)
        ctx = make_ctx()
        kmers = vectors.device_read_kmers(ctx, z)          # counts, if any, are ignored, as the reference ignores them
    try:
        kept = candidates(ctx, kmers, K, mode, d)
    except TooManyKmers as e:
        sys.stderr.write("zot ksnp: %s: %s\n" % (in_path, e))
        raise SystemExit(1)
    write_set(out_path, K, ctx=ctx, kmers_dev=kept)
