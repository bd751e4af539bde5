"""Run by tests/test_gpu_borrowed_stream.py in its own process (torch is imported first, as bench.py does for N > 1): a context
that borrows a torch stream with zk_set_stream -- the mode include/zotk.h advertises for a host that lives in torch.

One line per check, STREAM-OK at the end; the first failure exits non-zero and nothing is started after it.

  * the handles: a fresh context has a stream of its own; after set_stream(handle) get_stream() is that handle; set_stream(None)
    gives a new one; handle 0 is refused; borrowing twice in a row works; zk_destroy leaves a borrowed stream alive (torch goes on using it);
  * on the borrowed stream the entries give the oracle's results, at the small sizes of tests/test_gpu_views.py, and
    zk_profile / zk_profile_read record their launches;
  * ordering: inside `with torch.cuda.stream(s)`, with no host synchronisation in between, a torch producer that takes milliseconds
    (a sort of 2^24 values, copied into the input tensor), then the entries the header calls asynchronous (zk_can, zk_copy,
    zk_add_u64, zk_widen_counts) on borrowed torch tensors, then a torch consumer that clones their outputs.  The clones must
    equal the oracle.  THIS CHECK IS ONE-SIDED: it cannot fail on a correct library; if any of that work ran on another stream it
    would read the input before the producer has written it, or be cloned before it has run, and fail with high probability,
    though not with certainty (a race that happens to be won looks the same as ordering);
  * a bait table built on the context's own stream, used and freed after the context has switched to a borrowed one;
  * a plain FASTQ file read through zk_source (whose ring keeps a copy stream of its own) on the borrowed stream, compared with
    the file and with the same read on the context's own stream."""
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import zkoracle as zo                     # noqa: E402
from tests import _core_cases as cc                   # noqa: E402
from tests import _view_cases as V                    # noqa: E402
from zotmer_amd import native, synth                  # noqa: E402

U64 = np.uint64


def ok(name, cond, detail=""):
    print("%s %s%s" % ("ok  " if cond else "FAIL", name, (": " + str(detail)) if detail and not cond else ""), flush=True)
    if not cond:
        sys.exit(1)


def spec_of(name):
    return V.flat(dict(V.CASES)[name]())


def run_case(ctx, name):
    """the case of tests/test_gpu_views.py at lead 0: every result the oracle's, every frame intact"""
    try:
        for spec in spec_of(name):
            V.run(ctx, spec, "P0")
    except (AssertionError, native.ZotkError) as e:
        ok(name + " on the borrowed stream", False, e)
    ok(name + " on the borrowed stream", True)


def read_file(ctx, path, size):
    buf = ctx.empty(size + 4096, np.uint8)
    got, eof = [], False
    with ctx.source_open(path, threads=2) as src:
        while not eof:
            src.start(buf, 0, buf.n)
            n, eof = src.finish()
            got.append(buf.to_host(n))
    return np.concatenate(got) if got else np.zeros(0, dtype=np.uint8)


def main():
    torch.cuda.set_device(0)
    ctx = native.Context(0)

    # ---- the handles ---------------------------------------------------------------------------------------------------------
    own = ctx.get_stream()
    ok("a fresh context has a stream of its own", own != 0)
    baits = cc.capture_case()[1]
    table = ctx.bait_table(ctx.upload_stream(cc.stream_of(baits)), V.R.READ_K)          # built on the own stream
    s, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    ctx.set_stream(s.cuda_stream)
    ok("get_stream() is the borrowed handle", ctx.get_stream() == s.cuda_stream, (ctx.get_stream(), s.cuda_stream))
    ctx.set_stream(None)
    again = ctx.get_stream()
    ok("set_stream(None) gives a new stream of its own", again != 0 and again != s.cuda_stream, again)
    try:
        ctx.set_stream(0)
        refused = False
    except ValueError:
        refused = True
    ok("the null stream (torch's default stream) is refused, not taken for None", refused and ctx.get_stream() == again)
    ctx.set_stream(s2.cuda_stream)
    ctx.set_stream(s.cuda_stream)
    ok("borrowing twice in a row", ctx.get_stream() == s.cuda_stream)

    # ---- the entries on the borrowed stream ------------------------------------------------------------------------------------------
    ctx.profile(True)
    run_case(ctx, "kmerize-deep-K25-canonical")
    prof = ctx.profile_read()
    ctx.profile(False)
    ok("zk_profile_read records the launches on the borrowed stream",
       prof.get("pass_stream", {}).get("launches", 0) >= 1 and all(v["ms"] > 0 for v in prof.values()), prof)
    for name in ("kmerize-deep-K25-canonical-dedupe_bits18-strand_blocks1", "kmerize-tiny", "sort_keys-K31-tile_sort1-wide1", "sort_keys-tiny",
                 "union_sum-uint32", "union_sum-uint32-tiny", "merge_n-k5-kway2", "merge_n-k2-kway2-tiny", "hist-uint32", "hist-uint32-tiny",
                 "codec_encode-delta", "codec_decode-delta1", "codec_encode-u64-tiny", "codec_decode-delta0-tiny"):
        run_case(ctx, name)

    # ---- a table of the own stream, used and freed on the borrowed one ----------------------------------------------------------
    V._capture_table.put(ctx, table)
    run_case(ctx, "capture_hits")
    V._capture_table.put(ctx, None)
    table.free()
    run_case(ctx, "line_ends")
    ok("a bait table of the own stream, freed after the switch", True)

    # ---- ordering ------------------------------------------------------------------------------------------------------------------
    n, m, K = 1 << 24, 4096, 25
    src = torch.randint(0, 1 << 50, (n,), dtype=torch.int64, device="cuda")
    x = torch.zeros(n, dtype=torch.int64, device="cuda")
    out_can = torch.zeros(m, dtype=torch.int64, device="cuda")
    out_copy = torch.zeros(m, dtype=torch.int64, device="cuda")
    out_wide = torch.zeros(m, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    add = 0x0123456789ABCDEF
    with torch.cuda.stream(s):
        x.copy_(torch.sort(src).values)                                  # the producer: milliseconds
        tail = x[n - m:]                                                 # the largest values: the last the copy writes
        low = (tail & 0xFFFFFFFF).to(torch.int32)
        rcs = [ctx.lib.zk_can(ctx.h, K, tail.data_ptr(), m, out_can.data_ptr()),
               ctx.lib.zk_copy(ctx.h, out_copy.data_ptr(), tail.data_ptr(), 8 * m),
               ctx.lib.zk_add_u64(ctx.h, out_copy.data_ptr(), m, add),
               ctx.lib.zk_widen_counts(ctx.h, low.data_ptr(), out_wide.data_ptr(), m)]
        clones = [t.clone() for t in (out_can, out_copy, out_wide)]      # the consumer
        s.synchronize()
    ok("the asynchronous entries return ZK_OK", rcs == [0, 0, 0, 0], rcs)
    want = np.sort(src.cpu().numpy().astype(np.int64).view(U64))[n - m:]
    got = [c.cpu().numpy().view(U64) for c in clones]
    ok("zk_can between a torch producer and a torch consumer", np.array_equal(got[0], np.array([zo.can(K, int(v)) for v in want], dtype=U64)))
    with np.errstate(over="ignore"):
        ok("zk_copy and zk_add_u64 between them", np.array_equal(got[1], want + U64(add)))
    ok("zk_widen_counts between them", np.array_equal(got[2], want & U64(0xFFFFFFFF)))

    # ---- zk_source on the borrowed stream ---------------------------------------------------------------------------------------------
    text = synth.fastq_text(21, 0, 4000, 150, genome=0).encode()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "reads.fastq")
        with open(path, "wb") as f:
            f.write(text)
        borrowed = read_file(ctx, path, len(text))
        ctx.set_stream(None)
        owned = read_file(ctx, path, len(text))
    ok("zk_source on the borrowed stream reads the file", borrowed.tobytes() == text, (len(borrowed), len(text)))
    ok("... as on the context's own stream", np.array_equal(borrowed, owned))

    # ---- zk_destroy leaves a borrowed stream alive -----------------------------------------------------------------------------------
    ctx.set_stream(s.cuda_stream)
    run_case(ctx, "add_u64-tiny")
    ctx.close()
    with torch.cuda.stream(s):
        total = torch.arange(1 << 20, device="cuda", dtype=torch.int64).sum()
    s.synchronize()
    ok("the torch stream works after zk_destroy", int(total.item()) == (1 << 20) * ((1 << 20) - 1) // 2)
    print("STREAM-OK", flush=True)


if __name__ == "__main__":
    main()
