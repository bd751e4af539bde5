"""The core entry points on offset views of larger device arrays (include/zotk.h, "ARRAYS AND THEIR ALIGNMENT").

Production callers hand the entries sub-ranges of slabs: library/engine.py writes the table of zk_kmerize at an element offset of
a slab and union-sums two views of one slab, library/strand.py formats a.view(m, lo), parallel.py borrows data_ptr() + 8 * off
out of torch tensors.  Every other GPU test passes arrays that begin an allocation, which is 256-byte aligned, and looks for
stray writes behind an array only.  Here every device array of a call is a tests/_frames.py Frame: a view at a lead inside a
guarded allocation, so that an entry that stores whole 16-, 64- or 128-byte units into a caller's array, loads four tags at once
from it, rounds a pointer down to a line or writes a few words IN FRONT of an output fails a comparison (it cannot fault the
device: every stray write the frames can catch lies inside an allocation).

For every case and each placement (P0: lead 0, the control; P1: natural alignment only; P2: the last place before a 128-byte
line; P3: mixed phases, inputs and outputs on different leads):
  * the return code, every count and scalar equal the oracle's;
  * every output equals the oracle bit for bit, and what the same call wrote at P0 on the same context;
  * every output frame is intact outside the result -- list entries are called with cap = the length needed, which the header
    says is enough, so the guard begins at the first element behind the result;
  * every input frame holds what was uploaded, payload and guard; of an array that the entry destroys (zk_sort_count's d_keys) or
    works in place on, the guard.
The inputs and oracle results are those of tests/_core_cases.py (about three of the entry's largest tile plus 5) and tiny ones
whose results are 1, 3 and 5 elements, shorter than any vector unit (the builders assert the lengths; where an entry cannot give
them the smallest it can: 2, 6, 10 where every k-mer comes with its mirror -- zk_encode of both strands, zk_mirror_expand and
zk_kmerize at odd K --, whole lines and records for the texts of zk_format_pairs, zk_contig_render and zk_capture_gather, 2, 3
and 5 bytes for zk_synth_reads, whose reads have a base at least); zk_mirror_expand alone goes above (65 536 + 5 canonical
entries: its grouped route, pipeline.hip).

The entries that need a 16-byte aligned stream (zk_encode, zk_capture_filter, zk_kmerize, zk_stream_checksum, zk_fastq_mask)
get their streams on 16-byte leads above, and leads of 1, 4 and 8 bytes in test_sixteen_byte_rule: ZK_EINVAL, every output
frame wholly guard, and the same context then runs the aligned call."""
import pytest

from tests import _frames as F
from tests._view_cases import CASES, DEFAULT_KNOBS, EINVAL, SIXTEEN, check, flat, run
from zotmer_amd import native

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = native.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("placement", F.PLACEMENTS)
@pytest.mark.parametrize("name,build", CASES, ids=[c[0] for c in CASES])
def test_views(ctx, name, build, placement):
    check(ctx, name, flat(build()), placement)


# ---- the 16-byte rule -------------------------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("lead", [1, 4, 8])
@pytest.mark.parametrize("entry", sorted(SIXTEEN))
def test_sixteen_byte_rule(ctx, entry, lead):
    """a stream `lead` bytes off the 16-byte grid: ZK_EINVAL, every output frame wholly guard, the inputs untouched, and the same
    context then runs the aligned call"""
    name, off_grid = SIXTEEN[entry]
    spec = flat(dict(CASES)[name]())[0]
    frames = []
    for i, a in enumerate(spec.arrays):
        at = lead if i in off_grid else 0
        frames.append(F.Frame.output(ctx, a.want.dtype, a.cap, at) if a.role == "out" else F.Frame(ctx, a.data, at))
    try:
        ctx.tune(**spec.knobs)
        rc = spec.call(ctx, [f.arr for f in frames])[0]
        ctx.sync()
    finally:
        ctx.tune(**DEFAULT_KNOBS)
    assert rc == EINVAL, (entry, lead, rc)
    assert all(f.unchanged() for f in frames), (entry, lead)
    run(ctx, spec, "P0")
