"""What the device tests of the window front end (tests/test_gpu_window_bytes.py, tests/test_gpu_record_lengths.py) rest on, checked
where no device is needed: the streams of tests/_window_streams.py hold what they say, the references agree with one another on
them, and the phantom baits can tell a byte read as a base from one that ended its windows."""
import numpy as np
import pytest

from oracle import zkoracle as zo
from tests import _alufinder_restatement as AR
from tests import _capture_restatement as CR
from tests import _disass_restatement as DR
from tests import _hgvsindex_restatement as HR
from tests import _mlst_restatement as MR
from tests import _strand_restatement as SR
from tests import _window_streams as W

KS = (3, 25, 32)
SEED = 1
BASE_VALUES = sorted(W.CODE)


def test_the_alphabet():
    assert bytes(BASE_VALUES) == b"ACGTUacgtu"
    assert [W.CODE[c] for c in b"ACGTUacgtu"] == [0, 1, 2, 3, 3, 0, 1, 2, 3, 3]
    # the bytes that share bits with a base are not bases: A without bit 0, one low bit changed, bit 7 set, bit 6 cleared, NUL
    for v in b"@`EeQqSsWwDd\xc1\xe1\xd4\xf5\x01\x03\x07\x14\x15!#'45\x00":
        assert not W.is_base(v)


@pytest.mark.parametrize("K", KS)
def test_every_value_at_every_phase(K):
    stream, offs = W.byte_phase_stream(K, SEED)
    data = np.frombuffer(stream, dtype=np.uint8)
    assert offs.shape == (256, 16) and len(np.unique(offs)) == 4096
    assert np.array_equal(data[offs], np.broadcast_to(np.arange(256)[:, None], offs.shape))
    assert np.array_equal(offs % 16, np.broadcast_to(np.arange(16)[None, :], offs.shape))
    assert stream.endswith(b"\n")
    # K + 1 letters or more before v, K + 2 after, then the line end
    letters = np.isin(data, np.frombuffer(W.LETTERS, dtype=np.uint8))
    for d in range(1, K + 2):
        assert letters[offs - d].all()
    for d in range(1, K + 3):
        assert letters[offs + d].all()
    assert (data[offs + K + 3] == 10).all()
    assert {3: 60_000, 25: 250_000, 32: 310_000}[K] < len(stream) < {3: 80_000, 25: 280_000, 32: 350_000}[K]


@pytest.mark.parametrize("crlf", [False, True])
def test_fastq_form(crlf):
    K = 25
    text, offs, seqs = W.byte_phase_fastq(K, SEED, crlf)
    data = np.frombuffer(text, dtype=np.uint8)
    have = offs >= 0
    assert not have[10].any() and have[np.arange(256) != 10].all() and len(seqs) == 255 * 16
    assert np.array_equal(data[offs[have]], np.broadcast_to(np.arange(256)[:, None], offs.shape)[have])
    assert np.array_equal((offs % 16)[have], np.broadcast_to(np.arange(16)[None, :], offs.shape)[have])
    eol = b"\r\n" if crlf else b"\n"
    lines = text.split(b"\n")
    assert lines.pop() == b"" and len(lines) == 4 * len(seqs)
    for r, seq in enumerate(seqs):
        head, got, plus, qual = (l[:len(l) - len(eol) + 1] for l in lines[4 * r:4 * r + 4])
        assert got == seq and (not crlf or lines[4 * r + 1].endswith(b"\r"))
        # the other three lines: base letters only, and the quality line long enough to hold windows
        assert all(W.is_base(c) for c in head + plus + qual) and len(qual) == len(seq) > 2 * K
    # the records as the readers of the restatements cut them
    recs = CR.fastq_records(text.decode("latin-1"))
    assert len(recs) == len(seqs)
    assert [r[1].encode("latin-1") for r in recs] == list(seqs)          # v lies inside its line: nothing of it is stripped


def _as_text(data):
    return bytes(data).decode("latin-1")


@pytest.mark.parametrize("K", KS)
def test_references_agree_on_every_byte(K):
    """windows(), the C oracle (zo.kmers_list, zo.kmerize) and every restatement the device tests use give the same windows of a
    stream that holds every byte value at every phase"""
    stream, _ = W.byte_phase_stream(K, SEED)
    fwd = [x for _, x in W.windows(stream, K)]
    both = W.kmers_both(stream, K)
    assert np.array_equal(np.array(fwd, dtype=np.uint64), both[0::2])
    assert np.array_equal(zo.kmers_list(K, stream, False), both[0::2])
    assert np.array_equal(zo.kmers_list(K, stream, True), both)
    want = zo.kmerize(K, [stream])
    k, c = W.counted(both)
    assert np.array_equal(want["kmers"], k) and np.array_equal(want["counts"], c) and want["acgt"] == W.acgt_of(both)
    text = _as_text(stream)
    assert CR.kmers(K, text, False) == fwd and CR.kmers(K, text, True) == both.tolist()
    assert DR.kmers_list(K, text, True) == both.tolist()
    assert MR.kmers_both(K, text) == both.tolist()
    assert HR.kmers(K, text, True) == both.tolist()
    # the reader of the pile-up: positions too
    pos = W.windows(stream, K)
    f, r = AR.kmers_with_pos_lists(K, text)
    assert f == [(x, p + 1) for p, x in pos]
    assert r == [(W.revcomp(x, K), len(stream) - p - K + 1) for p, x in pos]
    # the genome tally skips line ends; on one piece (no '\n', '\r' inside) it counts the same windows
    v, s = ord("N"), 5
    _, offs = W.byte_phase_stream(K, SEED)
    piece = stream[offs[v, s] - K - 1:offs[v, s] + K + 3]
    mine = [x for _, x in W.windows(piece, K)]
    got, _, nw, _ = HR.tally(K, piece, set(mine))
    assert nw == len(mine) and sum(got.values()) == len(mine)


def test_references_agree_on_an_embedded_payload():
    K = 25
    payload = W.base_run(K + 7, 3)
    whole = W.embedded(payload, 7)
    assert bytes(whole[7:7 + len(payload)]) == payload and len(whole) == 7 + len(payload) + 256
    assert all(W.is_base(c) for c in bytes(whole))
    mine = [x for _, x in W.windows(payload, K)]
    assert len(mine) == 8
    assert zo.kmers_list(K, payload, False).tolist() == mine == CR.kmers(K, payload.decode(), False)
    # the surroundings are bases and not periodic: a window that leaves the payload is a k-mer the payload does not hold
    around = {x for _, x in W.windows(bytes(whole), K)} - set(mine)
    assert len(around) == len(whole) - K + 1 - len(mine)
    for lead in (0, 1, 7, 16, 112):
        w = W.embedded(payload, lead, tail=64)
        assert bytes(w[lead:lead + len(payload)]) == payload and len(w) == lead + len(payload) + 64


@pytest.mark.parametrize("K", [25, 32])
def test_phantoms_tell_a_misread_byte(K):
    stream, offs = W.byte_phase_stream(K, SEED)
    ph, have = W.phantom_baits(K, stream, offs)
    assert have.all() and ph.shape == (256, 16, K, 4, 2)
    real = W.kmers_both(stream, K)
    is_real = np.isin(ph, real)
    base = np.zeros(256, dtype=bool)
    base[BASE_VALUES] = True
    # a byte that is not a base: no phantom is a window of the stream or the reverse complement of one
    assert not is_real[~base].any()
    # a base: at every phase, every window around it is real for exactly the letter it stands for, on both strands
    for v in BASE_VALUES:
        assert is_real[v, :, :, W.CODE[v], :].all()
        assert int(is_real[v].sum()) >= 16 * K * 2
    # and a phantom of one (v, s) is no phantom of another byte value: a hit names the byte
    keys, t_offs, ids, n_rec = W.phantom_table(ph, have)
    assert n_rec == 256 and np.all(keys[1:] > keys[:-1]) and t_offs[0] == 0 and t_offs[-1] == len(ids)
    assert np.all(np.diff(t_offs.astype(np.int64)) == 1)
    # window j of (v, s) with letter b, forward: the k-mer of the bytes themselves
    data = bytearray(stream)
    v, s, j, b = 0xC1, 9, K // 2, 2
    p = int(offs[v, s])
    data[p] = ord("G")
    assert int(ph[v, s, j, b, 0]) == zo.kmers_list(K, bytes(data[p - K + 1 + j:p + 1 + j]), False)[0]
    assert int(ph[v, s, j, b, 1]) == zo.rc(K, int(ph[v, s, j, b, 0]))


def test_phantoms_of_the_fastq_form():
    K = 25
    for crlf in (False, True):
        text, offs, seqs = W.byte_phase_fastq(K, SEED, crlf)
        ph, have = W.phantom_baits(K, text, offs)
        assert np.array_equal(have, offs >= 0)
        real = np.concatenate([W.kmers_both(s, K) for s in seqs])
        is_real = np.isin(ph, real)
        base = np.zeros(256, dtype=bool)
        base[BASE_VALUES] = True
        assert not is_real[~base].any()
        for v in BASE_VALUES:
            assert is_real[v, :, :, W.CODE[v], :].all()
        # the other three lines hold windows, and none of them is a phantom or a window of a sequence line
        other = W.kmers_both(text, K)
        assert len(other) > 2 * len(real)
        extra = np.setdiff1d(other, real)
        assert len(extra) > len(real) // 2 and not np.isin(ph, extra).any()


def test_tagged_keys_with_every_window_kept():
    """zk_strand_keys with T = 4^K - 1 keeps every window: the keys straight from the windows are the restatement's"""
    K = 25
    _, _, seqs = W.byte_phase_fastq(K, SEED)
    part = seqs[::37]
    T = (1 << (2 * K)) - 1
    for reverse in (0, 1):
        want = SR.tagged_keys(K, [_as_text(s) for s in part], reverse, T)
        assert W.tagged_keys(K, part, reverse).tolist() == want and len(want) > 1000


@pytest.mark.parametrize("K", [1, 9, 25, 32])
def test_uniform_reads_have_one_length(K):
    for L in range(max(K - 1, 1), 561):
        reads = W.uniform_reads(L, K, seed=L)
        assert len(reads) == -(-40_000 // (L + 1)) and all(len(r) == L for r in reads)
        assert all(b"\n" not in r for r in reads)
        if L % 7 == 0:
            a, b = W.near_uniform(reads)
            whole = W.stream_of(reads)
            assert len(whole) % (L + 1) == 0 and whole.index(b"\n") == L
            assert len(a) == len(whole) - 1 and len(a) % (L + 1) != 0 and a.index(b"\n") == L
            assert len(b) == len(whole) and b.index(b"\n") == L and b != whole
            assert sum(x != y for x, y in zip(b, whole)) == 2 and b.count(b"\n") == whole.count(b"\n") and b.endswith(b"\n")
    some = b"".join(W.uniform_reads(150, K, seed=150))
    assert some.count(b"N") > 0 and any(c in some for c in b"acgt")
    # sampled from a genome of 2 000 bases: the k-mers repeat
    if K >= 9:
        xs = W.kmers_both(W.stream_of(W.uniform_reads(150, K, seed=150)), K)
        assert len(np.unique(xs)) < len(xs) // 3
