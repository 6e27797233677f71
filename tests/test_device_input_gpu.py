"""Gene calls on sequences that already lie in device memory (pga_batch_create_device / pga_batch_read, DeviceSequences,
Context.upload_device, GeneFinder.find_genes_batch(DeviceSequences)).

The packed letters are compared with the numpy restatement of the rule (tests/device_input_ref.py); every gene call is compared with
the existing host path -- Context.upload / GeneFinder on bytes -- which is itself pinned to the oracle and is never the code under
test.  Device memory comes from tests/hip_mem.py (the HIP runtime the library already loaded, no torch), but for the one torch test,
which runs in a child process."""
import functools
import io
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import hip_mem
from tests.device_input_ref import pack_reference
from tests.util import golden_path, read_fasta

pytestmark = pytest.mark.gpu

LETTERS = np.frombuffer(b"ACGTNacgtn", np.uint8)
ALPHABET = b"ACGTacgtn"                                     # 9 letters: 'N' only comes from ids outside the table
# the lengths of the issue's ragged batch (3072 is the extraction tile), in an order that puts the seams at 14 residues mod 16
RAGGED = [16, 31, 47, 5, 3072, 32, 3071, 15, 48, 3, 2, 3073, 17, 33, 1, 20000, 6145, 0, 49]
BAD_IDS = {1: [9, 255], 4: [-1, 9, 255, 256], 8: [-1, 9, 255, 256, 1 << 31, -(1 << 63)]}
DTYPES = {1: np.uint8, 4: np.int32, 8: np.int64}


@pytest.fixture(scope="module")
def ctx():
    from pyrodigal_amd import _cabi, benchdata
    c = _cabi.Context(0)
    c.set_models([b for _, b in benchdata.load_model_set()])
    yield c
    c.close()


LIVE = []        # what a test put on the device: closed when the test ends, passed or failed, while the module's context still exists


@pytest.fixture(autouse=True)
def release_device_objects():
    yield
    while LIVE:
        LIVE.pop().close()


def keep(x):
    LIVE.append(x)
    return x


def random_letters(rng, n):
    return LETTERS[rng.integers(0, len(LETTERS), size=n)]


def as_tokens(rng, letters, elem_bytes):
    """Token ids under ALPHABET that spell `letters`: every 'N' becomes one of the ids that lie outside the table."""
    index = np.full(256, -1, np.int64)
    index[np.frombuffer(ALPHABET, np.uint8)] = np.arange(len(ALPHABET))
    ids = index[letters]
    bad = np.array(BAD_IDS[elem_bytes], np.int64)
    ids = np.where(ids < 0, bad[rng.integers(0, len(bad), size=len(letters))], ids)
    return ids.astype(DTYPES[elem_bytes])


def ragged_source(rng, lens, elem_bytes, tokens, residues=False):
    """Contigs of random letters in one flat source with gaps of 0 .. 17 elements between them (filled with valid elements that would
    show if they leaked).  `residues`: the gaps are chosen so that the start of contig k lies at element k mod 16."""
    parts, offs, at = [], [], 0
    for k, n in enumerate(lens):
        gap = int(rng.integers(0, 18))
        if residues:
            gap = (k - at) % 16
            gap += 16 if gap < 2 and k % 3 == 0 else 0
        parts.append(np.full(gap, ord("A"), np.uint8))
        at += gap
        offs.append(at)
        parts.append(random_letters(rng, n))
        at += n
    parts.append(np.full(int(rng.integers(0, 18)), ord("A"), np.uint8))
    letters = np.concatenate(parts)
    data = as_tokens(rng, letters, elem_bytes) if tokens else letters
    return data, offs


def upload(ctx, data, lens, offs=None, alphabet=None, **kw):
    from pyrodigal_amd import DeviceSequences
    d = keep(hip_mem.DeviceArray.from_numpy(data))
    ds = DeviceSequences(d, lens, offsets=offs, alphabet=alphabet, **kw)
    return (keep(ctx.upload_device(ds)) if ctx is not None else None), d, ds


def check_letters_only(batch, want):
    assert batch.n == len(want) and batch.read() == b"".join(want)
    for i, w in enumerate(want):
        assert batch.read(i) == w, i


def check_letters(batch, want):
    assert batch.n == len(want) and batch.total == sum(len(w) for w in want)
    assert batch.read() == b"".join(want)
    for i, w in enumerate(want):
        assert batch.read(i) == w, i


# ---- 1. packed letters ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("elem_bytes,tokens", [(1, False), (1, True), (4, True), (8, True)])
def test_packed_letters_of_a_ragged_batch(ctx, elem_bytes, tokens):
    rng = np.random.default_rng(100 + elem_bytes + tokens)
    data, offs = ragged_source(rng, RAGGED, elem_bytes, tokens, residues=True)
    alphabet = ALPHABET if tokens else None
    want = pack_reference(data, offs, RAGGED, alphabet)
    assert sorted(len(w) for w in want) == sorted([0, 1, 2, 3, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 3071, 3072, 3073, 6145, 20000])
    batch, d, _ = upload(ctx, data, RAGGED, offs, alphabet)
    if elem_bytes == 1:
        assert {(d.ptr + o) % 16 for o, n in zip(offs, RAGGED) if n} == set(range(16))
    assert len({int(x) % 16 for x in np.cumsum(RAGGED)}) >= 8
    if tokens:
        assert b"N" in b"".join(want) and all(np.any(data == DTYPES[elem_bytes](b)) for b in BAD_IDS[elem_bytes])
    check_letters(batch, want)
    batch.close()
    d.close()


@pytest.mark.parametrize("elem_bytes,tokens", [(1, False), (1, True), (4, True), (8, True)])
def test_packed_letters_of_many_tiny_contigs(ctx, elem_bytes, tokens):
    """300 contigs of 1 .. 7 bases: many seams fall inside one 16-byte group."""
    rng = np.random.default_rng(200 + elem_bytes + tokens)
    lens = [int(x) for x in rng.integers(1, 8, size=300)]
    data, offs = ragged_source(rng, lens, elem_bytes, tokens)
    alphabet = ALPHABET if tokens else None
    batch, d, _ = upload(ctx, data, lens, offs, alphabet)
    check_letters(batch, pack_reference(data, offs, lens, alphabet))
    batch.close()
    d.close()


# ---- 2. padded rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("elem_bytes", [1, 4, 8])
def test_padded_rows_never_leak_their_padding(ctx, elem_bytes):
    rng = np.random.default_rng(300 + elem_bytes)
    lens = [77, 0, 1, 16, 40, 77, 0, 63, 15]
    rows = np.full((9, 77), ord("A"), np.uint8)                    # the padding: valid letters that would lengthen a contig
    for i, n in enumerate(lens):
        rows[i, :n] = random_letters(rng, n)
    tokens = elem_bytes > 1
    data = as_tokens(rng, rows.reshape(-1), elem_bytes).reshape(9, 77) if tokens else rows
    alphabet = ALPHABET if tokens else None
    batch, d, ds = upload(ctx, data, lens, None, alphabet)
    assert list(ds.offsets) == [77 * i for i in range(9)]
    want = pack_reference(data, ds.offsets, lens, alphabet)
    assert want == [rows[i, :n].tobytes() for i, n in enumerate(lens)] and batch.total == sum(lens)
    check_letters(batch, want)
    batch.close()
    d.close()


# ---- 3. overlapping, repeated and reordered source ranges --------------------------------------------------------------------------
def test_overlapping_repeated_and_reordered_ranges(ctx):
    from pyrodigal_amd import DeviceSequences
    rng = np.random.default_rng(400)
    rows = random_letters(rng, 5 * 50).reshape(5, 50)
    d = keep(hip_mem.DeviceArray.from_numpy(rows))
    ds = DeviceSequences(d, [50, 33, 0, 17, 50])
    for sub in (ds.take([1, 1, 1]), ds[::-1], ds.take([4, 0, 4, 2, 0])):
        batch = keep(ctx.upload_device(sub))
        check_letters(batch, pack_reference(rows, sub.offsets, sub.lengths, None))
        batch.close()
    flat = DeviceSequences(keep(hip_mem.DeviceArray.from_numpy(rows.reshape(-1))), [100, 100, 30, 250], offsets=[0, 50, 120, 0])      # overlaps
    batch = keep(ctx.upload_device(flat))
    check_letters(batch, pack_reference(rows, flat.offsets, flat.lengths, None))
    batch.close()
    d.close()


# ---- 4. end to end against a host-born batch ----------------------------------------------------------------------------------------
def blob(*arrays):
    out = []
    for a in arrays:
        b = a if isinstance(a, (bytes, bytearray)) else np.ascontiguousarray(a).tobytes()
        out.append(len(b).to_bytes(8, "little") + bytes(b))
    return b"".join(out)


def snap(res):
    """Everything deterministic of a BatchResult: the records field by field (they have padding bytes), masks, cuts, the sets' choice
    and the trimmed lengths."""
    parts = [res.genes[k] for k in res.genes.dtype.names] + [res.contigs[k] for k in res.contigs.dtype.names]
    parts += [np.asarray([res.node_passes, res.n_chains], np.int64)]
    parts += [b"" if res.masks is None else blob(*res.masks)]
    for name in ("cuts", "set_models", "set_scores", "model_scores", "terminal_repeats"):
        extra = getattr(res, name, None)
        parts.append(b"-" if extra is None else blob(extra))
    return blob(*parts)


@functools.lru_cache(maxsize=None)
def contigs():
    """The committed fixtures, cuts of them, a few contigs of 61 .. 400 bases, and one that ends in a copy of its first 40 bases."""
    miij, srr, kk = (read_fasta(n + ".fna.gz")[0][1].encode() for n in ("MIIJ01000039", "SRR492066", "KK037166"))
    rng = np.random.default_rng(500)
    low = bytearray(srr[30000:42000])
    low[2000:2600] = bytes(low[2000:2600]).lower()                  # a lower-case run for mask_lowercase
    circle = kk[4000:12000]
    out = [miij[:120000], srr, kk, miij[300000:300061], srr[1000:1400], bytes(low), kk[:3073], miij[500000:506145],
           np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=211)].tobytes(), circle + circle[:40], srr[50000:50100]]
    return tuple(out)


def device_batch(ctx, seqs, elem_bytes=1):
    """The contigs back to back with small gaps, as letters or as token ids, uploaded from device memory."""
    rng = np.random.default_rng(501)
    parts, offs, at = [], [], 0
    for s in seqs:
        gap = int(rng.integers(0, 18))
        parts.append(np.full(gap, ord("T"), np.uint8)); at += gap
        offs.append(at)
        parts.append(np.frombuffer(s, np.uint8)); at += len(s)
    letters = np.concatenate(parts)
    if elem_bytes == 1:
        return upload(ctx, letters, [len(s) for s in seqs], offs, None)
    table = bytes(sorted(set(letters.tolist())))
    index = np.zeros(256, DTYPES[elem_bytes])
    index[np.frombuffer(table, np.uint8)] = np.arange(len(table))
    return upload(ctx, index[letters], [len(s) for s in seqs], offs, table)


SETTINGS = ("mask", "regions", "circular", "sets", "trim")


def configure(batch, setting, seqs):
    """One of the issue's settings on a resident batch; returns (the batch to call, find_genes keywords)."""
    n = len(seqs)
    if setting == "mask":
        return batch, {"mask": True}
    if setting == "regions":
        regions = [None] * n
        regions[0] = [(1000, 1500), (90000, 90010)]
        regions[2] = [(0, 300)]
        batch.set_masks(regions, mask_lowercase=True)
        return batch, {}
    if setting == "circular":
        batch.set_circular([i in (1, 2, 9) for i in range(n)])
        return batch, {}
    if setting == "sets":
        batch.set_sets(["a", "b", "a", None, "b", "b", "c", "a", None, "c", None])
        return batch, {}
    assert setting == "trim"
    match, trim = batch.terminal_repeats()
    assert trim[9] == 40 and match[9] == 40
    return keep(batch.trim_terminal_repeats(trim)), {}


@pytest.mark.parametrize("setting", SETTINGS)
def test_find_genes_equals_the_host_born_batch(ctx, setting):
    seqs = list(contigs())
    host = keep(ctx.upload(seqs))
    dev, d, _ = device_batch(ctx, seqs, 4 if setting == "mask" else 1)
    assert dev.read() == b"".join(seqs)
    hb, kw = configure(host, setting, seqs)
    db, _ = configure(dev, setting, seqs)
    want, got = ctx.find_genes(hb, meta=True, **kw), ctx.find_genes(db, meta=True, **kw)
    assert len(want.genes) > 100
    assert snap(got) == snap(want)
    if setting == "trim":
        assert db.read() == hb.read()
    for b in {id(x): x for x in (hb, db, host, dev)}.values():
        b.close()
    d.close()


def test_translate_and_render_equal_the_host_born_batch(ctx):
    seqs = list(contigs())
    host = keep(ctx.upload(seqs))
    dev, d, _ = device_batch(ctx, seqs)
    want, got = ctx.find_genes(host, meta=True), ctx.find_genes(dev, meta=True)
    assert snap(got) == snap(want)
    pw, ow = ctx.translate_genes(host, want)
    pg, og = ctx.translate_genes(dev, got)
    assert pg.tobytes() == pw.tobytes() and og.tobytes() == ow.tobytes() and len(pw) > 10000
    ids = ["contig_%d" % i for i in range(len(seqs))]
    tw = ctx.render_genes(host, want, ids, ("gff", "faa", "fna"), meta=True, unbinned_model=0)
    tg = ctx.render_genes(dev, got, ids, ("gff", "faa", "fna"), meta=True, unbinned_model=0)
    for name in ("gff", "faa", "fna"):
        assert tg[name].data == tw[name].data and len(tw[name].data) > 1000, name
        assert np.array_equal(tg[name].contig_offsets, tw[name].contig_offsets)
    host.close(); dev.close(); d.close()


def test_single_mode_with_a_model_per_contig_equals_the_host_born_batch(ctx):
    seqs = list(contigs())
    moc = [i % 3 for i in range(len(seqs))]
    host = keep(ctx.upload(seqs))
    dev, d, _ = device_batch(ctx, seqs, 8)
    want = ctx.find_genes(host, meta=False, model_of_contig=moc)
    got = ctx.find_genes(dev, meta=False, model_of_contig=moc)
    assert len(want.genes) > 100 and snap(got) == snap(want)
    host.close(); dev.close(); d.close()


def test_context_find_genes_batch_takes_device_sequences(ctx):
    """Upload + find + free in one call, wherever it accepts a list of sequences."""
    seqs = list(contigs())
    _, d, ds = device_batch(None, seqs, 4)
    for kw in ({"mask": True}, {"mask_lowercase": True, "trim_terminal_repeats": True}, {"circular": [i in (1, 2) for i in range(len(seqs))]}):
        want, got = ctx.find_genes_batch(seqs, meta=True, **kw), ctx.find_genes_batch(ds, meta=True, **kw)
        assert len(want.genes) > 100 and snap(got) == snap(want), kw


def test_read_serves_every_kind_of_batch(ctx):
    """`Batch.read` on batches the library made itself: replicated and trimmed ones carry their lengths too."""
    seqs = list(contigs())
    dev, d, _ = device_batch(ctx, seqs)
    host = keep(ctx.upload(seqs))
    assert host.read(3) == seqs[3] and host.read() == b"".join(seqs)
    rep = keep(ctx.replicate(dev, [2, 10, 2, 3]))
    check_letters_only(rep, [seqs[2], seqs[10], seqs[2], seqs[3]])
    match, trim = dev.terminal_repeats()
    assert trim[9] == 40
    cut = keep(dev.trim_terminal_repeats(trim))
    check_letters_only(cut, [s[:len(s) - int(t)] for s, t in zip(seqs, trim)])
    check_letters_only(keep(ctx.replicate(cut, [9])), [seqs[9][:-40]])


# ---- 5. the same under poison ----------------------------------------------------------------------------------------
def test_result_does_not_depend_on_a_reused_allocation(ctx):
    """No poison: a larger batch of other letters is freed first, so the device-born batch gets that allocation back (the context's
    spare slot) with those letters still in it -- behind its own letters, and where its tile and pack tables go.  Letters and gene
    calls are those of the host-born batch.  (The 16 bytes behind the last letter, which the kernel sets to 'N', cannot be reached
    through pga_batch_read: this shows that nothing observable depends on the old content, not that write itself.)"""
    seqs = list(contigs())
    host = keep(ctx.upload(seqs))
    want = snap(ctx.find_genes(host, meta=True, mask=True))
    host.close()
    total = sum(len(s) for s in seqs)
    stale = ctx.upload([b"ATGAAACCCGGGTTTTAA" * (total // 18 + 4000)])
    stale.close()                                                   # its allocation is the next batch's
    dev, d, _ = device_batch(ctx, seqs, 8)
    assert dev.read() == b"".join(seqs)
    assert snap(ctx.find_genes(dev, meta=True, mask=True)) == want


@pytest.mark.parametrize("byte", [0xFF, 0x00])
def test_result_does_not_depend_on_what_the_memory_held(ctx, byte):
    """DESIGN.md 3.1 under pga_debug_poison: every floating-point workspace buffer holds `byte`, and the letters' allocation is handed
    out full of 'N'.  What this shows for the device-born batch: its tables and letters, and the call behind them, do not read a
    buffer the call did not write."""
    seqs = list(contigs())
    host = keep(ctx.upload(seqs))
    want = snap(ctx.find_genes(host, meta=True, mask=True))
    letters = host.read()
    host.close()                                                    # its allocation is the next batch's
    ctx.debug_poison(byte)
    try:
        dev, d, _ = device_batch(ctx, seqs, 4)
        assert dev.read() == letters
        assert snap(ctx.find_genes(dev, meta=True, mask=True)) == want
        dev.close(); d.close()
    finally:
        ctx.debug_poison(None)


# ---- 6. stream order -----------------------------------------------------------------------------------------------------------------
def test_upload_waits_for_the_producer_stream(ctx):
    """The source holds 'N'; the real letters are on their way on a producer stream, behind twenty fills of 1 GB.  The upload is
    called at once, without a synchronise: the batch holds the real letters."""
    from pyrodigal_amd import DeviceSequences
    hip = hip_mem.hip()
    rng = np.random.default_rng(600)
    n = 1 << 20
    lens = [n // 2, n // 4, n // 4]
    pinned = keep(hip_mem.PinnedArray(n))
    pinned.array[:] = random_letters(rng, n)
    real = pinned.array.tobytes()
    src = keep(hip_mem.DeviceArray.from_numpy(np.full(n, ord("N"), np.uint8)))
    scratch = keep(hip_mem.DeviceArray(1 << 30))
    producer = hip_mem.Stream()
    try:
        for k in range(20):
            hip_mem.check(hip.hipMemsetAsync(scratch.ptr, k, scratch.nbytes, producer.cuda_stream), "hipMemsetAsync")
        hip_mem.check(hip.hipMemcpyAsync(src.ptr, pinned.ptr, n, hip_mem.H2D, producer.cuda_stream), "hipMemcpyAsync")
        batch = keep(ctx.upload_device(DeviceSequences(src, lens, stream=producer)))
        got = batch.read()
        assert got == real
        assert got != b"N" * n
        batch.close()
    finally:
        producer.synchronize()                                       # (before the buffers it writes are released)
        producer.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------
class Raw:
    """A pointer and nothing else."""

    def __init__(self, ptr, shape, typestr="|u1"):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 3, "strides": None}


def raw_create(ctx, ptr, n_elems, elem_bytes, offs, lens, alphabet):
    """pga_batch_create_device itself, past the checks of DeviceSequences: (return code, pga_last_error)."""
    import ctypes
    off = (ctypes.c_int64 * len(offs))(*offs)
    ln = (ctypes.c_int64 * len(lens))(*lens)
    h = ctypes.c_void_p()
    rc = ctx.L.pga_batch_create_device(ctx.h, len(lens), ctypes.c_void_p(ptr), n_elems, elem_bytes, off, ln, alphabet,
                                       0 if alphabet is None else len(alphabet), None, ctypes.byref(h))
    assert rc != 0 and not h
    return rc, ctx.L.pga_last_error(ctx.h).decode()


def test_refusals_come_from_the_host_and_leave_the_context_usable(ctx):
    from pyrodigal_amd import DeviceSequences, _cabi
    rng = np.random.default_rng(700)
    letters = random_letters(rng, 1000)
    d = keep(hip_mem.DeviceArray.from_numpy(letters))
    good = DeviceSequences(d, [400, 600])
    host_array = letters.copy()
    with pytest.raises(ValueError, match="not device memory"):
        ctx.upload_device(DeviceSequences(Raw(host_array.ctypes.data, (1000,)), [400, 600]))
    rc, msg = raw_create(ctx, d.ptr, 1000, 1, [0, 500], [400, 501], None)
    assert rc == _cabi.PGA_EINVAL and "contig 1" in msg
    rc, msg = raw_create(ctx, d.ptr, 500, 2, [0, 100], [100, 100], b"ACGT")
    assert rc == _cabi.PGA_EINVAL and "elem_bytes" in msg
    rc, msg = raw_create(ctx, d.ptr, 250, 4, [0, 100], [100, 100], None)
    assert rc == _cabi.PGA_EINVAL and "alphabet" in msg
    rc, msg = raw_create(ctx, d.ptr, 1000, 1, [0, 100], [100, 100], b"ACG*")
    assert rc == _cabi.PGA_EINVAL and "alphabet entry 3" in msg and "not an ASCII letter" in msg
    rc, msg = raw_create(ctx, d.ptr, 1000, 1, [0, -1], [100, 100], None)
    assert rc == _cabi.PGA_EINVAL and "contig 1" in msg
    batch = keep(ctx.upload_device(good))                                # the context runs a good call afterwards
    check_letters(batch, [letters[:400].tobytes(), letters[400:].tobytes()])
    batch.close()
    d.close()


# ---- 8. GeneFinder -------------------------------------------------------------------------------------------------------------------
def texts(genes, sid):
    out = []
    for writer in ("write_gff", "write_translations", "write_genes"):
        f = io.StringIO()
        try:
            getattr(genes, writer)(f, sid)
            out.append(f.getvalue())
        except RuntimeError as e:                                   # (a sequence no bin won has no GFF header, on either path)
            out.append("RuntimeError: %s" % e)
    return out


def same_genes(got, want, seqs):
    assert len(got) == len(want) == len(seqs)
    n_genes = 0
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.sequence.data == w.sequence.data
        assert g.sequence.gc == w.sequence.gc and list(g.sequence.masks) == list(w.sequence.masks)
        fields = ("begin", "end", "strand", "partial_begin", "partial_end", "start_type", "rbs_motif", "rbs_spacer", "gc_cont",
                  "translation_table", "cscore", "rscore", "sscore", "tscore", "uscore", "score")
        assert [[getattr(x, f) for f in fields] for x in g] == [[getattr(x, f) for f in fields] for x in w], i
        assert [x.sequence() for x in g] == [x.sequence() for x in w]
        assert [x.translate(translation_table=4, include_stop=False) for x in g] == [x.translate(translation_table=4, include_stop=False) for x in w]
        assert (g.circular, g.cut, g.terminal_repeat, g.terminal_repeat_match) == (w.circular, w.cut, w.terminal_repeat, w.terminal_repeat_match)
        assert (g.set_score, g.model_scores, g.score) == (w.set_score, w.model_scores, w.score)
        assert (g.metagenomic_bin is None) == (w.metagenomic_bin is None)
        if g.metagenomic_bin is not None:
            assert g.metagenomic_bin.description == w.metagenomic_bin.description
        assert texts(g, "seq%d" % i) == texts(w, "seq%d" % i), i
        n_genes += len(g)
    return n_genes


@pytest.fixture(scope="module")
def lib():
    from pyrodigal_amd import lib
    return lib


@pytest.fixture(scope="module")
def bins(lib):
    from pyrodigal_amd import benchdata
    return lib.MetagenomicBins([lib.MetagenomicBin(lib.TrainingInfo(raw=b), n) for n, b in benchdata.load_model_set()])


def finder_sequences():
    return list(contigs()[1:])                                      # (without the 120 kbp cut: the host writers are Python)


@pytest.mark.parametrize("options", [
    {"translate": True},
    {"circular": [i in (0, 1, 8) for i in range(10)]},
    {"sets": ["a", "b", None, "b", "b", "c", "a", None, "c", "a"]},
    {"regions": [[(1000, 1500)], [(0, 300), (250, 400)]] + [None] * 8, "translate": True},
    {"trim_terminal_repeats": True},
], ids=["translate", "circular", "sets", "regions", "trim"])
def test_gene_finder_on_device_sequences(ctx, lib, bins, options):
    from pyrodigal_amd import DeviceSequences
    seqs = finder_sequences()
    kw = {"mask_lowercase": True} if "regions" in options else {}
    want = lib.GeneFinder(meta=True, metagenomic_bins=bins, **kw).find_genes_batch(seqs, **options)
    _, d, ds = device_batch(None, seqs, 8)
    finder = lib.GeneFinder(meta=True, metagenomic_bins=bins, **kw)
    got = finder.find_genes_batch(ds, **options)
    assert same_genes(got, want, seqs) > 100
    assert finder.stats["device_calls"] == 1 and finder.stats["sequences"] == len(seqs)
    if "trim_terminal_repeats" in options:
        assert got[8].terminal_repeat == 40 and len(got[8].sequence) == len(seqs[8]) - 40
    d.close()


def test_gene_finder_on_device_sequences_with_training_infos(ctx, lib):
    import gzip
    from pyrodigal_amd import DeviceSequences
    blobs = [gzip.open(golden_path(n)).read() for n in ("SRR492066.training.bin.gz", "GCF_001457455.1_NCTC11397_genomic_100kb.tinf_closed.bin.gz")]
    tinfs = [lib.TrainingInfo(raw=np.frombuffer(b, np.uint8).copy()) for b in blobs]
    seqs = finder_sequences()
    ts = [tinfs[i % 2] for i in range(len(seqs))]
    want = lib.GeneFinder().find_genes_batch(seqs, training_infos=ts, translate=True)
    _, d, ds = device_batch(None, seqs, 1)
    got = lib.GeneFinder().find_genes_batch(ds, training_infos=ts, translate=True)
    assert same_genes(got, want, seqs) > 50
    assert all(g.training_info is t for g, t in zip(got, ts))
    # several device calls: each takes a subset of the (offset, length) pairs, the results do not depend on the split
    small = lib.GeneFinder(coalesce_bases=50000)
    split = small.find_genes_batch(ds, training_infos=ts, translate=True)
    assert small.stats["device_calls"] > 1
    same_genes(split, want, seqs)
    d.close()


# ---- 9. torch ------------------------------------------------------------------------------------------------------------------------
TORCH_SCRIPT = r'''
import sys
import torch                                   # first: the library then binds to the HIP runtime of torch's wheel
if not torch.cuda.is_available():
    print("torch sees no GPU")
    sys.exit(0)
sys.path.insert(0, sys.argv[1])
import numpy as np
from pyrodigal_amd import DeviceSequences, benchdata, lib

bins = lib.MetagenomicBins([lib.MetagenomicBin(lib.TrainingInfo(raw=b), n) for n, b in benchdata.load_model_set()])
seqs = [benchdata.synthetic_contig(n, gc, 900 + i) for i, (n, gc) in enumerate(((20000, 0.4), (12345, 0.6), (0, 0.5), (61, 0.5), (30011, 0.5)))]
lens = [len(s) for s in seqs]
want = lib.GeneFinder(meta=True, metagenomic_bins=bins).find_genes_batch(seqs)
alphabet = "ACGT"
index = np.zeros(256, np.int64); index[np.frombuffer(b"ACGT", np.uint8)] = np.arange(4)
host_letters = torch.from_numpy(np.frombuffer(b"".join(seqs), np.uint8).copy()).pin_memory()
host_tokens = torch.full((len(seqs), max(lens)), 7, dtype=torch.int64)              # 7: outside the alphabet, would be 'N' if read
for i, s in enumerate(seqs):
    host_tokens[i, :len(s)] = torch.from_numpy(index[np.frombuffer(s, np.uint8)])
host_tokens = host_tokens.pin_memory()
side = torch.cuda.Stream()
fields = lambda genes: [[(g.begin, g.end, g.strand, g.start_type, g.score) for g in x] for x in genes]
with torch.cuda.stream(side):
    letters = torch.full((sum(lens),), ord("N"), dtype=torch.uint8, device="cuda:0")
    tokens = torch.full((len(seqs), max(lens)), 9, dtype=torch.int64, device="cuda:0")
    letters.copy_(host_letters, non_blocking=True)
    a = lib.GeneFinder(meta=True, metagenomic_bins=bins).find_genes_batch(DeviceSequences(letters, lens))
    tokens.copy_(host_tokens, non_blocking=True)          # enqueued after the first call returned: the second call has its own wait
    b = lib.GeneFinder(meta=True, metagenomic_bins=bins).find_genes_batch(DeviceSequences(tokens, torch.tensor(lens), alphabet=alphabet))
assert DeviceSequences(tokens, lens, alphabet=alphabet).stream == torch.cuda.current_stream().cuda_stream
for got in (a, b):
    assert fields(got) == fields(want), "gene records differ"
    assert [g.sequence.data for g in got] == seqs, "letters differ"
assert sum(len(x) for x in want) > 30
print("torch device input ok: %d genes" % sum(len(x) for x in want))
'''


def test_torch_tensors_in_a_fresh_process(tmp_path):
    """torch is imported by the child alone (this process holds the library's HIP runtime and gets no second one): the child says so
    when torch sees no GPU, and the test is skipped."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "torch_device_input.py"
    script.write_text(TORCH_SCRIPT)
    done = subprocess.run([sys.executable, str(script), root], timeout=120, capture_output=True, text=True)
    assert done.returncode == 0, "child ended with %d\n%s\n%s" % (done.returncode, done.stdout[-2000:], done.stderr[-4000:])
    if "torch sees no GPU" in done.stdout:
        pytest.skip("torch sees no GPU")
    assert "torch device input ok" in done.stdout
