"""pyrodigal_amd.pipeline without a device and without the built library: fakes stand in for ``_cabi.Context`` and
``_cabi.FastaReader``, and the three public functions are checked for what their callers rely on -- results in input order whatever
order the contexts finish in, a bounded number of batches pulled ahead of the consumer, a worker's exception raised at its place
in the order, an error of the source itself, a consumer that stops early, and, in all of these, threads joined, arenas handed
back, and the contexts and the reader closed by whoever owns them.

The fake run calls sleep a random few milliseconds, so completion order differs from submission order.  These are
characterization tests: they passed unchanged on the three hand-written loops that the pool replaced."""
import io
import random
import threading
import time

import pytest

from pyrodigal_amd import _cabi, pipeline

N_ITEMS = 40
SOURCE_FAILS_AFTER = 5


class Boom(Exception):
    pass


class FakeResult:
    def __init__(self, name, n_genes):
        self.name, self.genes, self.terminal_repeats = name, [0] * n_genes, None


class FakeBatch:
    def __init__(self, name, n):
        self.name, self.n, self.closed = name, n, 0

    def set_masks(self, regions=None, mask_lowercase=False):
        pass

    def set_circular(self, circular=None):
        pass

    def set_sets(self, labels):
        self.sets = list(labels)

    def close(self):
        self.closed += 1


class FakePacked:
    """What ``FastaReader.packed_batches`` yields: batch ``k`` of the fake file holds ``1 + k % 3`` records."""

    def __init__(self, world, k):
        self.world, self.k, self.n = world, k, 1 + k % 3
        self.ids = ["b%d_r%d" % (k, i) for i in range(self.n)]
        self.descriptions = ["batch %d" % k] * self.n
        self.lens = [100 + k + i for i in range(self.n)]
        self.total = sum(self.lens)
        self.released, self.release_calls = False, 0

    def sequence(self, i):
        assert not self.released, "the letters of batch %d were read after its arena was released" % self.k
        return b"A" * self.lens[i]

    def release(self):                      # idempotent, like PackedRecords.release
        self.release_calls += 1
        self.released = True


class World:
    """The state the fakes share with a test: what was created, pulled, yielded and closed."""

    def __init__(self, n_items=N_ITEMS, fail_at=None, source_fails_after=None, hold_first=False):
        self.n_items, self.fail_at, self.source_fails_after, self.hold_first = n_items, fail_at, source_fails_after, hold_first
        self.rng = random.Random(5)
        self.contexts, self.readers, self.packed, self.batches = [], [], [], []
        self.pulled = self.yielded = self.most_ahead = 0
        self.error = Boom("item %r" % (fail_at,))
        self.source_error = Boom("source")
        self.failed = threading.Event()
        self.threads_before = set(threading.enumerate())

    def pull(self):
        self.pulled += 1
        self.most_ahead = max(self.most_ahead, self.pulled - self.yielded)

    def run(self, k):
        """The body of a fake run call on item ``k``."""
        if self.hold_first and k == 0:          # item 0 ends only after the failure of item `fail_at` is known
            assert self.failed.wait(10)
            time.sleep(0.03)
        else:
            time.sleep(self.rng.uniform(0.0, 0.004))
        if k == self.fail_at:
            self.failed.set()
            raise self.error

    def stream_source(self):
        for k in range(self.n_items):
            if k == self.source_fails_after:
                raise self.source_error
            self.pull()
            yield ["contig_of_%d" % k]

    def pool_threads(self):
        return set(threading.enumerate()) - self.threads_before

    def consume(self, gen, out):
        for x in gen:
            self.yielded += 1
            out.append(x)


class FakeContext:
    world = None

    def __init__(self, device=0):
        self.device, self.closed, self.models = device, 0, None
        self._models = []
        self.world.contexts.append(self)

    def set_models(self, blobs):
        self.models = list(blobs)

    def close(self):
        self.closed += 1

    def find_genes_batch(self, batch, **kw):
        k = int(batch[0].rsplit("_", 1)[1])
        self.world.run(k)
        return FakeResult("stream%d" % k, k)

    def upload_packed(self, pb):
        pb.release()
        b = FakeBatch(pb.k, pb.n)
        self.world.batches.append(b)
        return b

    def upload(self, seqs):
        b = FakeBatch(None, len(seqs))
        self.world.batches.append(b)
        return b

    def find_genes(self, batch, **kw):
        if batch.name is None:
            time.sleep(self.world.rng.uniform(0.0, 0.004))
            return FakeResult("call", 2 * batch.n)
        self.world.run(batch.name)
        return FakeResult("file%d" % batch.name, batch.name)

    def render_genes(self, batch, result, ids, formats, *, meta=False, descriptions=None, first_seqnum=1, unbinned_model=None,
                     seqnums=None):
        seqnums = list(seqnums) if seqnums is not None else [first_seqnum + i for i in range(len(ids))]
        out = {}
        for name in formats:
            pieces = [("%s %s batch=%s seqnum=%d\n" % (name, rid, batch.name, s)).encode() for rid, s in zip(ids, seqnums)]
            offs = [0]
            for p in pieces:
                offs.append(offs[-1] + len(p))
            out[name] = _cabi.RenderedText(b"".join(pieces), offs, 1, 0.5)
        return out


class FakeReader:
    world = None
    records = None                          # what batches() yields, for the sets variant

    def __init__(self, path):
        self.path, self.closed, self.n_arenas = path, 0, None
        self.world.readers.append(self)

    def close(self):
        self.closed += 1

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def batches(self, max_bases=64 << 20, max_records=0):
        yield list(self.records[:2])
        yield list(self.records[2:])

    def packed_batches(self, max_bases=64 << 20, max_records=0, n_arenas=3):
        w = self.world
        self.n_arenas = n_arenas
        for k in range(w.n_items):
            held = sum(1 for pb in w.packed if not pb.released)
            assert held < n_arenas, "asked for batch %d while %d of %d arenas are unreleased" % (k, held, n_arenas)
            if k == w.source_fails_after:
                raise w.source_error
            w.pull()
            pb = FakePacked(w, k)
            w.packed.append(pb)
            yield pb


@pytest.fixture
def world(monkeypatch):
    def make(**kw):
        w = World(**kw)
        monkeypatch.setattr(pipeline._cabi, "Context", type("Ctx", (FakeContext,), {"world": w}))
        monkeypatch.setattr(pipeline._cabi, "FastaReader", type("Reader", (FakeReader,), {"world": w}))
        return w
    return make


# ---- the three public functions behind one face: (generator, key of a yielded item, in-flight bound) --------------------------------

def run_stream(w, n, contexts=None):
    assert contexts is None
    return pipeline.find_genes_stream(w.stream_source(), [b"m"], n_contexts=n), lambda x: x[1].name, 2 * n


def run_fasta(w, n, contexts=None):
    return (pipeline.find_genes_fasta("file.fa", [b"m"], n_contexts=n, contexts=contexts), lambda x: x[3].name, n + 1)


KINDS = {"stream": run_stream, "fasta": run_fasta}
NAME = {"stream": "stream%d", "fasta": "file%d"}


def check_teardown(w, owned=True, passed=()):
    assert not w.pool_threads()
    assert all(pb.released for pb in w.packed)
    assert all(b.closed == 1 for b in w.batches)
    assert all(r.closed >= 1 for r in w.readers)
    if owned:
        assert w.contexts and all(c.closed == 1 for c in w.contexts)
    assert all(c.closed == 0 for c in passed)


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_results_come_back_in_input_order_within_the_bound(world, kind, n):
    w = world()
    gen, key, ahead = KINDS[kind](w, n)
    got = []
    w.consume(gen, got)
    assert [key(x) for x in got] == [NAME[kind] % k for k in range(N_ITEMS)]
    assert len(w.contexts) == n and all(c.models == [b"m"] for c in w.contexts)
    assert w.pulled == N_ITEMS and 1 <= w.most_ahead <= ahead
    if kind == "fasta":
        assert w.readers[0].n_arenas == n + 2
        assert [list(x[0]) for x in got] == [pb.ids for pb in w.packed] and [list(x[2]) for x in got] == [pb.lens for pb in w.packed]
    check_teardown(w)


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_a_failing_item_is_raised_at_its_place(world, kind, n):
    w = world(fail_at=7)
    gen, key, ahead = KINDS[kind](w, n)
    got = []
    with pytest.raises(Boom) as err:
        w.consume(gen, got)
    assert err.value is w.error
    assert [key(x) for x in got] == [NAME[kind] % k for k in range(7)]
    assert 8 <= w.pulled <= 7 + ahead and w.most_ahead <= ahead
    check_teardown(w)


@pytest.mark.parametrize("kind,n", [("stream", 4), ("fasta", 7)])
def test_nothing_is_pulled_once_a_failure_is_known(world, kind, n):
    """Eight items in flight (the bound of both cases); item 7 fails while the consumer still waits for item 0, which ends only
    after that: the items before the failure are yielded, and no ninth item is pulled on the way to it."""
    w = world(fail_at=7, hold_first=True)
    gen, key, ahead = KINDS[kind](w, n)
    assert ahead == 8
    got = []
    with pytest.raises(Boom) as err:
        w.consume(gen, got)
    assert err.value is w.error and len(got) == 7
    assert w.pulled == 8
    check_teardown(w)


def test_a_failing_item_leaves_passed_contexts_open(world):
    w = world(fail_at=7)
    mine = [FakeContext.__new__(FakeContext) for _ in range(2)]
    for c in mine:
        c.closed, c.world = 0, w
    gen, key, ahead = run_fasta(w, 5, contexts=mine)
    got = []
    with pytest.raises(Boom):
        w.consume(gen, got)
    assert len(got) == 7 and not w.contexts           # none created
    assert w.readers[0].n_arenas == 4                   # sized by the contexts that were passed
    check_teardown(w, owned=False, passed=mine)


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_an_error_of_the_source_reaches_the_caller(world, kind, n):
    """The source is asked for its next item as soon as the bound allows, so its error arrives while up to ``ahead - 1`` results
    are still outstanding: those are worked (their arenas go back) and dropped."""
    w = world(source_fails_after=SOURCE_FAILS_AFTER)
    gen, key, ahead = KINDS[kind](w, n)
    got = []
    with pytest.raises(Boom) as err:
        w.consume(gen, got)
    assert err.value is w.source_error
    assert w.pulled == SOURCE_FAILS_AFTER
    assert [key(x) for x in got] == [NAME[kind] % k for k in range(max(0, SOURCE_FAILS_AFTER - ahead + 1))]
    if kind == "fasta":
        assert len(w.batches) == SOURCE_FAILS_AFTER   # every pulled batch went through the upload
    check_teardown(w)


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_a_consumer_that_stops_early(world, kind, n):
    w = world()
    gen, key, ahead = KINDS[kind](w, n)
    first = next(gen)
    assert key(first) == NAME[kind] % 0
    gen.close()
    assert w.pulled <= ahead
    check_teardown(w)


def test_early_close_leaves_passed_contexts_open(world):
    w = world()
    mine = [FakeContext.__new__(FakeContext) for _ in range(2)]
    for c in mine:
        c.closed, c.world = 0, w
    gen = pipeline.find_genes_fasta("file.fa", [b"m"], contexts=mine)
    next(gen)
    gen.close()
    check_teardown(w, owned=False, passed=mine)


# ---- render_fasta ---------------------------------------------------------------------------------------------------------------------

class CountingSink(io.BytesIO):
    """A sink that counts a batch as yielded when its text arrives."""

    def __init__(self, w):
        super().__init__()
        self.w = w

    def write(self, data):
        self.w.yielded += 1
        return super().write(data)


@pytest.mark.parametrize("n", [1, 2, 3])
def test_render_fasta_writes_every_sink_in_file_order(world, n):
    w = world()
    gff, faa = CountingSink(w), io.BytesIO()
    stats = pipeline.render_fasta("file.fa", [b"m"], gff=gff, faa=faa, n_contexts=n, first_seqnum=11)
    want = {"gff": [], "faa": []}
    seqnum = 11
    for pb in w.packed:
        for rid in pb.ids:
            for name in want:
                want[name].append(("%s %s batch=%d seqnum=%d\n" % (name, rid, pb.k, seqnum)).encode())
            seqnum += 1
    assert gff.getvalue() == b"".join(want["gff"]) and faa.getvalue() == b"".join(want["faa"])
    assert len(w.packed) == N_ITEMS and w.most_ahead <= n + 1 and w.readers[0].n_arenas == n + 2
    assert stats["records"] == sum(pb.n for pb in w.packed) == seqnum - 11
    assert stats["bases"] == sum(pb.total for pb in w.packed)
    assert stats["genes"] == sum(range(N_ITEMS))
    assert stats["fallback"] == 2 * N_ITEMS and stats["kernel_ms"] == {"gff": 0.5 * N_ITEMS, "faa": 0.5 * N_ITEMS}
    assert stats["regions_unmatched"] == [] and stats["circular_unmatched"] == []
    check_teardown(w)


def test_render_fasta_reads_the_letters_of_circles_before_the_upload(world, monkeypatch):
    """With GenBank output and circular records the host writer needs the letters, which live in the arena the upload releases."""
    w = world(n_items=4)
    seen = []
    monkeypatch.setattr(pipeline, "_host_genbank", lambda ctx, r, ids, letters, flags, options, meta, seqnum:
                        seen.append((seqnum, [len(s) for s in letters], flags)) or _cabi.RenderedText(b"G%d\n" % seqnum, [0], 0, 0.0))
    gbk = io.BytesIO()
    stats = pipeline.render_fasta("file.fa", [b"m"], gbk=gbk, circular=True)
    assert gbk.getvalue() == b"G1\nG2\nG4\nG7\n"
    assert sorted(seen) == [(1, [100], [True]), (2, [101, 102], [True] * 2), (4, [102, 103, 104], [True] * 3), (7, [103], [True])]
    assert stats["records"] == 7
    check_teardown(w)


def test_render_fasta_failure_in_the_middle(world):
    w = world(fail_at=7)
    gff = io.BytesIO()
    with pytest.raises(Boom) as err:
        pipeline.render_fasta("file.fa", [b"m"], gff=gff, n_contexts=2)
    assert err.value is w.error
    assert gff.getvalue().count(b"\n") == sum(pb.n for pb in w.packed[:7])       # the batches before it were written
    assert 8 <= w.pulled <= 7 + 3
    check_teardown(w)


@pytest.mark.parametrize("n", [1, 3])
def test_render_fasta_with_sets_writes_in_file_order(world, n):
    """Three device calls of at most 310 bases (two sets of 250 bases each, then a record on its own together with a one-record
    set); the records of set A are the 1st, 3rd and 5th of the file, so the text of every call is interleaved with the others'."""
    w = world()
    ids = ["r0", "r1", "r2", "r3", "r4", "r5", "r6"]
    lens = [100, 120, 100, 130, 50, 300, 10]
    pipeline._cabi.FastaReader.records = [(i, "d", b"A" * n_) for i, n_ in zip(ids, lens)]
    sets = {"r0": "A", "r2": "A", "r4": "A", "r1": "B", "r3": "B", "r6": "C", "ghost": "Z"}
    gff = io.BytesIO()
    stats = pipeline.render_fasta("file.fa", [b"m"], gff=gff, meta=True, sets_by_id=sets, max_bases=310, n_contexts=n, first_seqnum=5)
    assert gff.getvalue() == b"".join(("gff %s batch=None seqnum=%d\n" % (rid, 5 + i)).encode() for i, rid in enumerate(ids))
    assert stats["device_calls"] == 3 and stats["sets_unmatched"] == ["ghost"]
    assert sorted((b.sets for b in w.batches), key=len, reverse=True) == [["A", "A", "A"], ["B", "B"], [None, "C"]]
    assert stats["records"] == 7 and stats["bases"] == sum(lens) and stats["genes"] == 14
    assert stats["fallback"] == 3 and stats["kernel_ms"] == {"gff": 1.5}
    assert stats["regions_unmatched"] == [] and stats["circular_unmatched"] == []
    check_teardown(w)


def test_render_fasta_with_sets_of_a_file_without_records(world):
    w = world()
    pipeline._cabi.FastaReader.records = []
    gff = io.BytesIO()
    stats = pipeline.render_fasta("file.fa", [b"m"], gff=gff, meta=True, sets_by_id={"ghost": "Z"}, n_contexts=2)
    assert gff.getvalue() == b"" and stats["device_calls"] == 0 and stats["records"] == 0 and stats["sets_unmatched"] == ["ghost"]
    check_teardown(w)
