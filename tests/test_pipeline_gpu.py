"""pyrodigal_amd.pipeline on the device, where the pool's edges meet real contexts and a real reader: a consumer that stops
after one batch, a device call that fails in the middle of a file, and text output cut into batches on one and on three contexts.
One small file throughout: 8 synthetic records of 3 000 to 6 000 bases, read 12 000 bases a batch."""
import io

import pytest

pytestmark = pytest.mark.gpu

MAX_BASES = 12_000
# a batch is the shortest run of records that reaches the budget: two, two, three records and one -- four batches; the lengths of
# the third batch are the file's only ones of their kind, so a record of it can be named by its length
LENGTHS = [6000, 6000, 6000, 6000, 5531, 5024, 3000, 3211]


@pytest.fixture(scope="module")
def models():
    from pyrodigal_amd import benchdata
    return [b for _, b in benchdata.load_model_set()]


@pytest.fixture(scope="module")
def path(tmp_path_factory):
    from pyrodigal_amd import benchdata
    p = tmp_path_factory.mktemp("pipeline") / "eight.fna"
    with open(p, "w") as f:
        for k, n in enumerate(LENGTHS):
            s = benchdata.synthetic_contig(n, 0.35 + 0.04 * k, 9100 + k).decode()
            f.write(">rec%d of %d bases\n" % (k, n))
            f.writelines(s[i:i + 70] + "\n" for i in range(0, n, 70))
    return str(p)


def genes_by_batch(batches):
    return [(list(ids), [int(x) for x in lens], res.contigs["model"].tolist(), res.genes.tobytes()) for ids, _, lens, res in batches]


@pytest.fixture(scope="module")
def clean(path, models):
    """The file's batches on fresh contexts, computed once."""
    from pyrodigal_amd import pipeline
    got = genes_by_batch(pipeline.find_genes_fasta(path, models, n_contexts=2, max_bases=MAX_BASES, meta=True))
    assert [len(b[0]) for b in got] == [2, 2, 3, 1] and [i for b in got for i in b[0]] == ["rec%d" % k for k in range(len(LENGTHS))]
    assert [n for b in got for n in b[1]] == LENGTHS and sum(len(b[3]) for b in got) > 0
    return got


@pytest.fixture
def ctxs(models):
    from pyrodigal_amd import _cabi
    made = [_cabi.Context(0) for _ in range(2)]
    for c in made:
        c.set_models(models)
    yield made
    for c in made:
        c.close()


def test_a_consumer_that_stops_after_one_batch_leaves_the_contexts_usable(path, models, ctxs, clean):
    from pyrodigal_amd import pipeline
    gen = pipeline.find_genes_fasta(path, models, max_bases=MAX_BASES, contexts=ctxs, meta=True)
    first = next(gen)
    gen.close()
    assert genes_by_batch([first]) == clean[:1]
    assert genes_by_batch(pipeline.find_genes_fasta(path, models, max_bases=MAX_BASES, contexts=ctxs, meta=True)) == clean


def test_a_call_that_fails_in_the_middle_of_a_file(path, models, ctxs, clean, monkeypatch):
    """The third batch's call fails on the host before anything is launched (``PGA_FAULT_CONTIG_LEN`` names one of its records by
    length): the two batches before it arrive, then the error; the same contexts then read the whole file as if nothing had
    happened."""
    from pyrodigal_amd import _cabi, pipeline
    monkeypatch.setenv("PGA_FAULT_CONTIG_LEN", str(clean[2][1][0]))
    got = []
    with pytest.raises(_cabi.PgaError, match="PGA_FAULT_CONTIG_LEN"):
        for item in pipeline.find_genes_fasta(path, models, max_bases=MAX_BASES, contexts=ctxs, meta=True):
            got.append(item)
    assert genes_by_batch(got) == clean[:2]
    monkeypatch.delenv("PGA_FAULT_CONTIG_LEN")
    assert genes_by_batch(pipeline.find_genes_fasta(path, models, max_bases=MAX_BASES, contexts=ctxs, meta=True)) == clean


@pytest.fixture(scope="module")
def gff_in_one_batch(path, models):
    from pyrodigal_amd import pipeline
    out = io.BytesIO()
    stats = pipeline.render_fasta(path, models, gff=out, meta=True)
    assert stats["records"] == len(LENGTHS) and stats["bases"] == sum(LENGTHS) and stats["genes"] > 0
    return out.getvalue(), stats


@pytest.mark.parametrize("n_contexts", [1, 3])
def test_render_fasta_in_batches_writes_what_one_batch_writes(path, models, gff_in_one_batch, n_contexts):
    from pyrodigal_amd import pipeline
    want, want_stats = gff_in_one_batch
    out = io.BytesIO()
    stats = pipeline.render_fasta(path, models, gff=out, meta=True, n_contexts=n_contexts, max_bases=MAX_BASES)
    assert out.getvalue() == want
    assert [stats[k] for k in ("records", "bases", "genes")] == [want_stats[k] for k in ("records", "bases", "genes")]
