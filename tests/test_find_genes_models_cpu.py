"""Argument checks of GeneFinder.find_genes_batch(..., training_infos=...) and of the model-per-contig C entry point: all of
them happen before any device work, so they hold without a GPU."""
import pytest

from tests.util import golden_path


@pytest.fixture(scope="module")
def lib():
    try:
        from pyrodigal_amd import lib as L
    except ImportError:
        import __graft_entry__
        __graft_entry__.build_cython_host()
        from pyrodigal_amd import lib as L
    return L


def test_training_infos_argument_errors(lib):
    t = lib.TrainingInfo.load(golden_path("SRR492066.training.bin.gz"))
    seqs = ["ACGT" * 10000, "GGCC" * 10000]
    with pytest.raises(ValueError, match="meta"):
        lib.GeneFinder(meta=True).find_genes_batch(seqs, training_infos=[t, t])
    with pytest.raises(ValueError, match="2 sequences"):
        lib.GeneFinder().find_genes_batch(seqs, training_infos=[t])
    with pytest.raises(ValueError):
        lib.GeneFinder(t).find_genes_batch(seqs, training_infos=[t, t, t])
    with pytest.raises(TypeError, match=r"training_infos\[1\]"):
        lib.GeneFinder().find_genes_batch(seqs, training_infos=[t, t.raw])
    assert lib.GeneFinder().find_genes_batch([], training_infos=[]) == []


def test_model_of_contig_length_is_checked_on_the_host():
    from pyrodigal_amd import _cabi

    class FakeBatch:
        n, h = 3, None
    with pytest.raises(ValueError, match="3 contigs"):
        _cabi._find_genes(object(), FakeBatch(), meta=False, model_of_contig=[0, 1])


def test_train_batch_argument_errors(lib):
    seqs = ["ACGT" * 10000, "GGCC" * 10000]
    with pytest.raises(RuntimeError):
        lib.GeneFinder(meta=True).train_batch(seqs)
    with pytest.raises(ValueError, match="genome 1"):
        lib.GeneFinder().train_batch([seqs[0], "ACGT" * 100])
    with pytest.raises(ValueError, match="genome 0"):
        lib.GeneFinder().train_batch(seqs, translation_table=[7, 11])
    with pytest.raises(ValueError, match="2 genomes"):
        lib.GeneFinder().train_batch(seqs, start_weight=[4.35])
    assert lib.GeneFinder().train_batch([]) == []
