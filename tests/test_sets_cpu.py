"""Contig sets in meta mode without a device: the reference helper tests/sets_ref.py is pinned to the reference's own
loop, the inputs of the GPU tests are shown to exercise the rule, and the host-side parts (labels, the bin map, the packing of device
calls, the refusals) are checked."""
import io
import os

import numpy as np
import pytest

from oracle import oracle as orc
from tests import sets_ref as sr
from tests.util import read_fasta, synthetic_contig

NODE_FIELDS = ["ndx", "stop_val", "type", "strand", "edge", "traceb", "tracef", "ov_mark", "elim", "mot_ndx", "mot_len", "mot_spacer",
               "mot_spacendx", "rbs", "cscore", "sscore", "rscore", "uscore", "tscore", "mot_score", "score", "gc_cont"]


@pytest.fixture(scope="module")
def bins():
    return sr.meta_bins()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def same_as_reference(mb, seq, models, closed):
    """A member of a set of its own against Oracle.find_genes_meta: model, genes, every node field, as bit patterns."""
    w, o = sr.per_contig_winner(seq, models, closed)
    assert mb.model == w
    assert mb.set_model == w
    og, on = o.genes(), o.nodes()
    assert len(mb.genes) == len(og)
    for k in ("begin", "end", "start_ndx", "stop_ndx"):
        assert np.array_equal(mb.genes[k], og[k]), k
    if w >= 0:
        assert len(mb.nodes) == len(on)
        for k in NODE_FIELDS:
            assert np.array_equal(bits(mb.nodes[k]), bits(on[k])), k
        assert bits(np.float64(mb.set_score)) == bits(np.float64(o.path_score))
    return w


def test_sets_of_one_reproduce_the_reference_on_the_fixtures(bins):
    seqs = [read_fasta(n + ".fna.gz")[0][1].encode("ascii") for n in ("SRR492066", "KK037166", "GCF_001457455.1_NCTC11397_genomic_100kb")]
    for labels in ([None] * 3, ["a", "b", "c"]):
        out = sr.find_genes_sets(seqs, labels, bins)
        assert all(same_as_reference(mb, s, bins, False) >= 0 for mb, s in zip(out, seqs))


@pytest.mark.parametrize("closed", [False, True])
def test_sets_of_one_reproduce_the_reference_on_short_contigs(bins, closed):
    seqs = [b"", b"AT", b"ATGTAA", b"N" * 400]
    seqs += [synthetic_contig(L, gc, 500 + L) for L in (61, 130, 300, 700, 1400, 1600, 2900, 3000) for gc in (0.35, 0.55, 0.66)]
    out = sr.find_genes_sets(seqs, [None] * len(seqs), bins, closed=closed)
    winners = [same_as_reference(mb, s, bins, closed) for mb, s in zip(out, seqs)]
    assert len({w for w in winners if w >= 0}) >= 4


def own_windows(seqs, models):
    return [sr.models_in(sr.gc_count(s) / len(s) if len(s) else 0.0, models) for s in seqs]


@pytest.mark.parametrize("case", [sr.case_interleaved, sr.case_mixed_gc, sr.case_many_short, sr.case_no_nodes])
def test_gpu_cases_exercise_the_rule(bins, case):
    """Every labelled input of tests/test_sets_gpu.py: at least one member ends under a model other than its own per-contig winner."""
    seqs, labels = case()
    out = sr.find_genes_sets(seqs, labels, bins)
    own = [sr.per_contig_winner(s, bins)[0] for s in seqs]
    moved = [i for i, (mb, w) in enumerate(zip(out, own)) if labels[i] is not None and mb.model != w]
    assert moved
    # ... and the unlabelled contigs of the batch are untouched
    assert all(mb.model == w for mb, w, lab in zip(out, own, labels) if lab is None)


def test_interleaved_case_shape(bins):
    seqs, labels = sr.case_interleaved()
    a = [i for i, lab in enumerate(labels) if lab == "A"]
    assert len(a) == 3 and all(2000 <= len(seqs[i]) <= 8000 for i in a)
    assert all(j - i > 1 for i, j in zip(a, a[1:]))                      # members are not adjacent
    assert None in labels and "B" in labels
    out = sr.find_genes_sets(seqs, labels, bins)
    assert len({out[i].model for i in a}) == 1 and out[a[0]].model >= 0
    assert sum(len(out[i].genes) for i in a) > 0


def test_mixed_gc_case_needs_the_pooled_window(bins):
    """(b): members are scored under models outside their own window and in a translation-table group they would not be extracted
    for, and the set's model is one of those -- per-contig windows with a pooled choice cannot give this result."""
    seqs, labels = sr.case_mixed_gc()
    out = sr.find_genes_sets(seqs, labels, bins)
    own = own_windows(seqs, bins)
    w = out[0].set_model
    assert w >= 0 and all(mb.set_model == w for mb in out)
    for mb, win in zip(out, own):
        assert not set(mb.window) & set(win)                             # the pooled window holds none of the member's own models
        own_tables = {bins[m].trans_table for m in win}
        outside = [m for m in mb.scores if bins[m].trans_table not in own_tables]
        assert outside                                                   # scored in a table group it would not otherwise extract
    assert bins[w].trans_table == 4 and all(bins[m].trans_table == 11 for win in own for m in win)
    assert all(mb.model == w and len(mb.genes) > 0 for mb in out)


def test_many_short_case_shape(bins):
    seqs, labels = sr.case_many_short()
    members = [s for s, lab in zip(seqs, labels) if lab == "many"]
    assert len(members) == 300 and all(300 <= len(s) <= 600 for s in members)
    out = sr.find_genes_sets(seqs, labels, bins)
    mm = [mb for mb, lab in zip(out, labels) if lab == "many"]
    assert any(mb.model >= 0 for mb in mm) and any(mb.model < 0 for mb in mm)    # members with and without a path under W
    assert labels.index("many") < 256 <= max(i for i, lab in enumerate(labels) if lab == "many")   # the sum crosses a workgroup of 256 contigs


def test_no_nodes_and_no_model_cases(bins):
    seqs, labels = sr.case_no_nodes()
    out = sr.find_genes_sets(seqs, labels, bins)
    for mb, lab in zip(out, labels):
        if lab == "empty":
            o, scores = sr.walk(mb.seq, bins, mb.window, orc.Params())
            assert o.num_nodes == 0 and not scores
        if lab in ("empty", "nopath"):
            assert mb.window and mb.set_model == -1 and np.isnan(mb.set_score) and mb.model == -1 and len(mb.genes) == 0
    assert sr.walk(seqs[labels.index("nopath")], bins, out[labels.index("nopath")].window, orc.Params())[0].num_nodes > 0
    seqs, labels, subset = sr.case_no_model()
    models = [bins[m] for m in subset]
    out = sr.find_genes_sets(seqs, labels, models)
    assert out[0].window == [] and out[0].set_model == -1 and out[1].model == -1
    assert out[2].model >= 0                                             # (the unlabelled high-GC contig has one)
    assert sr.per_contig_winner(seqs[0], models)[0] == -1


# ---- host-side parts -------------------------------------------------------------------------------------------------------------------

def test_dense_set_ids():
    from pyrodigal_amd import _cabi
    ids = _cabi.dense_set_ids(["b", None, ("x", 1), "b", -1, 7, ("x", 1)], 7)
    assert ids.dtype == np.int32 and ids.tolist() == [0, -1, 1, 0, -1, 2, 1]
    assert _cabi.dense_set_ids([], 0).tolist() == []
    with pytest.raises(ValueError, match="3 entries for 2"):
        _cabi.dense_set_ids(["a", "b", "c"], 2)
    assert sr.dense_sets(["b", None, "c", "b"]) == [0, 1, 2, 0]


def test_parse_bin_map():
    from pyrodigal_amd import cli
    text = ["# contig\tbin\n", "c1\tbin.1\n", "\n", b"c2\tbin.2\r\n", "c3\tbin.1", "c1\tbin.1\n"]
    assert cli.parse_bin_map(text) == {"c1": "bin.1", "c2": "bin.2", "c3": "bin.1"}
    for bad in ("c1 bin.1\n", "c1\t\n", "\tbin\n", "c1\tb\textra\n"):
        with pytest.raises(ValueError, match="line 2"):
            cli.parse_bin_map(["c0\tb\n", bad], "map.tsv")
    with pytest.raises(ValueError, match="line 3.*'c1'"):
        cli.parse_bin_map(["c1\ta\n", "c2\ta\n", "c1\tb\n"])


def test_plan_set_calls():
    from pyrodigal_amd.pipeline import plan_set_calls
    ids = ["r0", "r1", "r2", "r3", "r4", "r5", "r6"]
    lens = [40, 10, 30, 50, 20, 200, 10]
    by_id = {"r0": "A", "r2": "B", "r4": "A", "r6": "B", "r5": "C", "nope": "A"}
    labels, calls, unmatched = plan_set_calls(ids, lens, by_id, 100)
    assert labels == ["A", None, "B", None, "A", "C", "B"] and unmatched == ["nope"]
    # sets in order of first appearance: A (60), r1 (10) | B (40), r3 (50) | C (200: larger than a call, on its own)
    assert calls == [[0, 1, 4], [2, 3, 6], [5]]
    for lab in ("A", "B", "C"):
        assert len({k for k, call in enumerate(calls) for i in call if labels[i] == lab}) == 1      # a set sits in one call
    assert sorted(i for call in calls for i in call) == list(range(7))
    assert plan_set_calls(ids, lens, {}, 1 << 30)[1] == [list(range(7))]
    assert plan_set_calls([], [], {"x": "A"}, 10) == ([], [], ["x"])


def test_command_line_refusals(tmp_path):
    from pyrodigal_amd import cli
    fa = tmp_path / "in.fa"
    fa.write_text(">c1\nACGT\n")
    good = tmp_path / "map.tsv"
    good.write_text("c1\tbin1\n")
    bad = tmp_path / "bad.tsv"
    bad.write_text("c1\tbin1\nc2 bin1\n")

    def run(*argv):
        err = io.StringIO()
        rc = cli.main(list(argv), stdout=io.BytesIO(), stderr=err)
        return rc, err.getvalue()

    rc, msg = run("-i", str(fa), "--bin-map", str(good))
    assert rc == 1 and "--bin-map" in msg and "-p meta" in msg
    for opt in (["--circular"], ["--circular-from-header"], ["--circular-ids", str(good)]):
        rc, msg = run("-i", str(fa), "-p", "meta", "--meta-bins", "x.bin", "--bin-map", str(good), *opt)
        assert rc == 1 and "--bin-map" in msg and "--circular" in msg
    rc, msg = run("-i", str(fa), "-p", "meta", "--meta-bins", "x.bin", "--bin-map", str(bad))
    assert rc == 1 and "--bin-map" in msg and "line 2" in msg
    rc, msg = run("-i", str(fa), "-p", "meta", "--meta-bins", "x.bin", "--bin-map", str(tmp_path / "missing.tsv"))
    assert rc == 1 and "--bin-map" in msg


def test_library_refusals_need_no_device(bins):
    from pyrodigal_amd import lib
    mb = lib.MetagenomicBins([lib.MetagenomicBin(lib.TrainingInfo(raw=b.tobytes()), "bin %d" % i) for i, b in enumerate(bins[:2])])
    meta = lib.GeneFinder(meta=True, metagenomic_bins=mb)
    seqs = [b"ACGT" * 100, b"ACGT" * 50]
    with pytest.raises(ValueError, match="1 entries for 2"):
        meta.find_genes_batch(seqs, sets=["a"])
    with pytest.raises(ValueError, match="circular"):
        meta.find_genes_batch(seqs, sets=["a", "a"], circular=[True, False])
    with pytest.raises(ValueError, match="training_infos"):
        meta.find_genes_batch(seqs, sets=["a", "a"], training_infos=[None, None])
    with pytest.raises(ValueError, match="single mode"):
        lib.GeneFinder(meta=False).find_genes_batch(seqs, sets=["a", "a"])
    from pyrodigal_amd.pipeline import render_fasta
    with pytest.raises(ValueError, match="meta-mode"):
        render_fasta(os.devnull, [], gff=io.BytesIO(), meta=False, sets_by_id={})
    with pytest.raises(ValueError, match="circular"):
        render_fasta(os.devnull, [], gff=io.BytesIO(), meta=True, sets_by_id={}, circular=True)


def test_new_entry_points_are_exported():
    import ctypes
    from pyrodigal_amd import _cabi
    L = ctypes.CDLL(_cabi.LIB_PATH)
    for name in ("pga_batch_set_sets", "pga_set_choice", "pga_model_scores", "pga_render_seqnums"):
        assert name in _cabi.EXPORTS and hasattr(L, name)
    # host arithmetic of the two getters on a handle-free path: bad arguments are refused, not dereferenced
    L.pga_set_choice.restype = ctypes.c_int
    L.pga_model_scores.restype = ctypes.c_int
    assert L.pga_set_choice(None, 1, None, None) == _cabi.PGA_EINVAL
    assert L.pga_model_scores(None, 1, 1, None) == _cabi.PGA_EINVAL
    assert L.pga_batch_set_sets(None, None) == _cabi.PGA_EINVAL
