"""Every route of a `GeneFinder` device call (lib.pyx: the one-step call, the resident batch with masks, circles, sets, terminal
repeats, translations and tokens, a model per sequence, host and device input) against the raw layer.

`_cabi.Context.find_genes_batch` is the reference: an implementation of its own over the same C calls, given the same sequences and
options.  The packed records of a `Genes` are not readable from Python, so every record is read through the `Gene` it becomes and
compared with the values that `decode` below works out from the raw layer's record, every field of it but `contig`, and with the
`Gene` that `lib._genes_from_records` makes of the raw layer's bytes.  Device memory comes from tests/hip_mem.py (no torch)."""
import numpy as np
import pytest

from tests import hip_mem
from tests.util import synthetic_contig

pytestmark = pytest.mark.gpu

N = 5
REGIONS = [[(2000, 2400), (2300, 2500)], None, None, None, None]           # contig 0 carries the caller's regions
CIRCULAR = [True, False, True, False, True]
SETS = ["a", "b", "a", None, "b"]
MODEL_OF = [0, 1, 0, 1, 0]
SINGLE_MODELS = (7, 4)                      # of the metagenomic set: the models of `training_infos` in single mode
REPEAT = 60

ROUTES = {
    "plain": {},
    "translate": {"call": {"translate": True}},
    "masks": {"finder": {"mask": True, "mask_lowercase": True}, "call": {"regions": REGIONS}},
    "circular": {"call": {"circular": CIRCULAR}},
    "trim": {"call": {"trim_terminal_repeats": True}},
    "sets": {"call": {"sets": SETS}},
    "models": {"models": True},
    "models_circular": {"models": True, "call": {"circular": CIRCULAR}},
    "models_trim": {"models": True, "call": {"trim_terminal_repeats": True}},
    "models_translate": {"models": True, "call": {"translate": True}},
}


def contigs():
    """Five synthetic contigs of 5 .. 12 kbp: one with the caller's regions, one that ends in a copy of its first 60 bases, one with
    a lower-case run, one with a run of N, one plain."""
    a = synthetic_contig(8000, 0.5, 4101)
    b = synthetic_contig(6000, 0.45, 4102)
    c = bytearray(synthetic_contig(7001, 0.55, 4103))
    c[3000:3080] = bytes(c[3000:3080]).lower()
    d = bytearray(synthetic_contig(5003, 0.5, 4104))
    d[2500:2560] = b"N" * 60
    e = synthetic_contig(11999, 0.62, 4105)
    return [a, b + b[:REPEAT], bytes(c), bytes(d), e]


SEQS = contigs()
LIVE = []        # what a test put on the device: closed when the test ends, passed or failed, while the module's contexts still exist


@pytest.fixture(autouse=True)
def release_device_objects():
    yield
    while LIVE:
        LIVE.pop().close()


def keep(x):
    LIVE.append(x)
    return x


@pytest.fixture(scope="module")
def lib():
    from pyrodigal_amd import lib
    return lib


@pytest.fixture(scope="module")
def bins(lib):
    from pyrodigal_amd import benchdata
    return lib.MetagenomicBins([lib.MetagenomicBin(lib.TrainingInfo(raw=b), n) for n, b in benchdata.load_model_set()])


@pytest.fixture(scope="module")
def tinfs(bins):
    """Two models for single mode: members of the metagenomic set, since a model trained on a genome finds next to no gene in
    random contigs."""
    return [bins[k].training_info for k in SINGLE_MODELS]


@pytest.fixture(scope="module")
def meta_ctx(bins):
    from pyrodigal_amd import _cabi
    c = _cabi.Context(0)
    c.set_models([b.training_info.raw for b in bins])
    yield c
    c.close()


@pytest.fixture(scope="module")
def single_ctx(tinfs):
    from pyrodigal_amd import _cabi
    c = _cabi.Context(0)
    c.set_models([t.raw for t in tinfs])
    yield c
    c.close()


@pytest.fixture(scope="module")
def repeats(meta_ctx):
    """(match, trim) of every contig under the default search, by the raw layer."""
    batch = meta_ctx.upload(SEQS)
    match, trim = batch.terminal_repeats()
    batch.close()
    assert trim.tolist() == [0, REPEAT, 0, 0, 0] and match.tolist() == trim.tolist()
    return match, trim


def device_sequences(meta_ctx):
    """The contigs back to back in device memory (the context has mapped the HIP runtime that tests/hip_mem.py binds)."""
    from pyrodigal_amd import DeviceSequences
    d = keep(hip_mem.DeviceArray.from_numpy(np.frombuffer(b"".join(SEQS), np.uint8)))
    return DeviceSequences(d, [len(s) for s in SEQS])


@pytest.fixture(scope="module")
def reference(meta_ctx, single_ctx):
    """`reference(route)`: the raw layer's result of a route, computed once per module and never changed."""
    results = {}

    def of(route):
        if route not in results:
            spec = ROUTES[route]
            call = dict(spec.get("call", {}))
            call.pop("translate", None)
            kw = dict(spec.get("finder", {}))
            if spec.get("models"):
                results[route] = single_ctx.find_genes_batch(SEQS, meta=False, model_of_contig=MODEL_OF, **call, **kw)
            else:
                results[route] = meta_ctx.find_genes_batch(SEQS, meta=True, **call, **kw)
        return results[route]

    return of


FIELDS = ("begin", "end", "strand", "partial_begin", "partial_end", "start_type", "rbs_motif", "rbs_spacer", "gc_cont",
          "translation_table", "cscore", "rscore", "sscore", "tscore", "uscore", "score")
START_TYPES = ("ATG", "GTG", "TTG", "Edge")


def read(gene, k):
    return [getattr(gene, f) for f in FIELDS] + [gene._gene_data("s", k), gene._score_data(), gene.sequence()]


def decode(lib, rec, tinf):
    """What a `Gene` reports, worked out here from a raw record (every field but `contig`) and the model: the values of FIELDS, then
    the indices of the start and stop nodes."""
    w, st = tinf.rbs_weights, tinf.start_weight
    r1, r2, ms = w[rec["rbs"][0]] * st, w[rec["rbs"][1]] * st, rec["mot_score"] * st
    if tinf.uses_sd:
        best = rec["rbs"][0] if r1 > r2 else rec["rbs"][1]
    elif tinf.missing_motif_weight > -0.5 and r1 > r2 and r1 > ms:
        best = rec["rbs"][0]
    elif tinf.missing_motif_weight > -0.5 and r2 >= r1 and r2 > ms:
        best = rec["rbs"][1]
    else:
        best = None
    if best is not None:
        motif, spacer = lib._RBS_MOTIF[best], lib._RBS_SPACER[best]
    elif rec["mot_len"] == 0:
        motif = spacer = None
    else:
        motif = "".join("AGCT"[(int(rec["mot_ndx"]) >> (2 * k)) & 3] for k in range(rec["mot_len"]))
        spacer = "%dbp" % rec["mot_spacer"]
    table = int(np.frombuffer(np.asarray(tinf.raw)[8:12].tobytes(), np.int32)[0])
    return [int(rec["begin"]), int(rec["end"]), int(rec["strand"]), bool(rec["partial_begin"]), bool(rec["partial_end"]),
            START_TYPES[rec["start_type"]], motif, spacer, float(rec["gc_cont"]), table, float(rec["cscore"]), float(rec["rscore"]),
            float(rec["sscore"]), float(rec["tscore"]), float(rec["uscore"]), float(rec["cscore"]) + float(rec["sscore"]),
            int(rec["start_ndx"]), int(rec["stop_ndx"])]


def check(lib, got, raw, route, bins, tinfs, repeats, first_id=1):
    """The `Genes` of a route against the raw layer's result; returns the proteins the host translates from the raw records."""
    spec = ROUTES[route]
    call = spec.get("call", {})
    meta = not spec.get("models")
    assert len(got) == N and len(raw.genes) > 20
    proteins = []
    for i, g in enumerate(got):
        c = raw.contigs[i]
        recs = np.ascontiguousarray(raw.genes_of(i))
        assert len(g) == len(recs) and len(recs) > 0, i                    # every contig has genes, on every route
        # topology and terminal repeats
        trim = 0 if raw.terminal_repeats is None else int(raw.terminal_repeats[i])
        circular = bool("circular" in call and CIRCULAR[i]) or trim > 0
        assert (raw.cuts is not None and raw.cuts[i] >= 0) == circular, i
        assert g.circular == circular and g.cut == (int(raw.cuts[i]) if circular else None), i
        if "trim_terminal_repeats" in call:
            assert trim == repeats[1][i]
            assert (g.terminal_repeat, g.terminal_repeat_match) == (trim, int(repeats[0][i])), i
        else:
            assert raw.terminal_repeats is None and g.terminal_repeat is None and g.terminal_repeat_match is None
        # the sequence: the record without its repeat, the masks of the call
        assert len(g.sequence) == len(SEQS[i]) - trim and g.sequence.data == SEQS[i][:len(SEQS[i]) - trim], i
        want_masks = [] if raw.masks is None else [tuple(iv) for iv in raw.masks[i].tolist()]
        assert [(m.begin, m.end) for m in g.sequence.masks] == want_masks, i
        assert g.sequence.gc == c["gc"] and g.score == c["score"], i
        # the model
        if meta:
            assert c["model"] >= 0 and g.metagenomic_bin is bins[c["model"]] and g.training_info is g.metagenomic_bin.training_info, i
        else:
            assert c["model"] == MODEL_OF[i] and g.metagenomic_bin is None and g.training_info is tinfs[MODEL_OF[i]], i
        assert g.meta == meta and g._num_seq == first_id + i
        # sets
        if "sets" in call:
            assert g.set_score == (float(raw.set_scores[i]) if raw.set_models[i] >= 0 else None), i
            assert g.model_scores == {j: float(x) for j, x in enumerate(raw.model_scores[i]) if x == x}, i
            assert SETS[i] is None or (g.set_score is not None and len(g.model_scores) > 0), i
        else:
            assert raw.set_scores is None and g.set_score is None and g.model_scores is None
        # the records, field by field
        want = lib._genes_from_records(g.sequence.data, recs.tobytes(), g.training_info, first_id + i, meta, g.metagenomic_bin,
                                       circular, g.cut)
        for k, (x, w) in enumerate(zip(g, want)):
            assert read(x, k) == read(w, k), (i, k)
            assert [getattr(x, f) for f in FIELDS] + [x.start_node.i, x.stop_node.i] == decode(lib, recs[k], g.training_info), (i, k)
        proteins.append([w.translate() for w in want])
        if call.get("translate"):
            assert [x.translate() for x in g] == proteins[-1], i           # the device's letters against the host's codon loop
    if route == "masks":
        assert len(got[0].sequence.masks) == 1 and len(got[2].sequence.masks) == 1 and len(got[3].sequence.masks) == 1
    if "sets" in call:
        assert got[0].set_score == got[2].set_score and got[0].metagenomic_bin is got[2].metagenomic_bin
    return proteins


def make_finder(lib, route, bins, **kw):
    spec = ROUTES[route]
    if spec.get("models"):
        return lib.GeneFinder(**kw)
    return lib.GeneFinder(meta=True, metagenomic_bins=bins, **spec.get("finder", {}), **kw)


def call_options(route, tinfs):
    spec = ROUTES[route]
    options = dict(spec.get("call", {}))
    if spec.get("models"):
        options["training_infos"] = [tinfs[m] for m in MODEL_OF]
    return options


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_route_equals_the_raw_layer(lib, bins, tinfs, meta_ctx, reference, repeats, route, where):
    raw = reference(route)
    finder = make_finder(lib, route, bins)
    given = SEQS if where == "host" else device_sequences(meta_ctx)
    got = finder.find_genes_batch(given, **call_options(route, tinfs))
    check(lib, got, raw, route, bins, tinfs, repeats)
    assert finder.stats["device_calls"] == 1 and finder.stats["sequences"] == N


@pytest.mark.parametrize("where", ["host", "device"])
def test_find_proteins_batch_equals_the_raw_layer(lib, bins, tinfs, meta_ctx, reference, repeats, where):
    from pyrodigal_amd import ProteinTokens
    from pyrodigal_amd._cabi import AMINO_ACIDS
    spec = ProteinTokens("-" + AMINO_ACIDS + "X*", bos=23, eos=24, pad=0, dtype="int32", layout="ragged")
    raw = reference("plain")
    total = int(spec.lengths(np.ascontiguousarray(raw.genes)).sum())
    want_out, got_out = (keep(hip_mem.DeviceArray.from_numpy(np.full(total + 8, -7, np.int32))) for _ in range(2))
    for out in (want_out, got_out):
        out.shape = (total,)                                               # (eight elements behind the tensor stay as they are)
    batch = keep(meta_ctx.upload(SEQS))
    res = meta_ctx.find_genes(batch, meta=True)
    want = meta_ctx.translate_tokens(batch, res, spec, out=want_out)
    finder = make_finder(lib, "plain", bins)
    given = SEQS if where == "host" else device_sequences(meta_ctx)
    got, dp = finder.find_proteins_batch(given, spec, out=got_out)
    check(lib, got, raw, "plain", bins, tinfs, repeats)
    assert finder.stats["device_calls"] == 1 and dp.tokens is got_out
    tokens = got_out.to_numpy(np.int32)
    assert np.array_equal(tokens, want_out.to_numpy(np.int32)) and np.all(tokens[total:] == -7) and np.all(tokens[:total] >= 0)
    assert dp.lengths.tolist() == want.lengths.tolist() and dp.offsets.tolist() == want.offsets.tolist()
    assert dp.gene_begin.tolist() == want.gene_begin.tolist() == [int(c["gene_begin"]) for c in raw.contigs] + [len(raw.genes)]


def test_sequence_numbers_run_on_across_calls(lib, bins, tinfs, meta_ctx, reference, repeats):
    """The queue of the plain call and the requests that take a context for themselves number their sequences from one counter."""
    finder = make_finder(lib, "plain", bins)
    first = finder.find_genes_batch(SEQS)
    second = finder.find_genes_batch(SEQS, sets=SETS)
    third = finder.find_genes_batch(device_sequences(meta_ctx), circular=CIRCULAR)
    assert [g._num_seq for g in first + second + third] == list(range(1, 3 * N + 1))
    check(lib, second, reference("sets"), "sets", bins, tinfs, repeats, first_id=N + 1)
    check(lib, third, reference("circular"), "circular", bins, tinfs, repeats, first_id=2 * N + 1)
    assert finder.stats["device_calls"] == 3 and finder.stats["sequences"] == 3 * N


@pytest.mark.parametrize("where", ["host", "device"])
def test_a_request_split_into_two_device_calls(lib, bins, tinfs, meta_ctx, reference, repeats, where):
    """30 000 bases per device call: the first four contigs (26 064 bases) ride one call, the fifth the next."""
    assert sum(map(len, SEQS[:4])) <= 30000 < sum(map(len, SEQS))
    raw = reference("models_circular")
    finder = make_finder(lib, "models_circular", bins, coalesce_bases=30000)
    given = SEQS if where == "host" else device_sequences(meta_ctx)
    before = dict(finder.stats)
    got = finder.find_genes_batch(given, **call_options("models_circular", tinfs))
    check(lib, got, raw, "models_circular", bins, tinfs, repeats)
    assert finder.stats["device_calls"] == before["device_calls"] + 2 and finder.stats["sequences"] == before["sequences"] + N
    again = finder.find_genes_batch(given, **call_options("models_circular", tinfs))
    check(lib, again, raw, "models_circular", bins, tinfs, repeats, first_id=N + 1)
