"""The mask-union builder -- pga_launch_mask_union: k_mask_paint_runs / find_runs, k_mask_paint_regions, k_mask_count, k_scan_counts,
k_mask_place -- on the catalogue of tests/mask_shapes.py: every reported list against the plain union of tests/mask_ref.py, every
node of the extraction behind it against the oracle (runs of unknown bases) or tests/extract_ref.py (known bases under a mask), and
one finder call over the joints and the run walk.  tests/test_mask_shapes_cpu.py proves from the reference alone that the catalogue
reaches every edge; here only the device is in question."""
import pytest

from oracle import oracle as orc
from tests import mask_shapes as ms
from tests.extract_ref import extract_ref
from tests.test_extract_shapes_gpu import check_topo
from tests.test_finder_gpu import compare_contig
from tests.test_stages_gpu import check
from tests.util import golden_path

pytestmark = pytest.mark.gpu

SERIES = ("bit", "lanes", "group", "joint", "short", "walk", "byte", "together", "densest")
_CATALOGUE, _REF, _NODES = [], {}, {}


@pytest.fixture(scope="module")
def ctx():
    from pyrodigal_amd import _cabi
    c = _cabi.Context(0)
    yield c
    c.close()


def shapes_of(series):
    if not _CATALOGUE:
        _CATALOGUE.extend(ms.catalogue())
    return [sh for sh in _CATALOGUE if sh.name.split("/")[0] == series]


def reference(sh):
    """The reference of a shape, computed once and left unchanged."""
    if sh.name not in _REF:
        _REF[sh.name] = [r.tolist() for r in ms.reference(sh)]
    return _REF[sh.name]


def orders(sh):
    """Catalogue order and the one fixed permutation (which moves every contig to another place of the bitmap)."""
    n = len(sh.seqs)
    return [list(range(n)), ms.permuted(n)] if n > 1 else [[0]]


def call(ctx, sh, idx, stage, **override):
    kw = dict(mask=sh.mask, min_mask=sh.min_mask, mask_lowercase=sh.lower, regions=None if sh.regions is None else [sh.regions[k] for k in idx])
    kw.update(override)
    return ctx.nodes_stage([sh.seqs[k] for k in idx], stage, **kw)


def harmless_source(sh, idx):
    """A second source that changes no list and forces the builder: a one-base named region inside the first masked run; where
    nothing is masked, lower-case masking (a shape of unknown runs holds no lower-case letter but n, which is unknown itself)."""
    ref = reference(sh)
    for at, k in enumerate(idx):
        if ref[k]:
            regions = [None] * len(idx)
            regions[at] = [(ref[k][0][0], ref[k][0][0] + 1)]
            return dict(regions=regions)
    return dict(mask_lowercase=True)


def check_lists(ctx, sh):
    from pyrodigal_amd import _cabi
    ref = reference(sh)
    for idx in orders(sh):
        want = [ref[k] for k in idx]
        got = call(ctx, sh, idx, _cabi.STAGE_SEQUENCE).masks
        assert [m.tolist() for m in got] == want, (sh.name, idx[:3])
        if ms.pure_unknown(sh):         # `mask=True` alone is the host-ordered path (k_find_masks); a second source forces the builder
            forced = call(ctx, sh, idx, _cabi.STAGE_SEQUENCE, **harmless_source(sh, idx)).masks
            assert [m.tolist() for m in forced] == want, (sh.name, idx[:3], "builder")


@pytest.mark.parametrize("series", SERIES)
def test_every_list_is_the_union(ctx, series):
    shapes = shapes_of(series)
    assert shapes
    for sh in shapes:
        check_lists(ctx, sh)


@pytest.mark.parametrize("n_groups", ms.SCAN_GROUPS)
def test_scan_rounds(ctx, n_groups):
    """4 095, 4 096 and 4 097 counts: one round of k_scan_counts not full, exactly full, and a second round whose carry holds one
    start more than ends."""
    for sh in ms.scan_shapes(n_groups):
        assert ms.groups_of(sh.seqs) == n_groups
        check_lists(ctx, sh)


def node_reference(sh, k):
    """Nodes of contig k of a shape under its reference list: the oracle where the masked bases are all unknown or nothing is masked,
    the restated sweep otherwise.  (kind, nodes), computed once per (letters, list)."""
    s, r = sh.seqs[k], reference(sh)[k]
    oracle_masks = ms.pure_unknown(sh)
    key = (s, tuple(map(tuple, r)), oracle_masks, sh.min_mask)
    if key not in _NODES:
        if oracle_masks or not r:
            o = orc.Oracle(s, mask=oracle_masks, mask_size=sh.min_mask)
            o.extract(11, orc.Params())
            o.sort()
            _NODES[key] = ("oracle", o.nodes())
        else:
            _NODES[key] = ("restated", extract_ref(s, r))
    return _NODES[key]


@pytest.mark.parametrize("series", SERIES)
def test_every_node_behind_the_union(ctx, series):
    from pyrodigal_amd import _cabi
    total = 0
    for sh in shapes_of(series):
        for idx in orders(sh):
            out = call(ctx, sh, idx, _cabi.STAGE_EXTRACT)
            assert len(out) == len(idx)
            for nd, k in zip(out, idx):
                kind, want = node_reference(sh, k)
                if kind == "oracle":
                    check(nd, want, 1)
                else:
                    check_topo(nd, want, (sh.name, k))
                total += nd["n"]
    assert total > 0


def test_masking_changes_the_nodes(ctx):
    """The comparison above is not vacuous: under its masks a shape holds another number of nodes than without them, for at least
    as many shapes as tests/test_mask_shapes_cpu.py counts from the references."""
    from pyrodigal_amd import _cabi
    changed = 0
    for series in SERIES:
        for sh in shapes_of(series):
            idx = list(range(len(sh.seqs)))
            masked = call(ctx, sh, idx, _cabi.STAGE_EXTRACT)
            plain = ctx.nodes_stage(sh.seqs, _cabi.STAGE_EXTRACT)
            changed += any(a["n"] != b["n"] for a, b in zip(masked, plain))
    assert changed >= ms.MASKING_CHANGES_NODES, changed


def models():
    """The models of tests/test_region_masks_gpu.py."""
    m = [orc.Training.load(golden_path("SRR492066.training.bin.gz")),
         orc.Training.load(golden_path("GCF_001457455.1_NCTC11397_genomic_100kb.tinf_closed.bin.gz")),
         orc.Training.load(golden_path("GCF_001457455.1_NCTC11397_genomic.tinf_closed.bin.gz"))]
    for src, gc, tt in [(0, 0.36, 11), (1, 0.47, 11), (2, 0.42, 4), (0, 0.33, 4), (1, 0.64, 11)]:
        t = m[src].copy(); t.set_gc(gc); t.set_trans_table(tt); m.append(t)
    return m


def test_one_finder_call_over_the_joints_and_the_run_walk(ctx):
    """The joint and run-walk series as runs of N, one batch, every contig against the oracle; the same letters with n for N under
    lower-case masking alone (the builder, where the first call took the host-ordered path) give the same gene records."""
    mm = ms.JOINT_MIN_MASK
    seqs = [s for series in ("joint", "walk") for sh in shapes_of(series) if ms.pure_unknown(sh) and sh.min_mask == mm for s in sh.seqs]
    assert len(seqs) > 300 and ms.WALK_MIN_MASK == mm
    use = models()
    ctx.set_models([m.buf for m in use])
    res = ctx.find_genes_batch(seqs, meta=True, want_nodes=True, mask=True, min_mask=mm)
    genes = 0
    for i, s in enumerate(seqs):
        o = orc.Oracle(s, mask=True, mask_size=mm)
        genes += compare_contig(res, i, s, o, use, meta=True)
        assert res.masks[i].tolist() == o.masks().tolist()
    assert genes > 0
    soft = [s.replace(b"N", b"n") for s in seqs]
    low = ctx.find_genes_batch(soft, meta=True, want_nodes=True, mask=False, mask_lowercase=True, min_mask=mm)
    assert low.genes.tobytes() == res.genes.tobytes() and len(res.genes) > 0
    assert [m.tolist() for m in low.masks] == [m.tolist() for m in res.masks]


def test_the_densest_lists_are_complete(ctx):
    """`cap`, FindCall's bound on the list, end to end: a list one interval short of it comes back whole."""
    from pyrodigal_amd import _cabi
    tight = 0
    for sh in shapes_of("densest"):
        ref = reference(sh)
        n = sum(len(r) for r in ref)
        tight += ms.cap_of(sh) - n == 1
        for kw in ({}, harmless_source(sh, list(range(len(sh.seqs)))) if ms.pure_unknown(sh) else {}):
            got = call(ctx, sh, list(range(len(sh.seqs))), _cabi.STAGE_SEQUENCE, **kw).masks
            assert sum(len(m) for m in got) == n == ms.claim(sh, "n"), sh.name
            flat = [(k, tuple(iv)) for k, m in enumerate(got) for iv in m.tolist()]
            want = [(k, tuple(iv)) for k, r in enumerate(ref) for iv in r]
            assert flat[0] == want[0] and flat[-1] == want[-1], sh.name
    assert tight >= 1
