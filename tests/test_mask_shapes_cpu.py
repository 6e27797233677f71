"""The catalogue of tests/mask_shapes.py without a GPU: the numpy reference against the oracle's own masking rule
wherever the only source is runs of unknown bases; the builder's bit logic restated against the reference on every shape; the events
the whole catalogue never produces, which must be exactly mask_shapes.IMPOSSIBLE; and every shape against what its design claims."""
from collections import Counter

import pytest

from oracle import oracle as orc
from tests import mask_shapes as ms
from tests.extract_ref import extract_ref

@pytest.fixture(scope="module")
def shapes():
    return ms.catalogue()


@pytest.fixture(scope="module")
def restated(shapes):
    """(reference, restated lists, events) per shape, the scan rounds included; computed once."""
    out = {}
    for sh in shapes:
        out[sh.name] = (ms.reference(sh),) + ms.restate(sh)
    for n in ms.SCAN_GROUPS:
        for sh in ms.scan_shapes(n):
            assert ms.groups_of(sh.seqs) == n
            ref = ms.reference(sh)
            assert ms.measure(sh, ref)["g"] == sh.claims["g"] and ms.claim(sh, "n") == len(sh.claims["g"])
            out[sh.name] = (ref,) + ms.restate(sh)
    return out


def test_names_are_unique_and_every_series_is_there(shapes):
    names = [sh.name for sh in shapes]
    assert len(set(names)) == len(names)
    assert {n.split("/")[0] for n in names} == {"bit", "lanes", "group", "joint", "short", "walk", "byte", "together", "densest"}
    for sh in shapes:
        assert sh.regions is None or len(sh.regions) == len(sh.seqs)
        assert sh.mask or sh.lower or sh.regions is not None, sh.name


def test_the_reference_is_the_oracles_rule_for_unknown_runs(shapes):
    n = 0
    for sh in shapes:
        if not ms.pure_unknown(sh):
            continue
        for s, want in zip(sh.seqs, ms.reference(sh)):
            assert orc.Oracle(s, mask=True, mask_size=sh.min_mask).masks().tolist() == want.tolist(), (sh.name, len(s))
            n += len(want)
    assert n > 3000


def test_the_restated_builder_is_the_reference(restated):
    for name, (ref, lists, _) in restated.items():
        assert [a.tolist() for a in lists] == [a.tolist() for a in ref], name


def test_events_never_produced_are_exactly_the_impossible_ones(restated):
    total = Counter()
    for _, _, ev in restated.values():
        total.update(ev)
    missing = {k for k in ms.EVENTS if total[k] == 0}
    assert missing == set(ms.IMPOSSIBLE), (sorted(missing - set(ms.IMPOSSIBLE), key=str), sorted(set(ms.IMPOSSIBLE) - missing, key=str))
    print({k: total[k] for k in ms.EVENTS})


def test_every_shape_holds_what_it_claims(shapes):
    for sh in shapes:
        got = ms.measure(sh)
        for key in ("n", "len", "bits", "words", "g"):
            want = ms.claim(sh, key)
            if want is not None:
                assert got[key] == want, (sh.name, key)
        assert got["base"][0] == 0
        assert sh.claims or sh.name.startswith("byte/")
    by = {sh.name: ms.measure(sh) for sh in shapes}
    # the residues the issue names, from the reference's intervals alone
    bits = [b for name, m in by.items() if name.startswith("bit/") for b in m["bits"]]
    assert {b[0] for b in bits} == {0, 1, 31} and {b[1] for b in bits} >= {0, 30, 31}
    assert {w for name, m in by.items() if name.startswith("lanes/") for w in m["words"]} == set(ms.LANE_WORDS)
    # every filler puts the first designed contig off a word boundary or where its design says
    assert all(len(sh.seqs[0]) > ms.GROUP or sh.name.startswith(("densest/", "joint/", "short/", "group/")) for sh in shapes)
    # the densest lists sit one below the bound where they are alone in their batch
    assert any(ms.cap_of(sh) - by[sh.name]["n"] == 1 for sh in shapes if sh.name.startswith("densest/alternating/alone"))
    assert all(by[sh.name]["n"] <= ms.cap_of(sh) for sh in shapes)


def test_joints_and_short_contigs_are_where_the_design_says(shapes):
    for sh in shapes:
        base = ms.bases_of(sh.seqs)
        if sh.name.startswith("joint/m"):
            e = sh.claims["empties"]
            joints = [j for _, j in ms.JOINTS]
            assert [j % 32 for j in joints] == [0, 1, 13, 0] and joints[3] % ms.GROUP == 0
            for j in joints:
                assert int((base[:-1] == j).sum()) == e + 1, (sh.name, j)
            assert (len(sh.seqs[0]) == 0) == (e > 0) and (len(sh.seqs[-1]) == 0) == (e > 0)
        if sh.name.startswith("short/") and "total" not in sh.name:
            assert len(sh.seqs) == 260 and all(len(sh.seqs[k]) in (1, 2) for k in (255, 256, 257))
        if sh.name.startswith("short/total"):
            assert len(sh.seqs) in (255, 256) and len(sh.seqs[-1]) == 2


def test_masking_changes_the_nodes_of_enough_shapes(shapes):
    """The extraction-stage comparison of the GPU module is not vacuous: the reference's nodes under the masks differ in number from
    the nodes without them (pure unknown-run shapes by the oracle, the others by tests/extract_ref.py)."""
    changed = 0
    for sh in shapes:
        ref = ms.reference(sh)
        diff = False
        for s, r in zip(sh.seqs, ref):
            if diff or not len(r) or len(s) > 4000:
                continue
            if ms.pure_unknown(sh):
                a, b = orc.Oracle(s, mask=True, mask_size=sh.min_mask), orc.Oracle(s)
                for o in (a, b):
                    o.extract(11, orc.Params())
                diff = len(a.nodes()) != len(b.nodes())
            else:
                diff = len(extract_ref(s, r.tolist())[0]) != len(extract_ref(s, ())[0])
        changed += diff
    print("shapes whose node count masking changes:", changed)
    assert changed >= ms.MASKING_CHANGES_NODES
