"""What tests/render_shapes.py contains, proven from the records and the host writers' text alone (no GPU): the populations
tests/test_render_shapes_gpu.py relies on; the host splice of flagged lines (_cabi._splice_fallback) on device-like texts; and
put_i64 and the closed forms of render_fmt.h (ORIGIN length and line starts, /translation bytes, record-body letters) through the
host shim, against a restatement of what the host writers write."""
import ctypes
import math
import os
import re
import subprocess
import textwrap
import types
from fractions import Fraction

import numpy as np
import pytest

from pyrodigal_amd import _cabi
from tests import render_shapes as rs

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "render_fmt_shim.cpp")
HDR = os.path.join(os.path.dirname(HERE), "pyrodigal_amd", "csrc", "render_fmt.h")
LIB = os.path.join(HERE, "librender_fmt_shim.so")


# ---- populations --------------------------------------------------------------------------------------------------------------------------

def gff_lines(case):
    return [ln for ln in rs.host_text(case, "gff")[1].decode().split("\n") if ln and not ln.startswith("#")]


def exact_halves(values, nd):
    """(rounded down, rounded up): the finite values that lie exactly on a rounding midpoint of '%.{nd}f', by what CPython prints."""
    down, up = [], []
    for v in values:
        if not math.isfinite(v):
            continue
        f = Fraction(v) * 10 ** nd
        if f.denominator == 2:
            printed = Fraction(("%%.%df" % nd) % v)
            (up if abs(printed) > abs(Fraction(v)) else down).append(v)
    return down, up


def test_number_populations():
    xs = rs.number_values()
    assert len(xs) > 20_000 and all(h in xs and -h in xs for h in rs.HALVES) and all(any(x == z and math.copysign(1, x) == math.copysign(1, z) for x in xs) for z in rs.SIGNED_ZEROS)
    # halves of every precision, in both directions: '%.2f' in the score fields, '%.1f' in the total, '%.3f' in gc_cont
    down, up = exact_halves(xs, 2)
    assert 0.125 in down and 0.375 in up and -0.375 in up and len(down) >= 3 and len(up) >= 3
    sums = [s + c for s, c in rs.SUM_PAIRS] + [x + 3.25 for x in xs]
    down, up = exact_halves(sums, 1)
    assert 0.25 in down and 0.75 in up and -0.75 in up
    down, up = exact_halves([float(x) for x in rs.gc_values()], 3)
    assert 0.0625 in down and 0.1875 in up and len(down) >= 4 and len(up) >= 4
    # what those print, in the host's text: signed zeros, halves, carries
    by_field = {c.name: gff_lines(c) for c in rs.number_cases()}
    for field in rs.SCORE_FIELDS[2:]:
        text = "\n".join(by_field["numbers_" + field])
        for want in ("-0.00", "0.12", "0.38", "-0.38", "10.00", "-10.00", "1.00", "100.00", "2.67", "2.68", "9007199254740991.00", "inf", "-inf", "nan"):
            assert ";%s=%s;" % (field, want) in text, (field, want)
    text = "\n".join(by_field["numbers_cscore"])
    assert ";score=-0.00;cscore=-3.25;" not in text and "\t-0.0\t" in "\n".join(by_field["numbers_sums"])
    sums_text = "\n".join(by_field["numbers_sums"])
    for want in ("\t0.3\t", "\t0.0\t", "\t-0.0\t", "\t0.2\t", "\t0.8\t", "\t-0.8\t", "\t10.0\t", "\t9.9\t", "\tinf\t", ";score=0.30;", ";score=-0.00;", ";score=0.00;"):
        assert want in sums_text, want
    assert 0.1 + 0.2 != 0.3                                   # the inexact sum
    gc = "\n".join(by_field["numbers_gc"])
    for want in ("gc_cont=0.062;", "gc_cont=0.188;", "gc_cont=0.000;", "gc_cont=1.000;", "gc_cont=1.500;", "gc_cont=inf;", "gc_cont=-inf;", "gc_cont=nan;", "gc_cont=0.500;"):
        assert want in gc, want
    # each value stands in each of the five fields, on both strands
    for field in rs.SCORE_FIELDS:
        case = rs.case_by_name("numbers_" + field)
        assert len(case.genes) == len(xs) and set(case.genes["strand"].tolist()) == {1, -1}
        col = case.genes[field]
        assert all((a == b) or (a != a and b != b) for a, b in zip(col.tolist(), xs))
    # the exact path's edges: 2^53 - 1 is printed, 2^53, the infinities and nan are flagged
    assert not rs.unprintable(2.0 ** 53 - 1) and all(rs.unprintable(x) for x in (2.0 ** 53, -2.0 ** 53, math.inf, -math.inf, math.nan))
    for case in rs.number_cases():
        flags = rs.expected_flags(case, "gff")
        assert 3 <= len(flags) <= 5, (case.name, flags)
        assert rs.expected_flags(case, "gff", margin=0.0) == flags          # none of these is flagged for a midpoint
        if "fna" in case.formats:
            assert rs.expected_flags(case, "fna") == rs.expected_flags(case, "faa") == flags and len(flags) == 4


def test_no_confidence_sits_at_the_margin():
    """A last-bit difference between the device's exp and the host's moves a confidence by about 1e-14: no case may hold one whose
    distance to a midpoint lies within 1e-11 of the margin, or its flag would depend on that bit.  (The confidence family keeps
    five and three orders away: test_confidence_populations.)"""
    for case in rs.all_cases():
        if "gff" not in case.formats:
            continue
        st_of = [rs.orc.Training(b).st_wt for b in case.blobs]
        for g in case.genes:
            score = float(g["cscore"]) + float(g["sscore"])
            if rs.unprintable(score):
                continue
            r, conf = rs.confidence(score, st_of[int(case.moc[int(g["contig"])])])
            if r < 41 and conf != 50.0:
                d = rs.midpoint_distance(conf) / 100
                assert abs(d - rs.MARGIN) > 1e-11, (case.name, score, conf, d)


def test_confidence_populations():
    st = rs.base_model().st_wt
    assert st == 4.35
    sc = rs.confidence_scores()
    assert sc["at_41"] / st == 41.0 and sc["below_41"] / st < 41 and math.nextafter(sc["at_41"], -math.inf) == sc["below_41"]
    case = rs.confidence_case()
    lines = gff_lines(case)
    names = [n for n in sc for _ in (1, -1)]
    assert len(lines) == len(names) and case.genes["strand"].tolist() == [1, -1] * len(sc)
    conf = {n: re.search(r";conf=([^;]+);", ln).group(1) for n, ln in zip(names, lines)}
    assert conf["below_41"] == "100.00" and conf["at_41"] == "99.99"
    assert conf["zero"] == conf["tiny"] == conf["huge_negative"] == conf["-inf"] == "50.00" and conf["inf"] == conf["nan"] == "99.99"
    assert rs.confidence(sc["tiny"], st)[1] == 50.0 and rs.confidence(sc["small"], st)[1] > 50.0
    flags = set(rs.expected_flags(case, "gff"))
    for mid in rs.MIDPOINTS:
        on, off = rs.confidence(sc["on_%s" % mid], st)[1], rs.confidence(sc["off_%s" % mid], st)[1]
        assert abs(on - mid) < 1e-12 and rs.midpoint_distance(on) / 100 < 1e-12
        assert all(abs(off - m) > 1e-6 for m in rs.MIDPOINTS) and rs.midpoint_distance(off) / 100 > 1e-6
        assert rs.midpoint_distance(on) < rs.MARGIN * 100 / 1e3 and rs.midpoint_distance(off) > rs.MARGIN * 100 * 1e3
    flagged = {names[k] for k in flags}
    assert flagged == {"on_%s" % m for m in rs.MIDPOINTS} | {"huge_negative", "inf", "-inf", "nan"}
    assert {names[k] for k in rs.expected_flags(case, "gff", margin=0.0)} == {"huge_negative", "inf", "-inf", "nan"}


def py_body_letters(g, protein, include_stop):
    n = int(g["end"]) - int(g["begin"]) + 1
    if not protein:
        return n
    stop_edge = g["partial_end"] if g["strand"] == 1 else g["partial_begin"]
    return max(n // 3 - (0 if stop_edge or include_stop else 1), 0)


def test_body_populations():
    seen_widths = set()
    for case in rs.body_cases():
        w = case.formats["faa"]["width"]
        assert case.formats["fna"]["width"] == w
        seen_widths.add(w)
        big = case.genes[case.genes["contig"] == 0]
        for strand in (1, -1):
            g = big[big["strand"] == strand]
            assert {(int(a), int(b)) for a, b in zip(g["partial_begin"], g["partial_end"])} == set(rs.PARTIALS)
            assert {int(e - b + 1) % 3 for b, e in zip(g["begin"], g["end"])} == {0, 1, 2}
            assert {1, 2, 3, 4, 5, 6} <= {int(e - b + 1) for b, e in zip(g["begin"], g["end"])}
            prot = {py_body_letters(x, 1, case.formats["faa"]["include_stop"]) for x in g}
            nuc = {py_body_letters(x, 0, 1) for x in g}
            want = set(rs.body_targets(w))
            assert want <= prot, (case.name, strand, sorted(want - prot))
            assert want - {0} <= nuc, (case.name, strand, sorted(want - nuc))
            if w <= 128:
                assert math.lcm(64, w) in want and {w - 1, w, w + 1, 2 * w} - {0} <= want | {0}
            assert any(b == 1 for b in g["begin"]) and any(e == rs.BODY_LEN for e in g["end"]) and any(b == 1 and e == rs.BODY_LEN for b, e in zip(g["begin"], g["end"]))
        assert max(rs.body_targets(w)) < 13_001
        # both models (tables 11 and 4) carry records
        assert set(case.genes["contig"].tolist()) == {0, 1} and rs.orc.Training(case.blobs[1]).trans_table == 4
    assert seen_widths == set(rs.BODY_WIDTHS) == {1, 2, 59, 60, 63, 64, 65, 70, 128, 13_001}
    opts = [c.formats["faa"] for c in rs.body_cases()]
    assert {o["include_stop"] for o in opts} == {True, False} and {o["strict_translation"] for o in opts} == {True, False}
    assert {o["translation_table"] for o in opts} == {None, 4, 11}


def unknown_positions(case, contig):
    """The codon positions (0, 1, 2) at which some codon of some gene of the contig holds its only unknown base, per strand."""
    seq = case.seqs[contig].upper()
    unk = np.frombuffer(bytes(0 if c in b"ACGT" else 1 for c in seq), np.uint8)
    out = {1: set(), -1: set()}
    for g in case.genes[case.genes["contig"] == contig]:
        b, e, strand = int(g["begin"]), int(g["end"]), int(g["strand"])
        for i in range((e - b + 1) // 3):
            p = [b - 1 + 3 * i + j for j in range(3)] if strand == 1 else [e - 1 - 3 * i - j for j in range(3)]
            u = [int(unk[q]) for q in p]
            if sum(u) == 1:
                out[strand].add(u.index(1))
    return out


def test_translation_populations():
    case = rs.body_cases()[0]
    pos = unknown_positions(case, 1)
    assert pos[1] == {0, 1, 2} and pos[-1] == {0, 1, 2}
    strict = {bool(c.formats["faa"]["strict_translation"]): rs.host_text(c, "faa")[1] for c in rs.body_cases()[:2]}
    assert b"X" in strict[True] and b"X" in strict[False]
    # internal stops, a forced M only on a whole first codon, and lower-case input
    text = rs.host_text(case, "faa")[1].decode()
    bodies = ["".join(r.split("\n")[1:]) for r in text.split(">")[1:]]
    assert any("*" in b[:-1] for b in bodies) and any(b.endswith("*") for b in bodies)
    heads = [r.split("\n")[0] for r in text.split(">")[1:]]
    starts = {(h.split(";partial=")[1][:2], b[:1] == "M") for h, b in zip(heads, bodies) if b}
    assert {p for p, _ in starts} == {"00", "10", "01", "11"}
    assert any(c.islower() for c in case.seqs[0].decode())


def test_gbk_populations():
    for case in rs.gbk_body_cases():
        for c in (0, 1):
            g = case.genes[case.genes["contig"] == c]
            for strand in (1, -1):
                chars = {15 + py_body_letters(x, 1, 0) for x in g[g["strand"] == strand]}
                assert {15, 58, 59, 60, 63, 64, 65, 118, 119} <= chars, (case.name, c, strand)
        text = rs.host_text(case, "gbk")[1].decode()
        assert '/translation=""\n' in text and "complement(<" in text and "..>" in text and "(<" in text
        pieces = {len(ln) - 21 for ln in text.split("\n") if ln.startswith(" " * 21) and not ln.startswith(" " * 21 + "/")}
        assert 1 in pieces and 59 in pieces          # a closing quote alone on its line, and whole pieces
    opts = [c.formats["gbk"] for c in rs.gbk_body_cases()]
    assert {o["strict_translation"] for o in opts} == {True, False} and {o["translation_table"] for o in opts} == {None, 4, 11}


def test_circular_populations():
    case = rs.circular_case()
    n = len(case.seqs[0])
    g = case.genes[case.genes["contig"] == 0]
    assert case.circular == [1, 0] and (case.genes["contig"] == 1).any()
    for strand in (1, -1):
        s = g[g["strand"] == strand]
        spans = {(int(b), int(e)) for b, e in zip(s["begin"], s["end"])}
        assert {(n, n + 1), (n, n + 2), (n, n + 3), (1, n), (2, n + 1), (n, 2 * n - 1)} <= spans
        assert max(e - b for b, e in spans) == n - 1
        # the codon that holds the origin: bases (n - 1, n, 1), (n, 1, 2), or none (the origin lies between two codons)
        phases = {(n - b + 1) % 3 for b, e in spans if e > n and e - b == 29} if strand == 1 else {(e - n) % 3 for b, e in spans if e > n and e - b == 29}
        assert phases == {0, 1, 2}
    text = rs.host_text(case, "gff")[0]
    assert b";topology=circular\n" in text[0] and b"topology" not in text[1]
    assert b"\tCDS\t%d\t%d\t" % (n, 2 * n - 1) in text[0]


def test_layout_populations():
    cases = {c.name: c for c in rs.layout_cases()}
    assert cases["layout_counts_030010"].contigs["n_genes"].tolist() == [0, 3, 0, 0, 1, 0]
    zero = cases["layout_counts_000000"]
    assert len(zero.genes) == 0 and rs.host_text(zero, "faa")[1] == b"" and rs.host_text(zero, "gff")[1].count(b"\n") == 18
    gff_units = {len(c.contigs) + len(c.genes) for n, c in cases.items() if n.startswith("layout_units")}
    gbk_units = {2 * len(c.contigs) + len(c.genes) for n, c in cases.items() if n.startswith("layout_units")}
    assert {255, 256, 257} <= gff_units and {255, 256, 257} <= gbk_units
    assert all(0 in c.contigs["n_genes"].tolist() for n, c in cases.items() if n.startswith("layout_units"))
    many = cases["layout_1001_genes"]
    assert b"ID=ctg1_1001;" in rs.host_text(many, "gff")[1] and b">ctg1_1001 # " in rs.host_text(many, "fna")[1]
    assert b"seqnum=999999999;" in rs.host_text(cases["layout_first_seqnum"], "gff")[1]
    assert b"ID=1000000002_3;" in rs.host_text(cases["layout_first_seqnum"], "faa")[1]
    text = rs.host_text(cases["layout_seqnums"], "gff")[1]
    assert all(b"seqnum=%d;" % s in text and b"ID=%d_1;" % s in text for s in (0, 7, 2 ** 40, -3))
    ids = cases["layout_ids_full"].ids
    assert ids[0] == "" and sorted({(len(i), len(i.encode()) > len(i)) for i in ids[1:]}) == [(22, False), (22, True), (23, False), (23, True), (24, False), (24, True)]
    assert {max(len(ch.encode()) for ch in i) for i in ids[1:]} == {1, 2, 3, 4}
    locus = [ln for ln in rs.host_text(cases["layout_ids_full"], "gbk")[1].decode().split("\n") if ln.startswith("LOCUS")]
    assert len(locus) == 13 and {len(ln.split(" bp ")[0]) for ln in locus} == {12 + 23 + 1 + 3, 12 + 24 + 1 + 3}          # in code points
    text = rs.host_text(cases["layout_gff_options"], "gff")[1]
    assert b"##gff-version" not in text and b";transl_table=11;conf=" in text and b"\tpyrodigal_amd-" in text
    assert b";transl_table=4;conf=" in rs.host_text(cases["layout_gff_tt"], "gff")[1]
    pos = cases["layout_positions"]
    assert set(pos.formats) == {"gff", "fna"} and len(pos.seqs[0]) == 100_001
    assert {len(str(int(x))) for x in pos.genes["end"]} == {1, 2, 3, 4, 5, 6} and {len(str(int(x))) for x in pos.genes["begin"]} == {1, 2, 3, 4, 5, 6}


def test_origin_populations():
    case = rs.origin_case()
    assert tuple(len(s) for s in case.seqs) == rs.ORIGIN_LENGTHS == (1, 9, 10, 11, 59, 60, 61, 119, 120, 121, 20_479, 20_480, 20_481, 40_960, 40_961)
    assert len(case.genes) == 0
    tails = [s[10 * ((len(s) - 1) // 10):] for s in case.seqs]
    assert all(t == b"N" * len(t) for t in tails[0::3]) and all(t.islower() for t in tails[1::3])
    assert all(not set(t) & set(b"ACGTacgtNn") for t in tails[2::3])
    for n, text in zip(rs.ORIGIN_LENGTHS, rs.host_text(case, "gbk")[0]):
        body = text.split(b"ORIGIN\n")[1]
        assert body.count(b"\n") == (n + 59) // 60 + 1 and body.endswith(b"//\n") and not set(body) - set(b"acgtn 0123456789/\n")


def test_rbs_populations():
    models = rs.rbs_models()
    assert [t.uses_sd for t in models] == [1, 1, 0, 0, 0, 0, 0] and [t.no_mot for t in models[2:6]] == [-0.4, -0.5, -0.6, math.nextafter(-0.5, 0.0)]
    assert -0.5 < models[5].no_mot and models[6].st_wt < 0
    single, meta = rs.rbs_cases()
    assert meta.meta and len(meta.descriptions) == len(models) and single.genes.tobytes() == meta.genes.tobytes()
    seen = {}
    for g in single.genes:
        t = models[int(g["contig"])]
        k0, k1 = int(g["rbs"][0]), int(g["rbs"][1])
        branch, site = rs.rbs_site(t, k0, k1, float(g["mot_score"]))
        st = t.st_wt
        r1, r2, ms = float(t.rbs_wt[k0]) * st, float(t.rbs_wt[k1]) * st, float(g["mot_score"]) * st
        marks = {branch}
        if not t.uses_sd and t.no_mot > -0.5:
            marks |= {m for m, hit in (("r1==r2", r1 == r2 and k0 != k1), ("ms==r1>r2", ms == r1 and r1 > r2), ("ms==r2>=r1", ms == r2 and r2 >= r1),
                                       ("ms just below r1", r1 > r2 and ms < r1 and float(g["mot_score"]) == rs.beside(float(t.rbs_wt[k0]), st, st < 0)),
                                       ("ms just above r1", r1 > r2 and ms > r1 and float(g["mot_score"]) == rs.beside(float(t.rbs_wt[k0]), st, st > 0))) if hit}
        if t.uses_sd and r1 == r2 and k0 != k1:
            marks.add("sd r1==r2")
        if branch == "motif":
            marks.add("motif none" if g["mot_len"] == 0 else "motif %d" % g["mot_len"])
            if not t.no_mot > -0.5:
                marks.add("no_mot %s" % t.no_mot)
        for m in marks:
            seen.setdefault(m, set()).add(int(g["strand"]))
    want = ["sd_first", "sd_second", "first", "second", "motif", "r1==r2", "ms==r1>r2", "ms==r2>=r1", "ms just below r1", "ms just above r1", "sd r1==r2",
            "motif none", "motif 3", "motif 4", "motif 5", "motif 6", "motif 16", "motif 17", "no_mot -0.5", "no_mot -0.6"]
    for m in want:
        assert seen.get(m) == {1, -1}, (m, seen.get(m))
    for c in range(len(models)):
        g = single.genes[single.genes["contig"] == c]
        assert set(g["rbs"][:, 0].tolist()) == set(range(28)) == set(g["rbs"][:, 1].tolist())
        assert set(g["start_type"].tolist()) == {0, 1, 2, 3} and {0, 255} <= set(g["mot_spacer"].tolist())
        assert (g["mot_ndx"] < 0).any() and (g["mot_ndx"] > 0).any()
    text = rs.host_text(single, "gff")[1]
    for want in (b"rbs_motif=None;rbs_spacer=None;", b"rbs_spacer=255bp;", b"rbs_spacer=0bp;", b"rbs_motif=AGGAGG;rbs_spacer=5-10bp;", b"start_type=Edge;",
                 b"rbs_motif=" + b"T" * 17 + b";", b"rbs_motif=CTTTTTTTTTTTTTTTT;", b"rbs_motif=TTTTTTTTTTTTTTTG;"):
        assert want in text, want
    assert b'run_type=Metagenomic;model="Caf\xc3\xa9 7";' in rs.host_text(meta, "gff")[1] and b'run_type=Single;model="Ab initio";' in text


def test_flag_populations():
    for case in rs.flag_cases():
        for fmt in case.formats:
            flags = rs.expected_flags(case, fmt)
            assert len(flags) == 9
            contig = case.genes["contig"][flags].tolist()
            begin, count = case.contigs["gene_begin"], case.contigs["n_genes"]
            first = [k for k in flags if k == begin[case.genes["contig"][k]]]
            last = [k for k in flags if k == begin[case.genes["contig"][k]] + count[case.genes["contig"][k]] - 1]
            assert first and last and any(k in first and k in last for k in flags)
            assert any(k + 1 in flags and k + 2 in flags for k in flags)                   # three in a row
            assert count.tolist()[2] == 0 and count.tolist()[4:6] == [0, 0] and count[-1] == 0
            assert {3, 6} <= set(contig)                                                    # after one, and after two, contigs without genes
    # the host's text of a flagged unit against the device's guess ("0.00" / "0.000" for the value)
    longer = rs.host_text(rs.case_by_name("flags_gff_longer"), "gff")[1]
    assert re.search(rb"=\d{301}\.00;", longer) and re.search(rb"=-\d{301}\.00;", longer) and b"=9007199254740992.00;" in longer
    shorter = rs.host_text(rs.case_by_name("flags_gff_shorter"), "gff")[1]
    assert b"=inf;" in shorter and b"=nan;" in shorter and len("inf") < len("0.00")
    for fmt in ("faa", "fna"):
        assert b"gc_cont=inf\n" in rs.host_text(rs.case_by_name("flags_gc_shorter"), fmt)[1]
        assert b"gc_cont=-inf\n" in rs.host_text(rs.case_by_name("flags_gc_shorter"), fmt)[1]
        assert re.search(rb"gc_cont=-?3\d{38}\.000\n", rs.host_text(rs.case_by_name("flags_gc_longer"), fmt)[1])


def test_scores_populations():
    """From the oracle's nodes of the contigs of the scores family.  Two populations are asserted absent (the only two of this file):
    1. a row group with stop_val < 0 or stop_val >= seqlen.  With open ends the node extraction pulls the stop value of an ORF that
       runs off the contig back inside it, three bases at a time (oracle/prodigal_oracle.c sweep_strand: while last + 3 > slen:
       last -= 3), and with closed ends it drops the starts of such an ORF: the stop values of start nodes lie in [2, seqlen - 3],
       and only stop nodes, which have no row, carry values outside.  The nearest the family gets are the groups at those two ends.
    2. a stop value shared by start nodes of both strands.  A forward stop codon at index p (stop_val = p) needs T at p, a reverse one
       that ends at p (stop_val = p) needs A there: the 'strand descending' part of the row order never decides between two rows
       that real stop codons made.  (Neither occurs in any contig of tests/start_shapes.py, with open or closed ends.)"""
    seqs, ids = rs.scores_contigs()
    t = rs.base_model()
    seen = set()
    counts = []
    for seq in seqs:
        o = rs.orc.Oracle(seq)
        o.find_genes_single(t)
        nd = o.nodes()
        counts.append(len(nd))
        st = nd[nd["type"] != 3]
        for strand in (1, -1):
            s = st[st["strand"] == strand]
            assert not (s["stop_val"] < 2).any() and not (s["stop_val"] > len(seq) - 3).any()          # absent population 1
            seen |= {("first stop value", strand)} if (s["stop_val"] <= 4).any() else set()
            seen |= {("last stop value", strand)} if (s["stop_val"] >= len(seq) - 5).any() else set()
            seen |= {("edge", strand)} if (s["edge"] != 0).any() else set()
            seen |= {("group of several rows", strand)} if len(s) > len(set(s["stop_val"].tolist())) else set()
        shared = set(st["stop_val"][st["strand"] == 1].tolist()) & set(st["stop_val"][st["strand"] == -1].tolist())
        assert not shared                                                                                  # absent population 2
    assert counts[0] == 0 and counts[-1] == 0 and all(counts[1:-1])
    # (a forward ORF that runs off the contig has the last stop value, a reverse one the first)
    assert seen == {("first stop value", -1), ("last stop value", 1), ("edge", 1), ("edge", -1), ("group of several rows", 1), ("group of several rows", -1)}
    # the restated writer on the oracle's nodes: headers, one blank line per group and one at the end, Edge rows
    o = rs.orc.Oracle(seqs[1])
    o.find_genes_single(t)
    text = rs.scores_text(o.nodes(), t, 2, len(seqs[1]), ids[1], True)
    assert text.startswith('# Sequence Data: seqnum=2;seqlen=%d;seqhdr="sc1"\n# Run Data: version=pyrodigal_amd.v' % len(seqs[1]))
    assert "\tEdge\t" in text and text.endswith("\n\n") and "\n\n\n" not in text
    assert rs.scores_text(rs.orc.Oracle(seqs[0]).nodes(), t, 1, 4, "sc0", False) == "\n"


# ---- the host splice ----------------------------------------------------------------------------------------------------------------------

def units_of(case, fmt, c):
    """The text of contig c cut into (gene index or None, bytes that a flag replaces, bytes that stay)."""
    text = rs.host_text(case, fmt)[0][c]
    lo = int(case.contigs["gene_begin"][c])
    if fmt == "gff":
        lines = text.split(b"\n")[:-1]
        head = [ln for ln in lines if ln.startswith(b"#")]
        body = [ln for ln in lines if not ln.startswith(b"#")]
        assert lines == head + body and len(body) == int(case.contigs["n_genes"][c])
        return [(None, b"", b"".join(ln + b"\n" for ln in head))] + [(lo + k, ln + b"\n", b"") for k, ln in enumerate(body)]
    recs = re.split(rb"(?m)^(?=>)", text)[1:] if text else []
    assert len(recs) == int(case.contigs["n_genes"][c])
    return [(lo + k, r[:r.index(b"\n") + 1], r[r.index(b"\n") + 1:]) for k, r in enumerate(recs)]


def device_like(case, fmt, flags, deltas):
    """A text in which every flagged unit holds a placeholder of another length: (data, contig offsets, fallback rows)."""
    data, coff, fb, n = [], [0], [], 0
    flags = set(flags)
    at = 0
    for c in range(len(case.seqs)):
        for k, replaced, kept in units_of(case, fmt, c):
            if k in flags:
                d = deltas[n % len(deltas)]
                n += 1
                guess = b"?" * max(1, len(replaced) + d)
                fb.append((k, at, at + len(guess)))
                data.append(guess)
                at += len(guess)
            else:
                data.append(replaced)
                at += len(replaced)
            data.append(kept)
            at += len(kept)
        coff.append(at)
    return b"".join(data), np.array(coff, np.int64), np.array(fb, np.int64).reshape(-1, 3)


SPLICE_CASES = [(c.name, f) for c in rs.flag_cases() + (rs.confidence_case(), rs.number_cases()[-1], rs.number_cases()[-2]) for f in c.formats]


@pytest.mark.parametrize("name,fmt", SPLICE_CASES)
@pytest.mark.parametrize("deltas", [(0,), (-3, 5), (300, -1, 0, 2), (-10_000,)])
def test_splice_fallback(name, fmt, deltas):
    case = rs.case_by_name(name)
    flags = rs.expected_flags(case, fmt)
    assert flags
    data, coff, fb = device_like(case, fmt, flags, deltas)
    ctx = types.SimpleNamespace(_models=[np.frombuffer(b, np.uint8) for b in case.blobs])
    opts = dict(_cabi._WRITER_DEFAULTS[fmt]); opts.update(case.formats[fmt])
    got, off = _cabi._splice_fallback(ctx, fmt, opts, data, coff, fb, case.genes, case.contigs, case.moc, case.ids, case.first_seqnum, case.seqnums)
    per_contig, want = rs.host_text(case, fmt)
    assert got == want
    assert off.tolist() == np.concatenate([[0], np.cumsum([len(t) for t in per_contig])]).tolist()


# ---- the shim: put_i64 and the closed forms -----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def shim():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", LIB, SRC], check=True)
    L = ctypes.CDLL(LIB)
    L.render_put_i64.restype = ctypes.c_int64
    L.render_put_i64.argtypes = [ctypes.c_int64, ctypes.c_char_p]
    for name in ("render_origin_len", "render_origin_line_at", "render_gbk_tr_bytes"):
        getattr(L, name).restype = ctypes.c_int64
        getattr(L, name).argtypes = [ctypes.c_int64]
    L.render_body_letters.restype = ctypes.c_int64
    L.render_body_letters.argtypes = [ctypes.c_int64, ctypes.c_int64] + [ctypes.c_int] * 5
    return L


def test_put_i64(shim):
    vals = [0, -(2 ** 63), 2 ** 63 - 1]
    for k in range(1, 19):
        vals += [10 ** k - 1, -(10 ** k - 1), 10 ** k, -(10 ** k)]
    buf = ctypes.create_string_buffer(24)
    for v in vals:
        n = shim.render_put_i64(v, buf)
        assert buf.raw[:n] == b"%d" % v, v


def origin_text(n):
    """ORIGIN as write_genbank writes it, for n bases."""
    seq = "a" * n
    out = ["ORIGIN\n"]
    for i in range(0, n, 60):
        out.append("{:>9}".format(i + 1))
        for j in range(i, min(i + 60, n), 10):
            out.append(" " + seq[j:j + 10])
        out.append("\n")
    out.append("//\n")
    return "".join(out)


def origin_line_len(k, n):
    """Bytes of ORIGIN line k of n bases: the position in at least nine columns, the bases, a space per ten-base block, a newline."""
    bases = min(60, n - 60 * k)
    return max(9, len(str(60 * k + 1))) + bases + (bases + 9) // 10 + 1


def first_line_with_digits(d):
    """The first ORIGIN line whose position 60 k + 1 has d digits, found on the printed length."""
    lo, hi = 0, 10 ** d
    while lo < hi:
        mid = (lo + hi) // 2
        if len(str(60 * mid + 1)) >= d:
            hi = mid
        else:
            lo = mid + 1
    return lo


def test_origin_closed_forms_small(shim):
    for n in list(range(1, 201)) + list(range(20_400, 20_560)) + [40_959, 40_960, 40_961]:
        text = origin_text(n)
        assert shim.render_origin_len(n) == len(text), n
        at = 7
        for k in range((n + 59) // 60):
            assert shim.render_origin_line_at(k) == at, (n, k)
            assert text[at - 1] == "\n" and text[at:at + 9].strip() == str(60 * k + 1)
            at += origin_line_len(k, n)
        assert at + 3 == len(text)
    assert shim.render_origin_len(0) == len(origin_text(0)) == 10


def test_origin_closed_forms_at_ten_digits(shim):
    """The first ORIGIN line whose position has ten digits is line 16 666 667 (position 1 000 000 021): from there a line is a byte
    longer.  No GPU test renders a contig of 10^9 bases, so this branch is tested here alone."""
    k10 = first_line_with_digits(10)
    assert k10 == 16_666_667 and 60 * k10 + 1 == 1_000_000_021 and len(str(60 * (k10 - 1) + 1)) == 9
    for k in (0, 1, k10 - 1, k10, k10 + 1, k10 + 2, (2 ** 31 - 2) // 60):
        assert shim.render_origin_line_at(k) == 7 + 76 * k + max(0, k - k10), k          # 76 = 9 + 60 + 6 + 1 of every full line before it
    for n in (999_999_960, 1_000_000_019, 1_000_000_020, 1_000_000_021, 1_000_000_080, 1_000_000_081, 1_000_000_082, 2 ** 31 - 1):
        lines = (n + 59) // 60
        full = lines - 1                                             # full lines, 76 bytes each and one more from line k10 on
        want = 7 + 76 * full + max(0, full - k10) + origin_line_len(full, n) + 3
        assert shim.render_origin_len(n) == want, n
        # the line starts around the first ten-digit line, summed from the lengths of the lines before
        at = 7 + 76 * (k10 - 2)
        for k in range(k10 - 2, min(lines, k10 + 4)):
            assert shim.render_origin_line_at(k) == at, (n, k)
            at += origin_line_len(k, n)
        if lines <= k10 + 4:
            assert shim.render_origin_len(n) == at + 3, n
    assert shim.render_origin_len(1_000_000_020) - shim.render_origin_len(1_000_000_019) == 1
    assert shim.render_origin_len(1_000_000_021) - shim.render_origin_len(1_000_000_020) == 10 + 1 + 1 + 1     # a ten-digit position, a space, a base, a newline
    assert shim.render_origin_len(1_000_000_081) - shim.render_origin_len(1_000_000_080) == 10 + 1 + 1 + 1


def test_translation_bytes(shim):
    for L in range(15, 201):
        tr = '/translation="%s"' % ("M" * (L - 15))
        want = sum(21 + len(block) + 1 for block in textwrap.wrap(tr, 59))
        assert shim.render_gbk_tr_bytes(L) == want, L
    assert [shim.render_gbk_tr_bytes(L) - L for L in (15, 58, 59, 60, 118, 119)] == [22, 22, 22, 44, 44, 66]


def test_body_letters(shim):
    for begin in (1, 2, 700):
        for n in range(1, 70):
            for strand in (1, -1):
                for pb, pe in rs.PARTIALS:
                    for protein in (0, 1):
                        for include_stop in (0, 1):
                            g = {"begin": begin, "end": begin + n - 1, "strand": strand, "partial_begin": pb, "partial_end": pe}
                            assert shim.render_body_letters(begin, begin + n - 1, strand, pb, pe, protein, include_stop) == py_body_letters(g, protein, include_stop)
