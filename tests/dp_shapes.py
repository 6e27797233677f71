"""Contigs and score arrays that put connection scoring -- dp.hip, dp_wave.hip, dpw_core.h and k_ovl_stops, which builds star_ptr for
it -- at its distance, overlap and window edges: the inputs of tests/test_dp_shapes_cpu.py and tests/test_dp_shapes_gpu.py (DESIGN.md
4.4.1, "Connection scoring at its edges").  A helper module, not a test.

Everything is designed, nothing drawn.  A contig is the quiet background of tests/extract_shapes.py with single codons written over it
(`Layout`): a forward gene is an ATG at x and a TAA at y, a reverse gene a TTA at x and a CAT at y (nodes at x + 2 and y + 2), so a
design is written once and built on either strand IN PLACE -- the same distances between the same roles (gene begin, gene end), which
is what the rules compare; the mirror image of the whole contig (`mirrored`) reverses the order of the nodes and so who is source and
who is target, and is run for the values alone.  Each shape carries a designed score assignment: cscore / sscore / rscore / uscore of
the nodes it names, DEFAULT for every other node (a start costs 50, so no path runs through a gene the design does not name), and
the probe: the pair of nodes whose connection the rule under test allows or refuses.  The scores are chosen so that the probe pair
decides the result: where the rule allows the connection the probe source is the target's traceb, where it refuses it is not.

Shapes come as neighbours: the same design at threshold - 1, at the threshold and at threshold + 1.  A distance at which no codon can
stand is listed in IMPOSSIBLE with the reason, not dropped."""
from collections import namedtuple

from tests.extract_shapes import quiet, revcomp

ST_WT = 4.35
IG = 0.15 * ST_WT                              # the unit of the intergenic term (ref: _connection.h:52-78)
DEFAULT = {"start": dict(cscore=-50.0, sscore=0.0, rscore=0.0, uscore=0.0), "stop": dict(cscore=0.0, sscore=0.0, rscore=0.0, uscore=0.0)}

# a designed node: kind "fb" forward start, "fs" forward stop, "rb" reverse start, "rs" reverse stop; position; stop_val
Node = namedtuple("Node", "kind ndx stop_val")
# name; letters; closed ends; {name: Node} of the designed nodes; total node count; {name: scores}; probe (source, target, allowed) or
# None; series and the neighbour's value within it; claims read by the CPU test; max_overlap for star_ptr
Shape = namedtuple("Shape", "name seq closed nodes n_nodes scores probe series at meta max_overlap")

KIND = {"fb": (1, False), "fs": (1, True), "rb": (-1, False), "rs": (-1, True)}


def kind_of(strand, is_stop):
    return ("f" if strand == 1 else "r") + ("s" if is_stop else "b")


class Layout:
    """A contig of background bases (at least L, it grows with what is written) with single codons written over it.  gene(x, y,
    strand): a forward gene has its start codon at x and its stop codon at y, a reverse gene its stop codon at x and its start codon
    at y; both give the nodes `name + "b"` (start) and `name + "s"` (stop).  Letters next to a codon that would read as a further codon
    are replaced (`guards`) unless another codon stands there."""

    def __init__(self, L, closed=True):
        self.L, self.closed = L, closed
        self.planted = {}                          # position -> letter
        self.guards = {}
        self.nodes = {}
        self.count = 0
        self.implicit = []                         # (kind, ndx) of stop codons that a run of start codons reads in the next frame

    def put(self, at, text, before=None, after=None):
        self.L = max(self.L, at + len(text) + 40)          # the contig grows with what is written
        for k, ch in enumerate(text):
            assert self.planted.get(at + k, ch) == ch, ("two codons disagree at", at + k)
            self.planted[at + k] = ch
        if before:
            self.guards.setdefault(at - 1, before)
        if after:
            self.guards.setdefault(at + len(text), after)

    def start(self, name, at, strand, stop_val, count=True, codon=None):
        """One start codon of the ORF that ends at stop_val (a node position)."""
        if strand == 1:
            self.put(at, codon or "ATG", before="G")        # C before ATG would read CAT
            self.nodes[name] = Node("fb", at, stop_val)
        else:
            self.put(at, codon or "CAT", after="C")         # G after CAT would read ATG
            self.nodes[name] = Node("rb", at + 2, stop_val)
        self.count += count

    def stop(self, name, at, strand, codon=None):
        """A stop codon; its node's stop_val -- the stop codon that ends the ORF on its far side -- is found in `finish`."""
        if strand == 1:
            self.put(at, codon or "TAA", before="G")      # C before TAA would read CTA
            self.nodes[name] = Node("fs", at, None)
        else:
            self.put(at, codon or "TTA", after="C")       # G after TTA would read TAG
            self.nodes[name] = Node("rs", at + 2, None)
        self.count += 1

    def gene(self, name, x, y, strand, stop_codon=None, start_codon=None):
        assert (y - x) % 3 == 0 and y - x >= 87, (name, x, y)
        if strand == 1:
            self.start(name + "b", x, 1, y, codon=start_codon)
            self.stop(name + "s", y, 1, stop_codon)
        else:
            self.stop(name + "s", x, -1, stop_codon)
            self.start(name + "b", y, -1, x + 2, codon=start_codon)

    def run(self, name, at, k, strand):
        """Cheap filler: k start codons of one ORF, one every three bases, and its stop codon 90 bases from the nearest of them: k + 1
        nodes, `name + "s"` and `name + "0"` .. (in ascending position).  Returns the first position behind it.  (A run of ATG reads
        TGA in the next frame, a run of CAT reads TCA: an ORF of that frame may not cross it.)"""
        if strand == 1:
            stop_at = at + 3 * (k - 1) + 90
            for j in range(k):
                self.start("%s%d" % (name, j), at + 3 * j, 1, stop_at)
            self.implicit += [("fs", at + 3 * j + 1) for j in range(k - 1)]
            self.stop(name + "s", stop_at, 1)
            return stop_at + 3
        self.stop(name + "s", at, -1)
        for j in range(k):
            self.start("%s%d" % (name, j), at + 90 + 3 * j, -1, at + 2)
        self.implicit += [("rs", at + 90 + 3 * j + 4) for j in range(k - 1)]
        return at + 90 + 3 * k

    def finish(self):
        """stop_val of the stop nodes of a closed contig: the nearest stop of the strand and frame on the ORF's far side, or what the
        extraction leaves where the frame holds none (ref: lib.pyx:2007-2018 / 2102-2113: frame - 6, L - frame + 5)."""
        for name, n in self.nodes.items():
            if n.stop_val is not None:
                continue
            same = [m.ndx for m in self.nodes.values() if m.kind == n.kind and m.ndx % 3 == n.ndx % 3]
            same += [v for k, v in self.implicit if k == n.kind and v % 3 == n.ndx % 3]
            if n.kind == "fs":
                far = [v for v in same if v < n.ndx]
                self.nodes[name] = n._replace(stop_val=max(far) if far else n.ndx % 3 - 6)
            else:
                far = [v for v in same if v > n.ndx]
                self.nodes[name] = n._replace(stop_val=min(far) if far else self.L - (self.L - 1 - n.ndx) % 3 + 5)
        return dict(self.nodes)

    def extra_start(self, name, at, gene_stop_node, strand):
        """A further start codon of the ORF whose stop node is `gene_stop_node` (same frame)."""
        self.start(name, at, strand, self.nodes[gene_stop_node].ndx)

    def seq(self):
        s = bytearray(quiet(self.L))
        for at, ch in self.guards.items():
            if at not in self.planted and 0 <= at < self.L:
                s[at] = ord(ch)
        for at, ch in self.planted.items():
            s[at] = ord(ch)
        return bytes(s)


def shape(name, lay, scores, probe, series, at, meta=None, max_overlap=60):
    return Shape(name, lay.seq(), lay.closed, lay.finish(), lay.count, scores, probe, series, at, meta or {}, max_overlap)


def mirrored(sh):
    """The reverse complement of the whole contig: node k of the design is node n - 1 - k of it (position L - 1 - ndx, the other strand,
    stop_val mirrored likewise), so the injector writes the same scores in reverse order.  No probe: source and target swap roles."""
    L = len(sh.seq)
    flip = {"fb": "rb", "fs": "rs", "rb": "fb", "rs": "fs"}
    nodes = {k: Node(flip[v.kind], L - 1 - v.ndx, L - 1 - v.stop_val) for k, v in sh.nodes.items()}
    return sh._replace(name=sh.name + "/mirror", seq=revcomp(sh.seq), nodes=nodes, probe=None, series=None)


# (comparison of the oracle's edge counters, lhs - rhs) that no input can reach, each with its reason: what the CPU test accepts as
# missing from the counters, and nothing else.  "letters" stands for: the two codons would have to share one or two positions, and no
# stop codon (TAA TAG TGA; on the reverse strand, as written, TTA CTA TCA) and start codon (ATG GTG TTG; CAT CAC CAA) agree there.
IMPOSSIBLE = {
    ("fs_fb", 1): "letters: a start one base behind a forward stop's first base",
    ("rb_rs", 1): "letters: a reverse stop that ends one base behind a reverse start's last base",
    ("fs_rs", 0): "letters: a reverse stop whose first base is the forward stop's last",
    ("fs_rs", 1): "letters: a reverse stop over the forward stop's last two bases",
    ("fb_fs", -1): "a gene's start and the stop before its ORF share the frame: the difference is a multiple of 3, and not 0",
    ("fb_fs", 0): "see fb_fs -1", ("fb_fs", 1): "see fb_fs -1",
    ("rs_rb", -1): "see fb_fs -1", ("rs_rb", 0): "see fb_fs -1", ("rs_rb", 1): "see fb_fs -1",
    ("fs_fs", -1): "letters: two forward stops one base apart", ("fs_fs", 1): "letters: two forward stops one base apart",
    ("rs_rs", -1): "letters: two reverse stops one base apart", ("rs_rs", 1): "letters: two reverse stops one base apart",
    ("fs_rb_apart", -1): "letters: as fs_rs +1", ("fs_rb_apart", 0): "letters: as fs_rs 0",
    ("tri_ovlp0", 1): "letters: as fs_rs 0 (overlaps 1, 2, 3 cannot be written; 4 is the first)",
    ("tri_no_traceb", 0): "a forward stop without a traceb is refused as a source before the rule is reached (the edge-artifact test)",
    ("igm_adj2", 1): "letters: as fs_fb +1 / rb_rs +1",
    ("igm_adj1", -1): "two nodes of one strand at one position are one codon", ("igm_adj1", 1): "letters: a start two bases before a stop",
    ("igm_ovl", 1): "forward: as fs_fb +1; reverse: a stop codon right before the start codon, in its frame, ends that start's ORF",
    ("igm_oper_ovl", 0): "an overlapping pair is 60 apart only in one frame: one ORF, the start is the stop's own",
    ("igm_quarter_ovl", 0): "as igm_oper_ovl 0, at 15",
    ("ovl_f_skip", -1): "letters: as fs_fb +1", ("ovl_r_skip", 1): "letters: as rb_rs +1",
    ("ovl_f_stopval", -1): "letters: as fs_fs", ("ovl_f_stopval", 1): "letters: as fs_fs",
    ("ovl_r_stopval", -1): "letters: as rs_rs", ("ovl_r_stopval", 1): "letters: as rs_rs",
}
# counters that count events, not differences: the slots that mean something
EVENT_SLOTS = {"fs_fs_star": (-1, 1), "rs_rs_star": (-1, 1), "artifact": (0,), "tri_no_traceb": (0,), "ovl_edge_stop": (0,)}
# not built: what the catalogue leaves open on purpose (DESIGN.md lists them)
NOT_BUILT = {
    "the walk-back search starting at the far end of its bracket, lo - 2 (ndx[lo] - stop_val) - 2":
        "needs two nodes at EVERY position between the ORF's far end and node lo; a start codon needs three letters to itself on its strand",
    "a target whose window start is the first node of its segment's sub-chain, or the node before it":
        "the window begins 1 000 nodes back, the shrunk plan's sub-chain 64 to 128; and `rb` answers 0 for v = a and v = a - 1 alike",
    "a reverse stop's third node on a sub-chain's first node":
        "the third node lies behind its stop and enters as values and positions, not as a re-based index (the operon sources c0..c2 do: segment/operon)",
}


# ---- (b) the intergenic term: gene end -> gene begin of the same strand ---------------------------------------------------------------

IGM_DISTANCES = (2, 3, 4, 14, 15, 16, 59, 60, 61, 179, 180, 181, 182)
IGM_RIVAL = {"oper": 0.0, "far": -IG}          # what the rival source's connection is worth in each design


def igm_formula(dist, overlap=False):
    """ref: _connection.h:52-78 without the adjacency term."""
    if dist > 180:
        return -IG
    if (dist <= 60 and not overlap) or dist * 4 < 60:
        return (2.0 - dist / 60) * 0.15 * ST_WT          # in the reference's order of operations: the scores are compared to the last bit
    return 0.0


def igm_series():
    """Gene 0 (begin b0: 100), then gene 1 right behind it, then the target: the begin of gene 2, d bases after the end of gene 1.
    The end of gene 1 (the probe source) is worth the end of gene 0 (the rival) minus 0.3 -- gene 1's own begin is priced for that --
    so it wins the target while its intergenic term is >= 0 and the rival's is 0 ("oper": the rival 61 .. 180 bases from the target,
    the flip is at d = 60 / 61) or while it is 0 and the rival's -0.15 st_wt ("far": the rival beyond 180, the flip at 180 / 181).
    In place on either strand: `e` + 3 below is the first base after a gene's end codon."""
    out = []
    for strand in (1, -1):
        for mode in ("oper", "far"):
            for d in IGM_DISTANCES:
                if (mode == "oper" and d > 61) or (mode == "far" and d < 59):
                    continue
                span = 90 if mode == "oper" else 240          # begin to end of gene 1
                lay = Layout(900)
                x0 = 60
                y0 = x0 + 120
                x1 = y0 + 3                                    # 3 bases behind the end of gene 0: (2 - 3/60) IG
                y1 = x1 + span
                x2 = y1 + d
                lay.gene("g0", x0, y0, strand)
                lay.gene("g1", x1, y1, strand)
                lay.gene("g2", x2, x2 + 120, strand)
                begin, end = ("b", "s") if strand == 1 else ("s", "b")
                price = -0.3 - igm_formula(3)
                scores = {"g0" + ("b"): dict(cscore=100.0), "g1b": dict(cscore=price), "g2b": dict(cscore=7.0)}
                src, rival, tgt = "g1" + end, "g0" + end, "g2" + begin
                rival_dist = x2 - y0
                assert (61 <= rival_dist <= 180) if mode == "oper" else rival_dist > 181
                allowed = d > 2 and igm_formula(d) - 0.3 >= IGM_RIVAL[mode]      # at 2 the codons share a letter: `left + 2 >= right`
                out.append(shape("igm/%s/%s/d%d" % (mode, "+-"[strand < 0], d), lay, scores, (src, tgt, allowed), "igm/%s/%s" % (mode, "+-"[strand < 0]), d,
                                 dict(rival=rival, formula=igm_formula(d), lose=IGM_RIVAL[mode] + 0.3)))
    return out


# ---- (a) pair rules ----------------------------------------------------------------------------------------------------------------------

SIGN = {1: "+", -1: "-"}


def opposite_series():
    """A gene's end, then the begin of a gene of the OTHER strand g bases on: forward stop -> reverse stop (`left + 2 >= right - 2`) and,
    in place on the other strand, reverse start -> forward start (`left >= right`).  g counts from the first base of the end codon
    to the first base of the begin codon.  Forward: g = 3 is the first that does not share a letter and connects (lhs - rhs = -1);
    g = -1 (TTAA) shares two letters and sorts the reverse stop behind the forward one, refused (+3).  Reverse: g = 3 connects (-1),
    g = 2 is CATTG, a TTG start on the last letter of CAT, refused (0); g = 4 cannot be written without a further codon (CATxATG: x = C reads
    CAT, G reads ATG, A reads TAA, T reads TTA), so the far neighbour is 5."""
    out = []
    for strand, gaps in ((1, ((-1, False), (3, True), (4, True))), (-1, ((2, False), (3, True), (5, True)))):
        for g, allowed in gaps:
            lay = Layout(700)
            lay.gene("g0", 60, 180, strand)
            x1 = 180 + g
            lay.gene("g1", x1, x1 + 120, -strand, start_codon="TTG" if (strand, g) == (-1, 2) else None)
            end, begin = ("s", "s") if strand == 1 else ("b", "b")
            scores = {"g0b": dict(cscore=100.0), "g1b": dict(cscore=7.0)}
            out.append(shape("opposite/%s/g%d" % (SIGN[strand], g), lay, scores, ("g0" + end, "g1" + begin, allowed), "opposite/" + SIGN[strand], g))
    return out


def _fs_rb(name, series, at, A, m, X, G, allowed):
    """Forward gene [A - 3m, A]; a reverse gene whose stop node lies X before A (bs = A - X) and whose start node G after that."""
    lay = Layout(1400)
    lay.gene("a", A - 3 * m, A, 1)
    p = A - X - 2
    lay.gene("b", p, p + G, -1)
    scores = {"ab": dict(cscore=100.0), "bb": dict(cscore=0.0)}
    return shape(name, lay, scores, ("as", "bb", allowed), series, at, dict(refused_traceb="bs"))


def fs_rb_series():
    """Forward stop -> reverse start, a reverse gene that reaches back over the forward gene's end: each of the four tests at equality
    and beside it (ref: _connection.h:205-267).  With A the forward stop, bs / bn the reverse gene's stop / start node, X = A - bs:
      apart  `bs - 2 >= A + 2`: bs = A + 5 refused (+1), A + 1 allowed (-3); A + 4, A + 3 cannot be written (IMPOSSIBLE)
      ovlp   `X + 5 >= 200`
      half   `X >= bn - A + 3`
      bnd    `X >= bs - 3 - bnd`, bnd the forward gene's own start
    Refused, the reverse start keeps its own stop (a sum of exactly 0.0 connects)."""
    A, out = 700, []
    for bs_off, allowed in ((5, False), (1, True), (-1, True)):
        out.append(_fs_rb("fs_rb/apart/%+d" % bs_off, "fs_rb/apart", bs_off, A, 60, -bs_off, 120, allowed))
    for ovlp in (198, 199, 200, 201):
        out.append(_fs_rb("fs_rb/ovlp/%d" % ovlp, "fs_rb/ovlp", ovlp, A, 140, ovlp - 5, 420, ovlp < 200))
    for k, G, X in ((-1, 96, 49), (0, 99, 51), (1, 96, 50)):
        assert X - (G - X + 3) == k
        out.append(_fs_rb("fs_rb/half/%+d" % k, "fs_rb/half", k, A, 60, X, G, k < 0))
    for k, m, X in ((-1, 40, 58), (0, 41, 60), (1, 40, 59)):
        assert X - (A - X - 3 - (A - 3 * m)) == k
        out.append(_fs_rb("fs_rb/bnd/%+d" % k, "fs_rb/bnd", k, A, m, X, 240, k < 0))
    return out


def _triple(name, series, at, a, m, X, Gn, mark, c3=5.0, maxov=60):
    """Forward gene [a - 3m, a]; reverse gene N = [ns, n3] with ns = a - X reaching back over a; reverse gene B whose stop b lies 31
    before n3, so that n3 is b's overlapping start (another frame than N's).  mark: is N's frame taken (ov_mark = n3 % 3)?"""
    lay = Layout(1500)
    lay.gene("a", a - 3 * m, a, 1)
    pn = a - X - 2
    lay.gene("n", pn, pn + Gn, -1)
    pb = pn + Gn - 31
    lay.gene("b", pb, pb + 150, -1)
    scores = {"ab": dict(cscore=100.0), "nb": dict(cscore=c3), "bb": dict(cscore=1.0)}
    n3 = pn + Gn + 2
    # N clear of the forward gene (X <= -5): the forward stop reaches b through N's own stop and the operon rule, worth n3's scores; taking
    # N's frame in the triple rule all the same would offer 0.65 more and take the target
    return shape(name, lay, scores, ("as", "bs", X > -5), series, at, dict(ov_mark=n3 % 3 if mark else -1, refused_traceb="ns"), maxov)


def triple_series():
    """Forward stop -> reverse stop with a third gene N between them on the reverse strand, whose start n3 is the target's overlapping
    start and whose stop lies `ovlp` = left - ns + 3 inside the forward gene (ref: _connection.h:270-367).  The connection is allowed
    either way; the rule decides whether N's frame is taken (ov_mark, and n3's scores in place of the intergenic term).
      ovlp0    ovlp <= 0: -1, 0 refused, 4 taken (1, 2, 3 cannot be written), each in the three frames of star_ptr
      ovlp200  198 .. 201
      n3       `ovlp >= n3 - left`
      traceb   `ovlp >= ns - nod[traceb].ndx - 2`
      zero     a candidate worth exactly 0.0 (not taken: strict `>`) and the smallest double above it"""
    import math
    out = []
    for shift in range(3):
        for ovlp in (-1, 0, 4):
            out.append(_triple("triple/ovlp0/f%d/%d" % (shift, ovlp), "triple/ovlp0/f%d" % shift, ovlp, 700 + shift, 60, ovlp - 5, 120, ovlp > 0))
    for ovlp in (198, 199, 200, 201):
        out.append(_triple("triple/ovlp200/%d" % ovlp, "triple/ovlp200", ovlp, 700, 140, ovlp - 5, 420, ovlp < 200))
    for k, Gn, X in ((-1, 90, 41), (0, 93, 43), (1, 90, 42)):
        assert 2 * X + 7 - Gn == k
        out.append(_triple("triple/n3/%+d" % k, "triple/n3", k, 700, 60, X, Gn, k < 0))
    for k, m, X in ((-1, 40, 56), (0, 41, 58), (1, 40, 57)):
        assert 2 * X + 7 - 3 * m == k
        out.append(_triple("triple/traceb/%+d" % k, "triple/traceb", k, 700, m, X, 240, k < 0))
    for c3, mark in ((0.0, False), (math.ulp(0.0), True), (-math.ulp(0.0), False)):
        out.append(_triple("triple/zero/%r" % c3, "triple/zero", c3, 700, 60, 20, 120, mark, c3=c3))
    return out


# ---- operons: the third node behind star_ptr; (c) overlapping starts ----------------------------------------------------------------

OPERON_DISTANCES = (-2, 1, 13, 14, 16, 17)          # multiples of 3 share the frame: one ORF, no overlap (IMPOSSIBLE); and those around max_overlap
ADJ_SCORES = {"neg": dict(rscore=-1.5, uscore=-2.5), "pos": dict(rscore=1.5, uscore=0.0), "mixed": dict(rscore=-0.75, uscore=3.0)}


def operon_series(maxov=60):
    """Gene A, and gene B whose begin lies d bases before A's end codon (d = -2: TAATG / CATTA, the begin on the end codon's last
    letter; d = 1: ATGA / TCAT, one base before it): forward stop -> forward stop through B's start, and in place reverse stop ->
    reverse stop through A's start; d = -3: the begin right behind the end codon, in its frame (the look-ahead of three indices meets
    it and `> ndx + 2` skips it).  The third node is an overlapping start while d <= max_overlap (and d >= -2); beyond, star_ptr
    of the frame is -1 and the rule refuses.  The target's score carries igm_same of an overlapping pair: a bonus below 15 only.
    Distances are scaled to max_overlap for (c): 60 -> maxov."""
    out = []
    dists = tuple(d for d in OPERON_DISTANCES if abs(d) < 20) + tuple(d for d in range(maxov - 2, maxov + 3) if d % 3) + (-3,)
    if maxov == 200:
        dists += (59, 61, 62)                         # `dist <= OPER_DIST` of an overlapping pair
    for strand in (1, -1):
        for d in dists:
            for adj in (("neg", "pos", "mixed") if d in (-2, 1) else ("neg",)):
                lay = Layout(900)
                yA = 300
                span = 120 if maxov < 200 else 240
                xB = yA - d
                if strand == 1:
                    lay.gene("a", yA - span, yA, 1, stop_codon="TGA" if d == 1 else None)
                    lay.gene("b", xB, xB + span, 1)
                    third, src, tgt, other = "bb", "as", "bs", "bb"
                else:
                    lay.gene("a", yA - span, yA, -1)
                    lay.gene("b", xB, xB + span, -1, stop_codon="TCA" if d == 1 else None)
                    third, src, tgt, other = "ab", "as", "bs", None
                scores = {"ab": dict(cscore=100.0), "bb": dict(cscore=7.0)}
                scores[third] = dict(scores[third], sscore=0.5, **ADJ_SCORES[adj])
                allowed = -2 <= d <= maxov
                if maxov == 200 and d == 14:                  # a second start codon of A, 99 before its stop: within max_overlap, but its stop_val IS the stop
                    lay.start("ax", yA - 99 if strand == 1 else yA - span + 99, strand, yA if strand == 1 else yA - span + 2)
                out.append(shape("operon%d/%s/d%d/%s" % (maxov, SIGN[strand], d, adj), lay, scores, (src, tgt, allowed), "operon%d/%s" % (maxov, SIGN[strand]), (d, adj),
                                 dict(third=third, refused_traceb=other if d > 0 else 0, overlap_dist=abs(d)), maxov))
    return out


# ---- (d) windows -------------------------------------------------------------------------------------------------------------------------

WINDOW_TARGETS = (499, 500, 501, 999, 1000, 1001, 1002)


def window_series():
    """The dominating source is node 1 (the end of gene D, worth 100), the target -- the begin of gene T -- node i, a run of i - 3 filler
    nodes between them.  The window starts at max(0, i - 1000) (ref: lib.pyx:1221-1233 without the stretch): node 1 is its first node
    at i = 1001 and one before it at i = 1002, where the target falls to the filler's end."""
    out = []
    for strand in (1, -1):
        for i in WINDOW_TARGETS:
            lay = Layout(400)
            lay.gene("d", 60, 180, strand)
            at = lay.run("r", 200, i - 3, strand)
            lay.gene("t", at + 30, at + 150, strand)
            end, begin = ("s", "b") if strand == 1 else ("b", "s")
            scores = {"db": dict(cscore=100.0), "tb": dict(cscore=7.0)}
            out.append(shape("window/%s/i%d" % (SIGN[strand], i), lay, scores, ("d" + end, "t" + begin, i <= 1001), "window/" + SIGN[strand], i,
                             dict(index={"t" + begin: i, "d" + end: 1}, window={"t" + begin: (max(0, i - 1000), False, max(0, i - 500))})))
    return out


WINDOW_LO = (7, 8, 12)          # the window's first node: the last node of a block of eight, the first, one inside


def window_lo_series():
    """The window's first node at 7, 0 and 4 (mod 8): the blocks of eight of the ring and of the max tree in the chain kernel, and the
    first node of the far range of k_dp_wave (its S1 / S2 / suffix pieces: the range begins at a block's last node, at its first, and
    inside one).  As window_series behind lo - 1 filler nodes: the dominating source is node lo of a target at 1000 + lo, and one
    before the window of a target at 1001 + lo."""
    out = []
    for strand in (1, -1):
        for lo in WINDOW_LO:
            for delta in (0, 1):
                lay = Layout(400)
                at = lay.run("p", 60, lo - 2, strand) + 60
                lay.gene("d", at, at + 120, strand)
                i = 1000 + lo + delta
                at = lay.run("r", at + 140, i - lo - 2, strand)
                lay.gene("t", at + 30, at + 150, strand)
                end, begin = ("s", "b") if strand == 1 else ("b", "s")
                scores = {"db": dict(cscore=100.0), "tb": dict(cscore=7.0)}
                out.append(shape("window_lo/%s/lo%d/%+d" % (SIGN[strand], lo, delta), lay, scores, ("d" + end, "t" + begin, delta == 0),
                                 "window_lo/%s/lo%d" % (SIGN[strand], lo), delta,
                                 dict(index={"t" + begin: i, "d" + end: lo}, window={"t" + begin: (lo + delta, False, 500 + lo + delta)}, lo_mod8=(lo + delta) % 8)))
    return out


def artifact_series():
    """The edge-artifact rule (ref: _connection.h:100-103): a forward stop, or a reverse start, that no connection has reached is no
    source.  Gene A at the default scores -- its begin costs 50, so its end is never reached -- and the begin of gene T behind it, 30
    bases (the intergenic term alone would be worth 0.15 st_wt (2 - 30 / 60) > 0) and 100 bases on (worth 0.0: `>=` would still
    connect): A's end is the ONLY source the target has, and the target stays without a traceb, at 0.0."""
    out = []
    for strand in (1, -1):
        for d in (30, 100):
            lay = Layout(700)
            lay.gene("a", 60, 180, strand)
            lay.gene("t", 180 + d, 300 + d, strand)
            end, begin = ("s", "b") if strand == 1 else ("b", "s")
            out.append(shape("artifact/%s/d%d" % (SIGN[strand], d), lay, {"tb": dict(cscore=7.0)}, ("a" + end, "t" + begin, False), None, d,
                             dict(refused_traceb=None, artifact=True)))
    return out


SEG_FIRST_128 = 192      # with segments of 128 nodes the sub-chain of nodes 256 .. 383 begins at node 192: two batches before a target at 337
SEG_FIRST = 128          # under the shrunk plan (segments of 64 from 256 nodes on, warm-up 64) the sub-chain of nodes 192 .. 255 begins at node 128


def segment_series():
    """load_target re-bases a target's indices to its segment's sub-chain: a range that begins before the sub-chain begins at 0 (`rb`), a
    single node before it is "none" (`one`: a reverse start's own stop, a reverse stop's operon source).  A reverse gene G whose stop
    is node 128 -- the first node of the sub-chain that nodes 192 .. 255 are walked in -- or node 127, one before it, with 80 filler
    nodes inside it (another frame) so that its begin is node 210 / 209:
      own     the target is G's begin, the single node its own stop
      operon  the target is the stop of a gene B that begins 14 bases before G's begin: the single node is G's stop again, as the operon
              source, through G's begin as B's overlapping start
    G's begin is worth 0.5, less than the 0.15 st_wt a later gene begin would cost, and every filler start costs 50: nothing else in
    the chain is reached, so every segment's walk from scores of 0 is exact already and the verification rejects nothing -- except, with
    the stop one node before the sub-chain, the target itself, which the exact re-scoring then repairs.  The results are the serial
    loop's either way.
    The chain kernel walks the batch before a target's own from registers, and under the shrunk plan a sub-chain is two batches long:
    there the single node always lies in that batch.  The second set (`segment128`, segments of 128 nodes, the same warm-up) puts it two
    batches before the target, where the far field looks it up by the re-based index."""
    out = []
    for first, inner_n, label in ((SEG_FIRST, 79, "segment"), (SEG_FIRST_128, 143, "segment128")):
      for kind in ("own", "operon"):
        for before in (0, 1):
            lay = Layout(400)
            at = lay.run("p", 60, first - before - 1, -1) + 60
            at += (61 - at) % 3                                   # G's codons at 1 (mod 3), the run inside it at 0: the stops it reads are not G's
            lay.stop("gs", at, -1)
            inner = lay.run("in", at + 99 + 32, inner_n, -1)
            yG = inner + (at - inner) % 3 + 30
            lay.start("gb", yG, -1, at + 2)
            scores = {"gb": dict(cscore=0.5)}
            end = yG + 300                                        # the next gene begin beyond 180 bases: it would cost 0.15 st_wt
            if kind == "operon":
                lay.gene("b", yG - 14, yG - 14 + 120, -1)
                probe, tgt = ("gs", "bs", True), first + inner_n + 2
                scores["gb"] = dict(cscore=0.25, sscore=0.25)
            else:
                probe, tgt = ("gs", "gb", True), first + inner_n + 2
            lay.run("tail", end + (0 - end) % 3, 119, -1)
            out.append(shape("%s/%s/%s" % (label, kind, "before" if before else "first"), lay, scores, probe, None, None,
                             dict(index={"gs": first - before, probe[1]: tgt - before}, segment=dict(clean=not before))))
    return out


def giant_series():
    """A gene G of more than 500 nodes' length (a filler run of 600 inside it, in another frame): for its end on the forward strand
    (a forward stop) and its begin on the reverse strand (a reverse start) the window is stretched to the node at stop_val, the
    ORF's far end, then widened by 500 (ref: lib.pyx:1224-1231).  G's begin codon right behind that far end is worth 100, a second
    one close to the target 3: the target's traceb is the far one only if the stretched window holds it.
      one      the walk lands on the one node at stop_val (forward: the stop of a gene P before G; reverse: G's own stop)
      two      ... on the higher of two nodes at that position (CATAA: a reverse start on the forward stop; TTATG: a forward start
               on the reverse stop)
      none     no node has the position (forward: the frame holds no stop before G, stop_val = frame - 6): the walk ends at 0.
               A reverse start's stop_val is its own stop node's position: no such case (IMPOSSIBLE)
    each with nothing before it (the second 500 clamped at 0) and with a run of 700 nodes before it (not clamped)."""
    out = []
    for strand in (1, -1):
        for case in ("one", "two", "none"):
            if strand == -1 and case == "none":
                continue
            for pre in (0, 700):
                lay = Layout(400)
                f = 61                                              # codon positions of G are 61 mod 3 = 1
                at = 60
                if pre:
                    at = lay.run("pre", 60 + (2 if strand == 1 else 0), pre, strand)         # codon class 2 (forward) / 0 (reverse): not G's, and the stops it reads are not
                    at += (f - at) % 3 + 30
                if strand == 1:
                    if case != "none":
                        lay.gene("p", at, at + 120, 1)
                        if case == "two":
                            lay.gene("q", at + 120 - 2 - 99, at + 120 - 2, -1)      # its start codon CAT ends on the T of P's TAA
                        g_begin = at + 123
                    else:
                        g_begin = at
                    inner = lay.run("in", g_begin + 31, 600, 1)       # codon class of G + 1
                    assert (g_begin + 31) % 3 == (g_begin + 1) % 3
                    g2 = inner + (g_begin - inner) % 3 + 30
                    lay.start("gb", g_begin, 1, g2 + 120)
                    lay.start("g2b", g2, 1, g2 + 120)
                    lay.stop("gs", g2 + 120, 1)
                    tgt, far = "gs", "gb"
                else:
                    g_stop = at
                    lay.stop("gs", g_stop, -1)
                    if case == "two":
                        lay.gene("q", g_stop + 2, g_stop + 2 + 120, 1)  # TTATG
                    lay.start("g2b", g_stop + 99, -1, g_stop + 2)      # G's nearest begin codon to its stop ... the far one from the target
                    inner = lay.run("in", g_stop + 99 + 32, 600, -1)   # codon class of G + 2
                    assert (g_stop + 99 + 32) % 3 == (g_stop + 2) % 3
                    gb = inner + (g_stop - inner) % 3 + 30
                    lay.start("gb", gb, -1, g_stop + 2)
                    tgt, far = "gb", "gs"
                if strand == 1:
                    scores = {"gb": dict(cscore=100.0), "g2b": dict(cscore=3.0)}
                    probe = ("gb", "gs", True)
                else:                                               # the reverse start's source is its own stop, the node looked for
                    scores = {"gb": dict(cscore=100.0)}
                    probe = ("gs", "gb", True)
                out.append(shape("giant/%s/%s/pre%d" % (SIGN[strand], case, pre), lay, scores, probe, None, None,
                                 dict(giant=dict(target=tgt, case=case, clamped=not pre)), 60))
    return out


def two_frames_series():
    """Two genes begin inside gene A, 13 and 29 bases before its end codon, in the two other frames.  po_overlapping_starts meets the
    nearer one first; the farther one takes its frame's place only if it is worth strictly more (ref: lib.pyx:2301-2305 / 2322-2326).
    Worth the same to the last bit: its frame stays empty and the operon connection into its gene is refused."""
    import math
    out = []
    near = (7.0 + 0.5) + (2.0 - 13 / 60) * 0.15 * ST_WT           # cscore + sscore + igm_same of an overlapping pair 13 apart
    for strand in (1, -1):
        for what, c in (("below", math.nextafter(near, 0.0)), ("equal", near), ("above", math.nextafter(near, 1e9))):
            lay = Layout(900)
            yA = 300
            lay.gene("a", yA - 120, yA, strand)
            lay.gene("b", yA - 13, yA - 13 + 120, strand)
            lay.gene("c", yA - 29, yA - 29 + 150, strand)
            if strand == 1:
                scores = {"ab": dict(cscore=100.0), "bb": dict(cscore=7.0, sscore=0.5), "cb": dict(cscore=c)}
                probe = ("as", "cs", what == "above")
            else:           # the stop is B's / C's, the overlapping start A's: one candidate per stop, nothing to replace -- run for the values
                scores = {"ab": dict(cscore=c), "bb": dict(cscore=7.0), "cb": dict(cscore=3.0)}
                probe = None
            out.append(shape("twoframes/%s/%s" % (SIGN[strand], what), lay, scores, probe, "twoframes/" + SIGN[strand] if probe else None, what))
    return out


def edge_stop_series():
    """OPEN contigs: ORFs that run off an end give edge nodes -- a stop without a codon (edge = 1), which takes no overlapping start, and
    a start whose stop_val is no node's position when its ORF holds no other start.  A gene B, and a start codon 14 bases before B's
    end whose ORF runs off the end of the contig: through an ordinary stop at its end that start would be B's overlapping start.
    Every start is worth 2 (meta["default"]): the chain runs through the edge genes."""
    out = []
    for strand in (1, -1):
        lay = Layout(500, closed=False)
        L = 420
        if strand == 1:
            lay.gene("b", 200, 320, 1)
            lay.start("x", 306, 1, None, count=False)
        else:
            lay.gene("b", 200, 320, -1)
            lay.start("x", 212, -1, None, count=False)
        seq = lay.seq()[:L] if strand == 1 else lay.seq()[100:L]          # cut behind / before the start codon's ORF: it runs off the end
        default = {"start": dict(DEFAULT["start"], cscore=2.0), "stop": DEFAULT["stop"]}
        out.append(Shape("edge/" + SIGN[strand], seq, False, {}, None, {}, None, None, None, dict(edge=True, default=default), 60))
    return out


# ---- (e) where the pair lies in the kernel's own units ---------------------------------------------------------------------------------

RS3 = "TTACTTACTTA"        # a reverse stop in each frame, no codon of the forward strand
FS3 = "TAAGTAAGTAA"        # a forward stop in each frame, no codon of the reverse strand


def _far_pair(name, strand, d, pad, tail, dense=None, series=None, meta=None):
    """The "far" design of igm_series (the probe source wins at d = 180 and loses at 181) behind `pad` filler nodes and before `tail`
    more.  dense = r: r repeats of CATG, a forward and a reverse start each, between the probe source and the target, with
    the stops they need in every frame far to the left and to the right (RS3, FS3): more nodes within 3 * OPER_DIST than a batch holds."""
    lay = Layout(400)
    at = 60
    if dense:
        lay.put(at, RS3, after="C")
        lay.implicit += [("rs", at + 4 * k + 2) for k in range(3)]
        at += 30
    if pad:
        assert pad >= 2
        at = lay.run("pad", at + 30, pad - 1, strand) + 230
    x0 = at + 30
    y0 = x0 + 120
    x1 = y0 + 3
    y1 = x1 + 240
    x2 = y1 + d
    lay.gene("g0", x0, y0, strand)
    lay.gene("g1", x1, y1, strand)
    lay.gene("g2", x2, x2 + 120, strand)
    at = x2 + 123
    n_dense = 0
    if dense:
        r = dense
        p = y1 + 8
        assert p + 4 * r < x2 - 6
        lay.put(p, "CATG" * r, before="G", after="C")
        lay.put(at + 90, FS3, before="G")
        lay.implicit += [("fs", at + 90 + 4 * k) for k in range(3)]
        at += 90 + 11
        n_dense = 2 * r
    if tail:
        assert tail >= 2
        lay.run("tail", at + 30, tail - 1, strand)
    end, begin = ("s", "b") if strand == 1 else ("b", "s")
    price = -0.3 - igm_formula(3)
    scores = {"g0b": dict(cscore=100.0), "g1b": dict(cscore=price), "g2b": dict(cscore=7.0)}
    sh = shape(name, lay, scores, ("g1" + end, "g2" + begin, d <= 180), series, d, meta)
    return sh, n_dense


def lane_series():
    """The decisive pair at 180 / 181 with the target in lane 63 and lane 0 of a 64-node batch: the source in its own batch, and in the
    last lane of the batch before."""
    out = []
    for strand in (1, -1):
        for tgt in (63, 64, 127, 128):
            for d in (180, 181):
                sh, _ = _far_pair("lane/%s/t%d/d%d" % (SIGN[strand], tgt, d), strand, d, tgt - 4, 40, series="lane/%s/t%d" % (SIGN[strand], tgt),
                                  meta=dict(index={"g2" + ("b" if strand == 1 else "s"): tgt, "g1" + ("s" if strand == 1 else "b"): tgt - 1}))
                out.append(sh._replace(n_nodes=tgt + 2 + 40))
    return out


SIZES = (255, 256, 257, 319, 320, 321, 1023, 1024, 1025)       # the shrunk segment plan (256 / 64 / 64) and PGA_RING


def size_series():
    """Chains of exactly N nodes around the decisive pair, whose target is node 128 (its p_near -- the probe source at 180 bases -- node
    127, one before a segment's first node under the shrunk plan) or node 129 (p_near 128, a segment's first node; 0 and 7 mod 8)."""
    out = []
    for strand in (1, -1):
        for N in SIZES:
            for tgt in (128, 129):
                for d in (180, 181):
                    sh, _ = _far_pair("size/%s/n%d/t%d/d%d" % (SIGN[strand], N, tgt, d), strand, d, tgt - 4, N - tgt - 2, series="size/%s/n%d/t%d" % (SIGN[strand], N, tgt),
                                      meta=dict(index={"g2" + ("b" if strand == 1 else "s"): tgt}, chain=N))
                    out.append(sh._replace(n_nodes=N))
    return out


DENSE = (31, 32, 33)         # repeats of the block: 62, 64, 66 nodes, and the probe source when it lies at 180


def dense_series():
    """The target in lane 0 with 62 .. 67 nodes within 3 * OPER_DIST bases before it: its p_near lies in the batch before (up to 64) or two
    batches back (from 65 on, where the step schedule reports a miss and the launch falls back to k_dpw_dyn).  At d = 180 the probe
    source is one more node within reach than the block holds."""
    out = []
    for strand in (1, -1):
        for r in DENSE:
            for d in (180, 181):
                inside = 2 * r + (d == 180)
                # nodes before the target without the padding: two genes, the block, and the stops of RS3 that end an ORF with a start in it
                # (all three on the forward strand; on the reverse strand the stops of the padding and of gene 1 end two of the frames first)
                base = 4 + 2 * r + (3 if strand == 1 else 1)
                pad = 192 - base
                name = "dense/%s/r%d/d%d" % (SIGN[strand], r, d)
                sh, n_dense = _far_pair(name, strand, d, pad, 30, dense=r, series="dense/%s/r%d" % (SIGN[strand], r),
                                        meta=dict(index={"g2" + ("b" if strand == 1 else "s"): 192}, near=inside))
                out.append(sh._replace(n_nodes=192 + 2 + (2 if strand == 1 else 3) + 30))       # the target gene, the stops of FS3 likewise, the tail
    return out


AHEAD = ((191, 0), (192, 0), (193, 0), (447, 0), (448, 0), (449, 0), (192, 245), (192, 244))      # nodes to the next forward stop, padding


def ahead_series():
    """A forward stop A whose next forward stop -- of one frame only; the other two frames have none behind it -- lies `ahead` nodes on:
    the end of an ORF R that begins inside gene A and holds ahead + 9 start codons, ten of them before A's stop.  A connects to it by
    the operon rule through the start 5 bases before A's stop (worth 5).  With padding A is node 255 / 256 of the contig."""
    out = []
    for ahead, pad in AHEAD:
        lay = Layout(400)
        at = 60
        if pad:
            at = lay.run("pad", 62, pad - 1, 1) + 200          # codon class 2: the stops it reads are of class 0
        yA = at + 120 + (1 - (at + 120) % 3) % 3               # class 1
        lay.gene("a", yA - 120, yA, 1)
        k = ahead + 9
        js = [j for j in range(k + 2) if j not in (10, 11)]    # the two codons that would share letters with A's stop are left out
        stop_at = yA - 32 + 3 * js[-1] + 90
        for j in js:
            lay.start("r%d" % j, yA - 32 + 3 * j, 1, stop_at)
        lay.implicit += [("fs", yA - 32 + 3 * j + 1) for j in js[:-1] if j + 1 in js]
        lay.stop("rs", stop_at, 1)
        scores = {"ab": dict(cscore=100.0), "r9": dict(cscore=5.0)}
        out.append(shape("ahead/%d/pad%d" % (ahead, pad), lay, scores, ("as", "rs", True), None, None,
                         dict(index={"as": pad + 11, "rs": pad + 11 + ahead})))
    return out


DEAD_END_GAP = 141         # nodes between the forward stop and its target: two batches, so every kernel meets it as a stored far value
DEAD_END_TAIL = 121        # nodes behind the target: 266 in all, a chain that the shrunk segment plan cuts


def dead_end_series():
    """The operon design at d = 13 -- gene A, gene B whose start lies 13 bases before A's end codon -- with B's ORF so long that
    DEAD_END_GAP reverse nodes lie between A's stop and B's: the tree kernels and the segment kernels then take what A's stop offers
    B's from the values stored when A's stop became final (`far_values`: V[frame] = score + x[frame]), not from a pair rule.
    DEAD_END_TAIL more reverse nodes follow, so that the shrunk segment plan cuts the chain and rebuilds those values (k_seg_build_far).
    `alive`: A's start is worth 100, its stop is reached and B's stop continues from it through B's start.  `dead`: A's start
    costs the default 50, its stop is never reached and offers nothing (ref: _connection.h:110-114) although 0 + x is more than
    B's own start gives; B's stop takes B's start."""
    out = []
    for state in ("alive", "dead"):
        lay = Layout(1200)
        lay.gene("a", 180, 300, 1)
        at = lay.run("pad", 330, DEAD_END_GAP - 1, -1)
        xB = 300 - 13
        yB = xB + 3 * ((at + 40 - xB) // 3 + 1)
        lay.gene("b", xB, yB, 1)
        lay.run("tail", yB + 40, DEAD_END_TAIL - 1, -1)
        scores = {"bb": dict(cscore=7.0, sscore=0.5)}
        if state == "alive":
            scores["ab"] = dict(cscore=100.0)
        out.append(shape("dead_end/+/%s" % state, lay, scores, ("as", "bs", state == "alive"), "dead_end/+", state,
                         dict(refused_traceb="bb", index={"as": 2, "bs": 3 + DEAD_END_GAP}, dead_end=state)))
    return out


LDS_STATIC = 3 * (6144 // 64) * 8 + 4 * 4      # s_m and s_cnt of k_dpw_topo_lds
LDS_FIRST_OVER = (65536 - LDS_STATIC - 32) // 12 + 1       # the first node count at which 12 n + 32 dynamic bytes and the static ones pass 64 KB
LDS_DYNAMIC_OVER = (65536 - 32) // 12 + 1                  # ... at which the dynamic bytes alone do
LDS_COUNTS = (LDS_FIRST_OVER - 1, LDS_FIRST_OVER, LDS_DYNAMIC_OVER - 1, LDS_DYNAMIC_OVER, 6143, 6144, 6145)


def lds_contigs():
    """{node count: contig} for LDS_COUNTS: synthetic sequence (dp_inject.contig_with_nodes' way: trimmed until the oracle extracts
    exactly that many nodes; a count that one sequence skips is taken from the next seed).  Scored under the "quant" family."""
    from tests import dp_inject
    from tests.util import synthetic_contig
    out = {}
    for seed in range(77, 97):
        seq = synthetic_contig(180000, 0.5, seed)
        if dp_inject.extracted(seq).num_nodes < max(LDS_COUNTS) + 8:
            continue
        for n in LDS_COUNTS:
            if n not in out:
                cut = dp_inject.trimmed_to_nodes(seq, n)
                if cut is not None:
                    out[n] = cut
        if len(out) == len(LDS_COUNTS):
            return out
    raise AssertionError(sorted(set(LDS_COUNTS) - set(out)))


def designed_index(sh, name):
    """Index of a named node in the sorted node list of a shape that names all its nodes (position ascending, forward first)."""
    assert sh.n_nodes == len(sh.nodes)
    order = sorted(sh.nodes, key=lambda k: (sh.nodes[k].ndx, -KIND[sh.nodes[k].kind][0]))
    return order.index(name)


def padded(sh, lane):
    """The shape behind a filler ORF of the reverse strand (a TTA, 90 bases, a run of CAT: its nodes are never reached, and neither
    strand's ORFs of the design see its codons), long enough to put the probe's target at `lane` of a 64-node batch: with lane 0 the
    probe source -- and whatever else lies before the target -- is in the batch before, where the kernel takes another path to the
    same pair (far ends and carries, not the in-batch walk).  Positions move by a multiple of 3."""
    ti = designed_index(sh, sh.probe[1])
    k = (lane - ti - 1) % 64                          # the filler's nodes: k starts and a stop
    if k < 2:
        k += 64
    filler = b"GCCGCCG" + b"TTA" + (b"CGC" * 29)[:87] + b"CAT" * k + b"C"
    filler += quiet(3 - len(filler) % 3 if len(filler) % 3 else 0)
    assert len(filler) % 3 == 0
    off = len(filler)

    def moved(n):
        sentinel = (n.kind == "fs" and n.stop_val < 0)
        return Node(n.kind, n.ndx + off, n.stop_val if sentinel else n.stop_val + off)
    nodes = {name: moved(n) for name, n in sh.nodes.items()}
    meta = dict(sh.meta, index={sh.probe[1]: ti + k + 1}, lane=lane)
    return sh._replace(name=sh.name + "/lane%d" % lane, seq=filler + sh.seq, nodes=nodes, n_nodes=sh.n_nodes + k + 1, meta=meta,
                       series=sh.series + "/lane%d" % lane if sh.series else None)


def all_pair_shapes():
    """The shapes of (a) - (c): tens of nodes each."""
    out = igm_series() + opposite_series() + fs_rb_series() + triple_series() + two_frames_series() + artifact_series()
    for m in (30, 60, 200):
        out += operon_series(m)
    return out


def all_shapes():
    pairs = all_pair_shapes()
    out = pairs + [mirrored(s) for s in pairs if s.series and s.series.split("/")[0] in ("igm", "fs_rb", "triple", "operon60")]
    out += [padded(s, 0) for s in pairs if s.probe] + [padded(s, 63) for s in pairs if s.probe and s.max_overlap == 60]
    return out + edge_stop_series() + window_series() + window_lo_series() + segment_series() + giant_series() + lane_series() + dense_series() + size_series() + ahead_series() + dead_end_series()
