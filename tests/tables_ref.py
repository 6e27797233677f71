"""The 24 NCBI genetic codes the library accepts, stated independently of the library's own copies: the standard code once, every
other table as the differences NCBI publishes, and a plain translator of one gene working on letters.  Reference for
tests/test_translation_tables_cpu.py and tests/test_translation_tables_gpu.py."""

BASES = "TCAG"
# the standard code (table 1) in NCBI's order: first base T, C, A, G; then the second; then the third
_STANDARD = ("FFLLSSSSYY**CC*W" "LLLLPPPPHHQQRRRR" "IIIMTTTTNNKKSSRR" "VVVVAAAADDEEGGGG")
STANDARD = {a + b + c: _STANDARD[16 * i + 4 * j + k] for i, a in enumerate(BASES) for j, b in enumerate(BASES) for k, c in enumerate(BASES)}

# differences from the standard code, as NCBI lists them ("N" in third place: all four codons)
DIFFERENCES = {
    1: "", 2: "TGA>W ATA>M AGA>* AGG>*", 3: "TGA>W CTN>T ATA>M", 4: "TGA>W", 5: "TGA>W ATA>M AGA>S AGG>S", 6: "TAA>Q TAG>Q",
    9: "TGA>W AAA>N AGA>S AGG>S", 10: "TGA>C", 11: "", 12: "CTG>S", 13: "TGA>W ATA>M AGA>G AGG>G",
    14: "TAA>Y TGA>W AAA>N AGA>S AGG>S", 15: "TAG>Q", 16: "TAG>L", 21: "TGA>W ATA>M AAA>N AGA>S AGG>S", 22: "TCA>* TAG>L",
    23: "TTA>*", 24: "TGA>W AGA>S AGG>K", 25: "TGA>G", 26: "CTG>A", 29: "TAA>Y TAG>Y", 30: "TAA>E TAG>E", 32: "TAG>W",
    33: "TAA>Y TGA>W AGA>S AGG>K",
}
TABLES = tuple(sorted(DIFFERENCES))

_NO_GTG = {1, 2, 3, 6, 10, 12, 14, 15, 16}
_NO_TTG = {1, 2, 3, 6, 9, 10, 14, 15, 16, 21, 22, 23, 24}


def code(table):
    """{codon: residue} of a table, over the 64 codons of A, C, G, T."""
    out = dict(STANDARD)
    for item in DIFFERENCES[table].split():
        codon, aa = item.split(">")
        for c in (BASES if codon[2] == "N" else codon[2]):
            out[codon[:2] + c] = aa
    return out


def stop_codons(table):
    return frozenset(c for c, aa in code(table).items() if aa == "*")


def start_codons(table):
    return frozenset(c for c, without in (("ATG", ()), ("GTG", _NO_GTG), ("TTG", _NO_TTG)) if table not in without)


_COMP = str.maketrans("ACGTN", "TGCAN")


def gene_letters(sequence, begin, end, strand):
    """The letters of a gene (1-based inclusive coordinates) as its own strand reads them, anything but A, C, G, T as N."""
    s = sequence.decode("ascii") if isinstance(sequence, (bytes, bytearray)) else sequence
    s = "".join(c if c in "ACGT" else "N" for c in s[begin - 1:end].upper())
    return s if strand == 1 else s.translate(_COMP)[::-1]


def translate(sequence, begin, end, strand, partial_begin, partial_end, table, include_stop=True, strict=True, unknown_residue="X"):
    """The protein of one gene.  `partial_begin` / `partial_end` are in sequence orientation (the left / right end of the gene
    runs off the sequence); the gene's own start is its left end on the forward strand and its right end on the reverse strand."""
    nuc = gene_letters(sequence, begin, end, strand)
    start_partial, stop_partial = (partial_begin, partial_end) if strand == 1 else (partial_end, partial_begin)
    n = len(nuc) // 3
    if not include_stop and not stop_partial:
        n -= 1
    tab, starts = code(table), start_codons(table)
    out = []
    for i in range(max(n, 0)):
        codon = nuc[3 * i:3 * i + 3]
        if "N" not in codon:
            if tab[codon] == "*":
                aa = "*"
            elif i == 0 and not start_partial and codon in starts:
                aa = "M"
            else:
                aa = tab[codon]
        else:
            aa = unknown_residue
            if not strict and "N" not in codon[:2]:
                family = {tab[codon[:2] + c] for c in BASES}
                if len(family) == 1:
                    aa = family.pop()
        out.append(aa)
    return "".join(out)


# ---- the inputs of the tests with several translation tables in one call ------------------------------------------------------------

def coded_contig(length, gc, seed, table):
    """Open reading frames on either strand between spacers of i.i.d. bases, written in the code of `table`: ATG, sense codons of
    that table drawn with their base frequencies (the codons other tables end a gene at among them), one of the table's stops."""
    import numpy as np
    rng = np.random.default_rng(seed)
    pb = {"A": (1 - gc) / 2, "C": gc / 2, "G": gc / 2, "T": (1 - gc) / 2}
    stops = sorted(stop_codons(table))
    sense = sorted(c for c in STANDARD if c not in stops)
    w = np.array([pb[c[0]] * pb[c[1]] * pb[c[2]] for c in sense])
    w /= w.sum()
    parts, n = [], 0
    while n < length:
        sp = "".join(rng.choice(list("ACGT"), size=int(rng.geometric(1 / 90.0)), p=[pb[b] for b in "ACGT"]))
        orf = "ATG" + "".join(rng.choice(sense, size=int(rng.geometric(1 / 250.0)), p=w)) + stops[int(rng.integers(len(stops)))]
        if rng.random() < 0.5:
            orf = orf.translate(_COMP)[::-1]
        parts += [sp, orf]
        n += len(sp) + len(orf)
    return "".join(parts)[:length].encode("ascii")


ODD_STOPS = ("AGA", "AGG", "TCA", "TTA", "TAA", "TAG", "TGA")          # every codon some table ends a gene at
_QUIET_CODONS = [c for c in sorted(STANDARD) if c not in ODD_STOPS and c[::-1].translate(_COMP) not in ODD_STOPS]


def revcomp(seq):
    return bytes(seq).translate(bytes.maketrans(b"ACGTN", b"TGCAN"))[::-1]


def quiet_codons(n, seed):
    """n codons that no table reads as a stop, on either strand, in their own frame."""
    import numpy as np
    rng = np.random.default_rng(seed)
    return "".join(rng.choice(_QUIET_CODONS, size=n))


def end_contigs():
    """Short contigs that end in an open reading frame whose last complete codon is one of ODD_STOPS, with 0, 1 or 2 bases behind
    it and lengths of every residue mod 3, then their reverse complements (the reverse strand's first codon): a table that reads
    the codon as a stop closes the frame there, any other leaves it open at the sequence end.  Returns (contigs, [(codon, position
    of the codon, strand)])."""
    from tests.util import synthetic_contig
    seqs, where = [], []
    for c, codon in enumerate(ODD_STOPS):
        for r in range(3):
            trail = (c + r) % 3
            tail = "ATG" + quiet_codons(70, 100 * c + r) + codon + "CG"[:trail]
            length = 3 * (200 + 14 * c) + r
            head = synthetic_contig(length - len(tail), 0.5, 7000 + 10 * c + r).decode()
            seqs.append((head + tail).encode())
            where.append((codon, length - trail - 3, 1))
    n = len(seqs)
    for k in range(n):
        seqs.append(revcomp(seqs[k]))
        where.append((where[k][0], len(seqs[k]) - 1 - where[k][1], -1))
    return seqs, where


TILE = 3072


def boundary_contigs():
    """Contigs without a stop in any frame but one codon of ODD_STOPS, written in the frame of the start codons, beginning at
    3070 .. 3074 and again at 6142 .. 6146 (across and next to the borders of the 3072-base extraction tiles), on either strand.
    Returns (contigs, [(codon, (the two positions of the codon's first base on its strand), strand)])."""
    unit = "GCC" * 100 + "ATG" + "GCC" * 100 + "GTG"
    fwd = unit * 11
    rev = revcomp(fwd.encode()).decode()
    seqs, where = [], []
    for strand, back in ((1, fwd), (-1, rev)):
        for codon in ODD_STOPS:
            for d in range(5):
                s = list("C" * ((TILE - 2 + d) % 3) + back[:2 * TILE + 500])
                word = codon if strand == 1 else revcomp(codon.encode()).decode()
                at = (TILE - 2 + d, 2 * TILE - 2 + d)
                for p in at:
                    s[p:p + 3] = word
                seqs.append("".join(s).encode())
                where.append((codon, at if strand == 1 else (at[0] + 2, at[1] + 2), strand))
    return seqs, where


# (statistics fixture, GC label, table) of the models of the several-table calls, in loading order: four groups in order of first
# appearance 4, 11, 15, 22 with 3, 1, 5 and 2 models, interleaved; all of them meet between GC 0.45 and 0.55, only the third group
# has a model near 0.70, only the fourth one near 0.28, and no model lies between 0.29 and 0.44
GROUP_SPEC = [(0, 0.47, 4), (2, 0.50, 11), (1, 0.70, 15), (3, 0.28, 22), (1, 0.45, 15), (3, 0.52, 4), (0, 0.49, 15), (2, 0.48, 22),
              (3, 0.53, 15), (1, 0.55, 4), (2, 0.51, 15)]


def group_models(tables=(4, 11, 15, 22)):
    """The models of GROUP_SPEC whose table is among `tables`: copies of three Shine-Dalgarno fixtures and of a model without
    Shine-Dalgarno motif (trained on KK037166) under other GC labels and tables."""
    from oracle import oracle as orc
    from tests.util import golden_path, read_fasta
    src = [orc.Training.load(golden_path("SRR492066.training.bin.gz")),
           orc.Training.load(golden_path("GCF_001457455.1_NCTC11397_genomic_100kb.tinf_closed.bin.gz")),
           orc.Training.load(golden_path("GCF_001457455.1_NCTC11397_genomic.tinf_closed.bin.gz")),
           orc.Oracle(read_fasta("KK037166.fna.gz")[0][1]).train()]
    assert src[3].uses_sd == 0
    out = []
    for s, gc, tt in GROUP_SPEC:
        if tt in tables:
            t = src[s].copy()
            t.set_gc(gc)
            t.set_trans_table(tt)
            out.append(t)
    return out


def group_order(models):
    """The tables of `models` in order of first appearance: the table groups of a device call."""
    order = []
    for m in models:
        if m.trans_table not in order:
            order.append(m.trans_table)
    return order


def group_contigs(unknown_runs=False):
    """About 45 contigs of 300 bases to 25 kb: reading frames written in each of the four codes near GC 0.5 (every group in the
    window), near 0.70 (the third group only) and near 0.28 (the fourth only), one near 0.37 (no model), plain random sequence, and
    the degenerate inputs.  `unknown_runs`: runs of N of 30 to 120 bases written over the longer ones."""
    import numpy as np
    from tests.util import synthetic_contig
    seqs, k = [], 0
    for tt in (4, 15, 11, 22):
        for length, gc in [(300, 0.5), (900, 0.48), (2500, 0.52), (6200, 0.5), (9300, 0.47), (14000, 0.53), (25000, 0.5)]:
            seqs.append(coded_contig(length, gc, 9000 + k, tt))
            k += 1
    for length, gc, tt in [(5000, 0.28, 22), (3000, 0.27, 11), (7000, 0.29, 4), (4100, 0.28, 22), (5000, 0.72, 15), (3100, 0.74, 11),
                           (8000, 0.71, 22), (4000, 0.36, 11)]:
        seqs.append(coded_contig(length, gc, 9100 + k, tt))
        k += 1
    seqs += [synthetic_contig(4000, 0.5, 1), synthetic_contig(1200, 0.45, 2), b"", b"ATG", b"N" * 400]
    if unknown_runs:
        rng = np.random.default_rng(5)
        for i, s in enumerate(seqs):
            if len(s) >= 2500:
                s = bytearray(s)
                for n in (30, 50, 75, 120):
                    at = int(rng.integers(0, len(s) - n))
                    s[at:at + n] = b"N" * n
                seqs[i] = bytes(s)
    return seqs


def group_winners(seqs, models, closed=False, mask=False):
    """Per contig, from the oracle alone: (winning model or -1, its group or -1, the groups with a model in the contig's GC window)."""
    from oracle import oracle as orc
    from tests import sets_ref
    order = group_order(models)
    out = []
    for s in seqs:
        o = orc.Oracle(s, mask=mask)
        w = o.find_genes_meta(models, orc.Params(closed=closed))
        gc = sets_ref.gc_count(s) / len(s) if len(s) else 0.0
        seen = sorted({order.index(models[m].trans_table) for m in sets_ref.models_in(gc, models)})
        out.append((w, order.index(models[w].trans_table) if w >= 0 else -1, seen))
    return out


SPECIAL_CODONS = ("CTN", "AGN", "TAN", "TGN", "ATN", "GCN", "NCT", "ANG")
SPECIAL_AT = 30          # the index of the first of them in the protein of a gene that carries them


def translation_contig(seed=31):
    """About 20 kb of reading frames in the code of table 4 (TGA among the sense codons) on either strand, each behind a ribosome
    binding site and an in-frame stop, with no other start codon inside: starts ATG, GTG and TTG on both strands, the eight
    SPECIAL_CODONS as whole codons from codon SPECIAL_AT on in some, a frame cut off at the contig's left end and one at its right
    end.  Returns (contig, [(begin, end, strand, start codon, carries the special codons)]) with 1-based inclusive coordinates; the
    two cut frames are not listed."""
    import numpy as np
    rng = np.random.default_rng(seed)
    sense = [c for c in sorted(STANDARD) if c not in ("TAA", "TAG", "ATG", "GTG", "TTG")]
    body = lambda n: "".join(rng.choice(sense, size=n))                                          # noqa: E731
    spacer = lambda n: "".join(rng.choice(list("ACGT"), size=n))                                 # noqa: E731
    parts, planted, n = [body(260) + "TAA"], [], 783
    plan = [("ATG", 1, False), ("GTG", 1, True), ("TTG", -1, True), ("TTG", 1, False), ("GTG", -1, False), ("ATG", -1, True),
            ("TTG", 1, True), ("GTG", 1, False), ("TTG", -1, False), ("GTG", -1, True), ("ATG", 1, False), ("TTG", 1, False),
            ("GTG", -1, False), ("TTG", -1, True), ("ATG", 1, True), ("GTG", 1, True)]
    for start, strand, special in plan:
        length = int(rng.integers(220, 420))
        inner = body(length)
        if special:
            inner = inner[:3 * (SPECIAL_AT - 1)] + "".join(SPECIAL_CODONS) + inner[3 * (SPECIAL_AT - 1):]
        orf = "TAA" + "AGGAGG" + "TAAACC"[:6] + start + inner + ("TAA" if rng.random() < 0.5 else "TAG")
        lead = spacer(int(rng.integers(40, 120)))
        if strand == -1:
            orf = orf.translate(_COMP)[::-1]
            begin, end = n + len(lead) + 1, n + len(lead) + len(orf) - 15
        else:
            begin, end = n + len(lead) + 15 + 1, n + len(lead) + len(orf)
        planted.append((begin, end, strand, start, special))
        parts += [lead, orf]
        n += len(lead) + len(orf)
    parts += [spacer(60), "TAA" + "AGGAGG" + "TAAACC" + "ATG" + body(260)]
    return "".join(parts).encode("ascii"), planted
