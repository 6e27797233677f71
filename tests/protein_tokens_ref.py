"""The rule of pga_translate_genes_tokens (include/pyrodigal_amd.h) restated in numpy, on residue LETTERS: which letters a gene has is
the business of the translation (tests/tables_ref.py on the CPU, Context.translate_genes on the device), not of this file.  Also the
synthetic gene records both token tests use."""
import numpy as np

AMINO_ACIDS = "ACDEFGHIKLMNPQRSTVWY"


def vocab_table(vocabulary, unknown=None, unknown_residue="X"):
    """ids[letter code] for the 128 7-bit letters: the letter's own id, else `unknown`, else the id of `unknown_residue`."""
    given = {ch: k for k, ch in enumerate(vocabulary)} if isinstance(vocabulary, str) else dict(vocabulary)
    rest = unknown if unknown is not None else given[unknown_residue]
    return np.array([given.get(chr(k), rest) for k in range(128)], np.int64)


def protein_tokens_ref(proteins, ids, *, bos=None, eos=None, pad=0, max_length=None, layout="padded", width=None, dtype=np.int64):
    """`proteins`: one str / bytes of residue letters per gene; `ids`: vocab_table().  Returns (tokens, lengths, offsets): tokens is
    [G, width] (width: the longest gene when None) for "padded" and offsets None, or 1-D for "ragged" with gene g at
    tokens[offsets[g]:offsets[g + 1]]."""
    s = (bos is not None) + (eos is not None)
    assert max_length is None or max_length >= s + 1
    rows = []
    for p in proteins:
        r = np.frombuffer(p.encode("ascii") if isinstance(p, str) else bytes(p), np.uint8)
        if max_length is not None:
            r = r[:max_length - s]
        rows.append(([bos] if bos is not None else []) + [int(ids[x]) for x in r] + ([eos] if eos is not None else []))
    lengths = np.array([len(r) for r in rows], np.int64)
    if layout == "ragged":
        offsets = np.zeros(len(rows) + 1, np.int64)
        np.cumsum(lengths, out=offsets[1:])
        return np.array([t for r in rows for t in r], np.int64).astype(dtype), lengths, offsets
    assert layout == "padded"
    w = (int(lengths.max()) if len(rows) else 0) if width is None else width
    out = np.full((len(rows), w), pad, np.int64)
    for g, r in enumerate(rows):
        assert len(r) <= w
        out[g, :len(r)] = r
    return out.astype(dtype), lengths, None


# ---- the synthetic records ---------------------------------------------------------------------------------------------------------
CODON_COUNTS = (0, 1, 2, 3, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 100)
TABLES = (11, 11, 4)
CIRCULAR = (False, True, False)


def synthetic_contigs():
    """About 1 kbp of random ACGTN; a contig to be flagged circular; a contig that is read under table 4."""
    rng = np.random.default_rng(4100)
    draw = lambda n, p: np.frombuffer(b"ACGTN", np.uint8)[rng.choice(5, size=n, p=p)].tobytes()       # noqa: E731
    return [draw(1103, [0.24, 0.24, 0.24, 0.24, 0.04]), draw(701, [0.25, 0.25, 0.25, 0.25, 0.0]), draw(907, [0.2, 0.2, 0.3, 0.3, 0.0])]


def synthetic_records():
    """(contig, begin, end, strand, partial_begin, partial_end), 1-based inclusive, in contig order: every codon count on both strands
    with and without the partial flags on contigs 0 and 2, mixed flags on some, and one gene across the origin of contig 1."""
    lens = [len(s) for s in synthetic_contigs()]
    recs, k = [], 0
    for c in CODON_COUNTS:
        for strand in (1, -1):
            for flags in ((0, 0), (1, 1), (1, 0), (0, 1)):
                if flags[0] != flags[1] and c % 2:
                    continue
                contig = 0 if k % 2 == 0 else 2
                n = max(3 * c + k % 3, 1)                       # bases: c codons and 0 .. 2 more
                begin = 1 + (37 * k) % (lens[contig] - n + 1)
                recs.append((contig, begin, begin + n - 1, strand, flags[0], flags[1]))
                k += 1
    recs.append((1, 650, 650 + 3 * 33 - 1, 1, 0, 0))             # across the origin: ends at base 47
    recs.append((1, 690, 690 + 3 * 20 - 1, -1, 0, 0))
    recs.append((1, 10, 10 + 3 * 12 - 1, 1, 0, 0))
    return sorted(recs, key=lambda r: r[0])


def synthetic_proteins(include_stop=False, strict=True, unknown_residue="X"):
    """The residue letters of the synthetic records by tests/tables_ref.py (a circular contig is read on at its base 1)."""
    from tests import tables_ref
    seqs = synthetic_contigs()
    return [tables_ref.translate(seqs[c] + seqs[c] if CIRCULAR[c] else seqs[c], b, e, st, bool(pb), bool(pe), TABLES[c],
                                 include_stop=include_stop, strict=strict, unknown_residue=unknown_residue)
            for c, b, e, st, pb, pe in synthetic_records()]
