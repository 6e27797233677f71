"""The rule of pga_group_proteins (include/pyrodigal_amd.h) restated in plain Python, from the header's text: the string of every gene
record (its residues by tests/tables_ref.translate, its bases by tests/gene_windows_ref.base_class), the groups by a dict, the digest
by Python integers.  A record is (contig, begin, end, strand, partial_begin, partial_end) with 1-based inclusive begin and end, as in
pga_gene; end > length names a gene across the origin of a circular contig."""
import numpy as np

from tests import gene_windows_ref, tables_ref

M = (1 << 61) - 1
B0, B1 = 0x0123456789ABCDEF, 0x1BADB002C0FFEE11


def digest(string):
    """(h under b0, h under b1): h = 1, and h = (h b + r) mod M for every byte r in order."""
    out = []
    for b in (B0, B1):
        h = 1
        for r in bytes(string):
            h = (h * b + r) % M
        out.append(h)
    return tuple(out)


def string_of(seqs, circular, record, unit, tables=None, include_stop=False, strict=True, unknown_residue="X"):
    """The string of one record, as bytes."""
    c, b, e, strand = record[:4]
    pb, pe = (record[4], record[5]) if len(record) > 4 else (0, 0)
    seq, circ = seqs[c], bool(circular[c]) if circular is not None else False
    if unit == "gene":
        return "".join("ACGTN"[gene_windows_ref.base_class(seq, circ, (c, b, e, strand), t)] for t in range(e - b + 1)).encode("ascii")
    assert unit == "protein"
    # (a circular contig is read on at its base 1)
    return tables_ref.translate(seq + seq if circ else seq, b, e, strand, bool(pb), bool(pe), tables[c], include_stop=include_stop,
                                strict=strict, unknown_residue=unknown_residue).encode("ascii")


def groups_of(strings):
    """(group of every string, representatives, sizes): equal strings share a group, a group's representative is its first member,
    and groups are numbered in order of first appearance."""
    number, group, reps, sizes = {}, [], [], []
    for g, s in enumerate(strings):
        u = number.setdefault(bytes(s), len(number))
        if u == len(reps):
            reps.append(g)
            sizes.append(0)
        sizes[u] += 1
        group.append(u)
    return group, reps, sizes


def protein_groups_ref(seqs, circular, records, unit="protein", tables=None, include_stop=False, strict=True, unknown_residue="X"):
    """(group [G], representatives [U], sizes [U], digests [G, 2]) as int64 arrays, and the strings."""
    strings = [string_of(seqs, circular, r, unit, tables, include_stop, strict, unknown_residue) for r in records]
    group, reps, sizes = groups_of(strings)
    digests = np.array([digest(s) for s in strings], np.int64).reshape(len(strings), 2)
    return np.array(group, np.int64), np.array(reps, np.int64), np.array(sizes, np.int64), digests, strings
