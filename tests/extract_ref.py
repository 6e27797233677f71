"""Node extraction restated in plain Python with the mask list as an ARGUMENT: sweep_strand and the sort of
oracle/prodigal_oracle.c, line for line.  The C oracle can only mask runs of unknown bases; this restatement takes any sorted,
disjoint list of [begin, end) intervals, so it is the reference for named regions and lower-case runs over KNOWN bases (DESIGN.md 4.9,
tests/test_extract_shapes_gpu.py, tests/test_region_masks_gpu.py).  tests/test_extract_shapes_cpu.py holds it against the C oracle
wherever both apply.  A helper module, not a test; slow (a Python loop over every position): contigs of 12 000 bases or fewer."""
import numpy as np

T_ATG, T_GTG, T_TTG, T_STOP = 0, 1, 2, 3
MAX_LEN = 12000
_COMP = bytes.maketrans(b"ACGTN", b"TGCAN")
_TAA = {1, 2, 3, 4, 5, 9, 10, 11, 12, 13, 15, 16, 21, 22, 23, 24, 25, 26, 32}
_TAG = {1, 2, 3, 4, 5, 9, 10, 11, 12, 13, 14, 21, 23, 24, 25, 26, 33}
_TGA = {1, 6, 11, 12, 15, 16, 22, 23, 26, 29, 30, 32}


def letters(seq):
    """Upper-case ACGT, every other byte as N (po_new)."""
    s = bytes(seq).upper()
    return s.translate(bytes(c if c in b"ACGT" else ord("N") for c in range(256)))


def stop_codons(tt):
    out = set()
    if tt in _TAA: out.add(b"TAA")
    if tt in _TAG: out.add(b"TAG")
    if tt in _TGA: out.add(b"TGA")
    if tt == 2: out |= {b"AGA", b"AGG"}
    if tt == 22: out.add(b"TCA")
    if tt == 23: out.add(b"TTA")
    return out


def start_codons(tt):
    out = {b"ATG"}
    if tt in (6, 10, 14, 15, 16, 2):
        return out
    if tt not in (1, 3, 12):
        out.add(b"GTG")
    if not (tt < 4 or tt == 9 or 21 <= tt < 25):
        out.add(b"TTG")
    return out


def _sweep(s, strand, masks, stops, starts, closed, min_gene, min_edge_gene, out):
    """One right-to-left sweep over the strand's own letters `s`, three frame automata (sweep_strand)."""
    slen, nmask = len(s), len(masks)
    mask = list(masks) + [(0, 0)]                      # the sentinel the reverse walk may step onto
    last, saw, mind, mk = [0] * 3, [0] * 3, [min_edge_gene] * 3, [0] * 3
    for f in range(3):
        fr = (f + slen % 3) % 3
        last[fr] = slen + f
        if not closed:
            while last[fr] + 3 > slen:
                last[fr] -= 3
        mk[f] = (nmask - 1 if strand == 1 else 0) if nmask > 0 else -1

    def push(ndx, typ, stop_val, edge):
        if strand == 1:
            out.append((ndx, stop_val, typ, 1, edge))
        else:
            out.append((slen - ndx - 1, slen - stop_val - 1, typ, -1, edge))

    for i in range(slen - 3, -1, -1):
        fr = i % 3
        cod = s[i:i + 3]
        if cod in stops:
            if saw[fr]:
                edge = int(s[last[fr]:last[fr] + 3] not in stops)
                if strand == 1:
                    out.append((last[fr], i, T_STOP, 1, edge))
                else:
                    out.append((slen - last[fr] - 1, slen - i - 1, T_STOP, -1, edge))
            mind[fr], last[fr], saw[fr] = min_gene, i, 0
            continue
        if last[fr] >= slen:
            continue
        if strand == 1:
            while mk[fr] != -1 and last[fr] < mask[mk[fr]][0]:
                mk[fr] = -1 if mk[fr] == 0 else mk[fr] - 1
            if mk[fr] != -1 and mask[mk[fr]][0] < last[fr] and i < mask[mk[fr]][1]:
                continue
        else:
            while mk[fr] != -1 and slen - last[fr] - 1 > mask[mk[fr]][1]:
                mk[fr] = -1 if mk[fr] == nmask else mk[fr] + 1
            if mk[fr] != -1 and mask[mk[fr]][0] < slen - i - 1 and slen - last[fr] - 1 < mask[mk[fr]][1]:
                continue
        if last[fr] - i + 3 >= mind[fr] and cod in starts:
            saw[fr] = 1
            push(i, T_ATG if cod[0] == 65 else (T_TTG if cod[0] == 84 else T_GTG), last[fr], 0)
        elif i <= 2 and not closed and last[fr] - i > min_edge_gene:
            saw[fr] = 1
            push(i, T_ATG, last[fr], 1)
    for f in range(3):
        if not saw[f]:
            continue
        edge = int(s[last[f]:last[f] + 3] not in stops)
        if strand == 1:
            out.append((last[f], f - 6, T_STOP, 1, edge))
        else:
            out.append((slen - last[f] - 1, slen - f + 5, T_STOP, -1, edge))


def extract_ref(seq, masks=(), tt=11, closed=False, min_gene=90, min_edge_gene=60):
    """(ndx, stop_val, type, strand, edge) of the sorted nodes of `seq` under the mask list `masks` ([begin, end) pairs, sorted and
    disjoint: what pga_result.masks reports)."""
    assert len(seq) <= MAX_LEN, "extract_ref is a Python loop over every position"
    fwd = letters(seq)
    masks = [(int(b), int(e)) for b, e in masks]
    assert all(masks[k][1] < masks[k + 1][0] for k in range(len(masks) - 1)), "the mask list is the merged union"
    out = []
    if len(fwd) >= 3:
        stops, starts = stop_codons(tt), start_codons(tt)
        _sweep(fwd, 1, masks, stops, starts, closed, min_gene, min_edge_gene, out)
        _sweep(fwd.translate(_COMP)[::-1], -1, masks, stops, starts, closed, min_gene, min_edge_gene, out)
    out.sort(key=lambda n: (n[0], -n[3]))              # ndx ascending, the forward strand first (node_order)
    a = np.asarray(out, np.int64).reshape(-1, 5)
    return tuple(a[:, k] for k in range(5))


def union(intervals):
    """Sorted, disjoint, touching intervals joined."""
    out = []
    for b, e in sorted((int(b), int(e)) for b, e in intervals):
        if out and b <= out[-1][1]:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([b, e])
    return [tuple(x) for x in out]
