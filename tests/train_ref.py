"""A plain restatement of the training (pyrodigal_amd/csrc/train.inl) over the oracle's node array, with counters.  A helper module,
not a test.

  ref: lib.pyx:5236-5279   (GeneFinder._train)
       lib.pyx:724-768     (Sequence._max_gc_frame_plot), Prodigal node.c record_gc_bias
       lib.pyx:4284-4358   (TrainingInfo._calc_dicodon_gene)
       lib.pyx:4391-4599   (_train_starts_sd), Prodigal node.c determine_sd_usage
       lib.pyx:4601-4827   (_train_starts_nonsd), Prodigal node.c build_coverage_map

Taken from the oracle, because other tests prove them: the digits, the sorted nodes, the path of the training pass of the dynamic
programme (traceb, ipath) and the nodes' coding scores and RBS bins under the half-trained model.  Everything else is restated here,
slowly: the GC frame plot as the windowed sum the device claims it is, the frame bias per node and its ordered sum, the walk of the
path into genes, the hexamer counts, the ten Shine-Dalgarno rounds both as one walk per stop (the device's form) and as the reference's
strand sweep with carried state (asserted equal in every round), the SD decision, the twenty motif rounds with the coverage map, and
the upstream composition.  `log` is math.log, the host's libm, as on both other sides; every sum but the bias sum is a sum of counts.

The counters say which side of every rule an input reaches.  Keys are (name, strand) for what a node decides (strand 1 / -1) and
(name, None) for what a genome decides; tests/test_train_cpu.py asserts them over tests/train_shapes.py before
tests/test_train_shapes_gpu.py compares the device on the same genomes."""
import math
from collections import Counter

import numpy as np

from oracle import oracle as orc

T_STOP = 3
GC_HALF = 60                                     # GC_WINDOW / 2
MT = 4 * 4 * 4096
# byte offsets in struct _training
OFF_GC, OFF_TT, OFF_ST_WT, OFF_BIAS, OFF_TYPE_WT, OFF_USES_SD, OFF_RBS_WT, OFF_UPS, OFF_MOT_WT, OFF_NO_MOT, OFF_GENE_DC = (
    0, 8, 16, 24, 48, 72, 80, 304, 1328, 525616, 525624)
FIELDS = (("gc", OFF_GC, 1), ("st_wt", OFF_ST_WT, 1), ("bias", OFF_BIAS, 3), ("type_wt", OFF_TYPE_WT, 3), ("rbs_wt", OFF_RBS_WT, 28),
          ("ups_comp", OFF_UPS, 128), ("mot_wt", OFF_MOT_WT, MT), ("no_mot", OFF_NO_MOT, 1), ("gene_dc", OFF_GENE_DC, 4096))
assert OFF_GENE_DC + 8 * 4096 == orc.TRAINING_SIZE


# ---- C arithmetic: what Python raises for, C answers with inf and NaN -------------------------------------------------------------

def cdiv(a, b):
    try:
        return a / b                                         # IEEE division, also of inf and NaN
    except ZeroDivisionError:
        with np.errstate(all="ignore"):
            return float(np.float64(a) / np.float64(b))


def cmul(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) * np.float64(b))


def clog(x):
    if x != x:
        return x
    if x == 0.0:
        return -math.inf
    if x < 0.0:
        return math.nan
    return math.log(x) if x != math.inf else x


def clamp(v, lim):
    """`if (v > lim) v = lim; else if (v < -lim) v = -lim`: a NaN passes."""
    return lim if v > lim else (-lim if v < -lim else v)


def max_fr(a, b, c):
    return (0 if a > c else 2) if a > b else (1 if b > c else 2)


def tie_kind(a, b, c):
    """Which of the three totals tie at the maximum: "ab", "ac", "bc", "abc", or None."""
    m = max(a, b, c)
    k = "".join(n for n, v in (("a", a), ("b", b), ("c", c)) if v == m)
    return k if len(k) > 1 else None


def comp(d):
    return d ^ 3 if d <= 3 else 6


# ---- GC frame plot ----------------------------------------------------------------------------------------------------------------

def is_gc(dig):
    d = np.asarray(dig)
    return ((d != 0) & (d != 3)).astype(np.int64)              # unknown bases count as GC


def gc_totals_windowed(dig):
    """tot[i] = sum of gc[i + 3 m] for |m| < 20 inside the sequence: what k_gc_frame says the running sums reduce to."""
    g = is_gc(dig)
    L = len(g)
    tot = np.zeros(L, np.int64)
    for m in range(-(GC_HALF // 3 - 1), GC_HALF // 3):
        lo, hi = max(0, -3 * m), min(L, L - 3 * m)           # the i for which 0 <= i + 3 m < L
        if lo < hi:
            tot[lo:hi] += g[lo + 3 * m:hi + 3 * m]
    return tot


def gc_totals_running(dig):
    """The reference's form (lib.pyx:724-768): running sums per frame from either end, the window cut out by subtraction."""
    g = is_gc(dig).tolist()
    n, half = len(g), GC_HALF
    fwd, bwd, tot = [0] * n, [0] * n, [0] * n
    for i in range(n):
        fwd[i] = (fwd[i - 3] if i >= 3 else 0) + g[i]
        bwd[n - i - 1] = (bwd[n - i + 2] if i >= 3 else 0) + g[n - 1 - i]
    for i in range(n):
        tot[i] = fwd[i] + bwd[i] - g[i]
        if i >= half:
            tot[i] -= fwd[i - half]
        if i + half < n:
            tot[i] -= bwd[i + half]
    return np.asarray(tot, np.int64)


def gc_frame_plot(tot, counters=None):
    L = len(tot)
    gp = np.full(L, -1, np.int64)
    t = tot.tolist()
    for i in range(0, L - 2, 3):
        gp[i] = gp[i + 1] = gp[i + 2] = max_fr(t[i], t[i + 1], t[i + 2])
        if counters is not None:
            k = tie_kind(t[i], t[i + 1], t[i + 2])
            if k:
                counters[("plot_tie_" + k, None)] += 1
    return gp


# ---- inputs -----------------------------------------------------------------------------------------------------------------------

class Inputs:
    """What the restatement takes from the oracle for one genome and one set of options."""

    def __init__(self, seq, tt=11, start_weight=4.35, closed=False, min_gene=90, min_edge_gene=60, max_overlap=60, mask=False):
        p = orc.Params(closed=closed, min_gene=min_gene, min_edge_gene=min_edge_gene, max_overlap=max_overlap)
        o = orc.Oracle(seq, mask=mask)
        self.L, self.gc, self.tt, self.st_wt = o.slen, o.gc, tt, float(start_weight)
        self.dig = o.digits()
        t = orc.Training()
        t.set_gc(self.gc); t.set_trans_table(tt); t._f64(OFF_ST_WT)[0] = self.st_wt
        o.extract(tt, p); o.sort()
        self.n = o.num_nodes
        self.ipath = -1
        if self.n:
            o.record_gc_bias(t)
            o.overlapping_starts(t, flag=0, max_overlap=max_overlap)
            self.ipath = o.dprog(t, final=False)
        nd = o.nodes()
        for k in ("ndx", "stop_val", "strand", "type", "edge", "traceb", "star_ptr"):
            setattr(self, k, nd[k].tolist())
        o.train(p, force_nonsd=False, start_weight=start_weight, tt=tt, upto=3)
        nd2 = o.nodes()
        assert len(nd2) == self.n and np.array_equal(nd2["ndx"], nd["ndx"]) and np.array_equal(nd2["strand"], nd["strand"])
        self.cscore = nd2["cscore"].tolist()
        self.rbs = nd2["rbs"].tolist()


# ---- frame bias -------------------------------------------------------------------------------------------------------------------

def record_gc_bias(I, gp, c):
    """Per start node: how often each codon position is the GC-richest between the start and its stop; then the ordered sum."""
    gpl = gp.tolist()
    score, gbias = [None] * I.n, [0] * I.n
    for i in range(I.n):
        if I.type[i] == T_STOP:
            continue
        fr, st = I.ndx[i] % 3, I.strand[i]
        assert 0 <= I.stop_val[i] < I.L and 0 <= I.ndx[i] < I.L
        if st == 1:                                         # every codon from the stop back to the start
            at = gp[np.arange(I.stop_val[i], I.ndx[i] - 1, -3)]
            ctr = np.bincount((at + 3 - fr) % 3, minlength=3).tolist()
            den = 1.0 * (I.stop_val[i] - I.ndx[i] + 3)
        else:
            at = gp[np.arange(I.stop_val[i], I.ndx[i] + 1, 3)]
            ctr = np.bincount(((3 - at) + fr) % 3, minlength=3).tolist()
            den = 1.0 * (I.ndx[i] - I.stop_val[i] + 3)
        last = I.stop_val[i] if st == 1 else I.ndx[i]
        c[("bias_walk_reaches_last_codon", st)] += int(last >= I.L - 5)
        c[("bias_walk_reads_unset_plot", st)] += int(gpl[I.stop_val[i]] == -1 or gpl[I.ndx[i]] == -1)
        score[i] = [cdiv(3.0 * ctr[q], den) for q in range(3)]
        gbias[i] = max_fr(*ctr)
        k = tie_kind(*ctr)
        if k:
            c[("ctr_tie_" + k, st)] += 1
    b = [0.0, 0.0, 0.0]
    for i in range(I.n):                                    # node order: the one ordered floating-point sum
        if I.type[i] == T_STOP:
            continue
        ln = abs(I.stop_val[i] - I.ndx[i]) + 1
        b[gbias[i]] += (score[i][gbias[i]] * ln) / 1000.0
    tot = b[0] + b[1] + b[2]
    return [cmul(b[q], cdiv(3.0, tot)) for q in range(3)]


# ---- hexamers ---------------------------------------------------------------------------------------------------------------------

def mer(dig, L, i, ln, strand):
    v = 0
    if strand == 1:
        for j in range(ln):
            v |= (dig[i + j] & 3) << (2 * j)
    else:
        k = L - 1 - i
        for j in range(ln):
            v |= (comp(dig[k - j]) & 3) << (2 * j)
    return v


def path_genes(I, c):
    """(left, right, strand) in strand-local coordinates of the genes of the path, walked from its end."""
    genes, in_gene, left, right = [], 0, -1, -1
    p = I.ipath
    while p != -1:
        if I.strand[p] == 1:
            if I.type[p] == T_STOP:
                in_gene, right = 1, I.ndx[p] + 2
            elif in_gene == 1:
                genes.append((I.ndx[p], right, 1)); in_gene = 0
        else:
            if I.type[p] != T_STOP:
                in_gene, left = -1, I.L - I.ndx[p] - 1
            elif in_gene == -1:
                genes.append((left, I.L - I.ndx[p] + 1, -1)); in_gene = 0
        p = I.traceb[p]
    for left, right, st in genes:
        c[("gene_ends_within_5_of_the_downstream_end", st)] += int(right >= I.L - 5)
        c[("gene_starts_within_5_of_the_upstream_end", st)] += int(left <= 5)
    c[("path_without_genes", None)] += int(not genes)
    c[("path_with_genes", None)] += int(bool(genes))
    abutting_starts(I, c)
    return genes


def abutting_starts(I, c):
    """A start codon that abuts the stop codon before it in its frame: what k_ovl_starts0 would add to that stop's starts if its
    `me + 2` / `me - 2` lay one base further out.  Counted also where that stop has a start of another frame among its starts: there
    the connection from a stop of the other strand looks through the slots, and one start too many changes its score."""
    stops = {(I.ndx[i], I.strand[i]): i for i in range(I.n) if I.type[i] == T_STOP and not I.edge[i]}
    for j in range(I.n):
        st = I.strand[j]
        s = stops.get((I.ndx[j] - 3 * st, st))
        if I.type[j] == T_STOP or s is None:
            continue
        c[("start_abuts_the_stop_before_it", st)] += 1
        c[("start_abuts_a_stop_that_has_overlapping_starts", st)] += int(any(q != -1 for q in I.star_ptr[s]))


def gene_dc(I, genes):
    d, L = I.dig.tolist(), I.L
    gc_ = [0] * 4096
    # every window of both strands: the word at p read forwards, and read backwards in complement (the reverse strand's word there)
    a = np.asarray(I.dig, np.int64)
    ca = np.where(a <= 3, a ^ 3, 6)
    nw = max(L - 5, 0)
    fw, rv = np.zeros(nw, np.int64), np.zeros(nw, np.int64)
    for j in range(6):
        fw |= (a[j:j + nw] & 3) << (2 * j)
        rv |= (ca[5 - j:5 - j + nw] & 3) << (2 * j)
    bg = (np.bincount(fw, minlength=4096) + np.bincount(rv, minlength=4096)).tolist()
    for i in (0, L - 6):
        if 0 <= i < nw:
            assert fw[i] == mer(d, L, i, 6, 1) and rv[i] == mer(d, L, L - 6 - i, 6, -1)
    for left, right, st in genes:
        for i in range(left, right - 5, 3):
            gc_[mer(d, L, i, 6, st)] += 1
    glob_bg, glob = sum(bg), sum(gc_)
    out = [0.0] * 4096
    for i in range(4096):
        b, p = cdiv(float(bg[i]), float(glob_bg)), cdiv(float(gc_[i]), float(glob))
        if p == 0 and b != 0:
            v = -5.0
        elif b == 0:
            v = 0.0
        else:
            v = clog(cdiv(p, b))
        out[i] = clamp(v, 5.0)
    return out


# ---- start training: shared pieces ------------------------------------------------------------------------------------------------

def pick_rbs(w, r0, r1, c=None, strand=None):
    w0, w1 = w[r0], w[r1]
    if c is not None:
        c[("pick_rbs_weights_exactly_one_apart", strand)] += int(w0 == w1 + 1.0 or w0 == w1 - 1.0)
    if w0 > w1 + 1.0:
        ex, r = "pick_rbs_w0_above", r0
    elif r1 == 0:
        ex, r = "pick_rbs_r1_zero", r0
    elif w0 < w1 - 1.0:
        ex, r = "pick_rbs_w0_below", r1
    elif r0 == 0:
        ex, r = "pick_rbs_r0_zero", r1
    else:
        ex, r = "pick_rbs_larger_bin", max(r0, r1)
    if c is not None:
        c[(ex, strand)] += 1
    return r


def log_odds(real, bgv, nq, c, name):
    s = 0.0
    for j in range(nq):
        s += float(real[j])
    c[(name + "_sum_zero", None)] += int(s == 0.0)
    c[(name + "_sum_nonzero", None)] += int(s != 0.0)
    if s == 0.0:
        return [0.0] * nq
    out = []
    for j in range(nq):
        r = float(real[j]) / s
        out.append(clamp(clog(cdiv(r, bgv[j])) if bgv[j] != 0 else -4.0, 4.0))
    return out


def count_upstream(I, d, pos, strand, ups, c):
    k = 0
    for lo, hi in ((1, 3), (15, 45)):
        cut = 0
        for j in range(lo, hi):
            if strand == 1:
                if pos >= j:
                    ups[k][d[pos - j] & 3] += 1
                else:
                    cut += 1
            else:
                if pos + j < I.L:
                    ups[k][comp(d[pos + j]) & 3] += 1
                else:
                    cut += 1
            k += 1
        c[("ups_window_%d_cut_%d" % (lo, cut), strand)] += 1


def walk_of_a_stop(ndx, stop_val, strand, type_, s, lo, n):
    """The nodes that k_ts_best weighs for the stop node s, in the order it meets them: away from the stop over the nodes [lo, n), to
    the other end of the ORF or to the next stop of its strand and frame, and the index at which the walk ended (outside [lo, n) if
    it ran out of nodes).  Edge starts are among them; the caller passes them over."""
    st, ph, sv = strand[s], ndx[s] % 3, stop_val[s]
    step = -1 if st == 1 else 1
    out = []
    j = s + step
    while lo <= j < n:
        if (ndx[j] <= sv) if st == 1 else (ndx[j] >= sv):
            break
        if strand[j] == st and ndx[j] % 3 == ph:
            if type_[j] == T_STOP:
                break
            out.append(j)
        j += step
    return out, j


def best_by_walk(I, value, sthresh, c):
    """The device's form: one walk per stop node, away from the stop, over the non-edge starts of its ORF.  Among equal best starts
    the one met first stays.  Returns [(stop, best start, extra)] of the confident ORFs, in node order of the stops."""
    out = []
    for s in range(I.n):
        if I.type[s] != T_STOP:
            continue
        st = I.strand[s]
        best, bndx, bex = 0.0, -1, None
        for j in walk_of_a_stop(I.ndx, I.stop_val, I.strand, I.type, s, 0, I.n)[0]:
            if I.edge[j]:
                continue
            v, ex = value(j)
            if bndx == -1:
                c[("first_start_taken_at_zero_or_above", st)] += int(v >= 0.0)
                c[("first_start_refused_below_zero", st)] += int(v < 0.0)
                c[("first_start_exactly_zero", st)] += int(v == 0.0)
                take = v >= 0.0
            else:
                c[("later_start_replaces_the_best", st)] += int(v > best)
                c[("later_start_equals_the_best", st)] += int(v == best)
                take = v > best
            if take:
                best, bndx, bex = v, j, ex
        if bndx == -1:
            c[("orf_without_a_usable_start", st)] += 1
            continue
        c[("orf_confident", st)] += int(best >= sthresh)
        c[("orf_not_confident", st)] += int(not best >= sthresh)
        c[("orf_best_exactly_at_sthresh", st)] += int(best == sthresh)
        if best >= sthresh:
            out.append((s, bndx, bex))
    return out


def best_by_sweep(I, value, sthresh):
    """The reference's form: one sweep per strand in strand order, one carried best per frame, `>=`."""
    out = []
    for strand in (1, -1):
        best, bndx, bex = [0.0] * 3, [-1] * 3, [None] * 3
        order = range(I.n) if strand == 1 else range(I.n - 1, -1, -1)
        for j in order:
            if I.type[j] != T_STOP and I.edge[j]:
                continue
            if I.strand[j] != strand:
                continue
            ph = I.ndx[j] % 3
            if I.type[j] == T_STOP:
                if best[ph] >= sthresh and bndx[ph] != -1:
                    out.append((j, bndx[ph], bex[ph]))
                best[ph], bndx[ph], bex[ph] = 0.0, -1, None
            else:
                v, ex = value(j)
                if v >= best[ph]:
                    best[ph], bndx[ph], bex[ph] = v, j, ex
    return sorted(out)


def ups_to_log(ups, gc, c):
    out = []
    c[("ups_gc_low", None)] += int(gc <= 0.1)
    c[("ups_gc_high", None)] += int(gc >= 0.9)
    c[("ups_gc_middle", None)] += int(0.1 < gc < 0.9)
    for i in range(32):
        s = 0.0
        row = [float(x) for x in ups[i]]
        for x in row:
            s += x
        band = "low" if gc <= 0.1 else ("high" if gc >= 0.9 else "middle")
        c[("ups_row_zero_" + band, None)] += int(s == 0.0)
        c[("ups_row_nonzero_" + band, None)] += int(s != 0.0)
        if s == 0.0:
            out.append([0.0] * 4); continue
        r = []
        for j in range(4):
            u = row[j] / s
            at = j in (0, 3)
            if gc <= 0.1:
                u = clog(u * 2.0 / (0.90 if at else 0.10))
            elif gc >= 0.9:
                u = clog(u * 2.0 / (0.10 if at else 0.90))
            else:
                u = clog(u * 2.0 / (1.0 - gc)) if at else clog(u * 2.0 / gc)
            if u > 4.0:
                u = 4.0
            if u < -4.0:
                u = -4.0
            r.append(u)
        out.append(r)
    return out


def sd_terms(w):
    """The four terms of determine_sd_usage: uses_sd = not (A or (B and (C or D)))."""
    return (w[0] >= 0.0, w[16] < 1.0 and w[13] < 1.0 and w[15] < 1.0, w[0] >= -0.5, w[22] < 2.0 and w[24] < 2.0 and w[27] < 2.0)


def sd_rule(a, b, cc, d):
    return 0 if (a or (b and (cc or d))) else 1


def determine_sd_usage(w, c):
    t = sd_terms(w)
    uses = sd_rule(*t)
    c[("sd_terms_%d%d%d%d" % tuple(int(x) for x in t), None)] += 1
    for k, name in enumerate("ABCD"):
        flipped = list(t); flipped[k] = not flipped[k]
        c[("sd_term_%s_decides_alone" % name, None)] += int(sd_rule(*flipped) != uses)
    return uses


# ---- the Shine-Dalgarno rounds ----------------------------------------------------------------------------------------------------

def train_starts_sd(I, c, variant=()):
    d = I.dig.tolist()
    wt = I.st_wt
    type_wt, rbs_wt = [0.0] * 3, [0.0] * 28
    tbg = [0.0] * 3
    for i in range(I.n):
        if I.type[i] != T_STOP:
            tbg[I.type[i]] += 1.0
    s = tbg[0] + tbg[1] + tbg[2]
    tbg = [cdiv(x, s) for x in tbg]
    sthresh, halved, kept = 35.0, 0, 0
    ups = None
    for it in range(10):
        rbg = [0.0] * 28
        for j in range(I.n):
            if I.type[j] == T_STOP or I.edge[j]:
                continue
            rbg[pick_rbs(rbs_wt, I.rbs[j][0], I.rbs[j][1], c, I.strand[j])] += 1.0
        s = 0.0
        for x in rbg:
            s += x
        rbg = [cdiv(x, s) for x in rbg]

        def value(j):
            mr = pick_rbs(rbs_wt, I.rbs[j][0], I.rbs[j][1])
            return I.cscore[j] + wt * rbs_wt[mr] + wt * type_wt[I.type[j]], mr
        conf = best_by_walk(I, value, sthresh, c)
        assert sorted(conf) == best_by_sweep(I, value, sthresh), ("SD round", it)
        rreal, treal = [0] * 28, [0] * 3
        ups = [[0] * 4 for _ in range(32)]
        for stop, b, mr in conf:
            rreal[mr] += 1; treal[I.type[b]] += 1
            c[("confident_start_rbs_bin_nonzero", I.strand[b])] += int(mr != 0)
            if it == 9:
                count_upstream(I, d, I.ndx[b], I.strand[b], ups, c)
        rbs_wt = log_odds(rreal, rbg, 28, c, "rbs")
        type_wt = log_odds(treal, tbg, 3, c, "type")
        c[("halves_at_equality", None)] += int(sum(treal) * 2000.0 == I.n)
        c[("keeps_one_node_below_equality", None)] += int(sum(treal) * 2000.0 == I.n + 1)
        if sum(treal) * 2000.0 <= I.n and not ("halving_lt" in variant and sum(treal) * 2000.0 == I.n):
            sthresh /= 2.0; halved += 1
        else:
            kept += 1
    c[("sd_rounds_halve_and_keep", None)] += int(halved > 0 and kept > 0)
    c[("sd_rounds_all_halve", None)] += int(kept == 0)
    return type_wt, rbs_wt, tbg, ups


# ---- the motif rounds -------------------------------------------------------------------------------------------------------------

def spacer_index(j, start, i):
    if j <= start - 16 - i:
        return 3
    if j <= start - 14 - i:
        return 2
    if j >= start - 7 - i:
        return 1
    return 0


def build_coverage_map(real, ng):
    """real, good: [4][4][4096] as arrays of shape (4, 4, 4096)."""
    good = np.zeros((4, 4, 4096), np.int64)
    with np.errstate(all="ignore"):
        hit = (real[0, :, :64] / np.float64(ng)) >= 0.2
    for j in np.flatnonzero(hit.any(axis=0)).tolist():
        good[0, :, j] = 1
    j4, j5, j6 = np.arange(256), np.arange(1024), np.arange(4096)
    for i in range(4):
        g0 = good[0, i]
        if not g0.any():
            continue                                         # nothing frequent enough: every longer word stays 0
        good[1, i, :256] = (g0[(j4 & 252) >> 2] != 0) & (g0[j4 & 63] != 0)
        whole = (g0[(j5 & 1008) >> 4] != 0) & (g0[(j5 & 252) >> 2] != 0) & (g0[j5 & 63] != 0)
        g2 = [0] * 1024
        for j in np.flatnonzero(whole).tolist():             # in table order: a word marked 2 by a neighbour becomes 1 at its own turn
            g2[j] = 1
            tmp = j
            for k in (0, 16):
                tmp ^= k
                for l in (0, 32):
                    tmp ^= l
                    if g2[tmp] == 0:
                        g2[tmp] = 2
        g2 = np.asarray(g2, np.int64)
        good[2, i, :1024] = g2
        a, b = g2[(j6 & 4092) >> 2], g2[j6 & 1023]
        good[3, i] = np.where((a != 0) & (b != 0), np.where((a == 1) & (b == 1), 1, 2), 0)
    return good


def train_starts_nonsd(I, tbg, c, variant=()):
    d, L, wt = I.dig.tolist(), I.L, I.st_wt
    starts = [i for i in range(I.n) if I.type[i] != T_STOP and not I.edge[i]]
    row = {i: r for r, i in enumerate(starts)}
    # every candidate of every start, once: (flat table index, spacer, mer, length) in the order the search meets them
    cand = []
    for i0 in starts:
        st = I.strand[i0]
        start = I.ndx[i0] if st == 1 else L - 1 - I.ndx[i0]
        mine = []
        for i in range(3, -1, -1):
            for j in range(start - 18 - i, start - 5 - i):
                if j < 0:
                    c[("motif_candidate_dropped_len_%d" % (i + 3), st)] += 1
                    continue
                si, m = spacer_index(j, start, i), mer(d, L, j, i + 3, st)
                mine.append(((i * 4 + si) * 4096 + m, start - j - i - 3, m, i + 3, si))
        c[("motif_search_without_candidates", st)] += int(not mine)
        cand.append(mine)
    every = [np.asarray([x[0] - (x[0] // 4096 % 4) * 4096 + k * 4096 for x in mine for k in range(4)], np.int64) for mine in cand]
    width = max([len(m) for m in cand] + [1])
    flat = np.zeros((len(starts), width), np.int64)
    have = np.zeros((len(starts), width), bool)
    for r, mine in enumerate(cand):
        flat[r, :len(mine)] = [x[0] for x in mine]
        have[r, :len(mine)] = True

    mot_wt = np.zeros(MT)
    no_mot, type_wt = 0.0, [0.0] * 3
    sthresh, halved, kept = 35.0, 0, 0
    ups = None
    good = np.zeros((4, 4, 4096), np.int64)
    for it in range(20):
        stage = 0 if it < 4 else (1 if it < 12 else 2)
        assert not np.isnan(mot_wt).any()
        # best motif of every start: the first of the highest weights, -100 where nothing is left of the search
        sc = np.where(have, mot_wt[flat], -100.0)
        pick = sc.argmax(axis=1).tolist() if len(starts) else []
        mot = {}
        for r, i0 in enumerate(starts):
            st = I.strand[i0]
            bsc = float(sc[r, pick[r]]) if cand[r] else -100.0
            if stage == 2 and (bsc == -4.0 or bsc < no_mot + 0.69):
                # (the first term never decides alone: no_mot >= -4, so -4 < no_mot + 0.69; and while no_mot is NaN every weight is 0)
                c[("stage2_falls_back_at_minus_four", st)] += int(bsc == -4.0)
                c[("stage2_falls_back_below_no_mot_alone", st)] += int(bsc != -4.0)
                assert bsc != -4.0 or bsc < no_mot + 0.69
                mot[i0] = (0, 0, 0, 0, no_mot)
            else:
                c[("stage2_keeps_its_motif", st)] += int(stage == 2)
                if cand[r]:
                    _, sp, m, ln, si = cand[r][pick[r]]
                    mot[i0] = (m, ln, si, sp & 15, bsc)
                else:
                    mot[i0] = (0, 0, 0, 0, bsc)

        def update(cnt, i0, real):
            m, ln, si, sp, _ = mot[i0]
            if ln == 0:
                return 1
            st = I.strand[i0]
            start = I.ndx[i0] if st == 1 else L - 1 - I.ndx[i0]
            if stage == 0:                                  # every candidate of the search, under all four spacer classes
                np.add.at(cnt, every[row[i0]], 1)
            elif stage == 1:
                cnt[((ln - 3) * 4 + si) * 4096 + m] += 1
                for i in range(ln - 3):
                    for j in range(start - sp - ln, start - sp - i - 2):
                        if j < 0:
                            c[("stage1_update_skips_before_the_sequence", st)] += 1
                            continue
                        cnt[(i * 4 + spacer_index(j, start, i)) * 4096 + mer(d, L, j, i + 3, st)] += 1
                c[("stage1_update_with_submotifs", st)] += int(ln > 3)
            else:
                cnt[((ln - 3) * 4 + si) * 4096 + m] += 1
            return 0

        mbg = np.zeros(MT)
        zbg = 0.0
        for i0 in starts:
            zbg += update(mbg, i0, False)

        def value(j):
            return I.cscore[j] + wt * mot[j][4] + wt * type_wt[I.type[j]], None
        conf = best_by_walk(I, value, sthresh, c)
        assert sorted(conf) == best_by_sweep(I, value, sthresh), ("motif round", it)
        mreal = np.zeros(MT)
        zreal, ngenes, treal = 0.0, float(len(conf)), [0] * 3
        ups = [[0] * 4 for _ in range(32)]
        for stop, b, _ in conf:
            treal[I.type[b]] += 1
            zreal += update(mreal, b, True)
            if it == 19:
                count_upstream(I, d, I.ndx[b], I.strand[b], ups, c)
        s = float(mbg.sum()) + zbg                       # counts: exact in any order
        with np.errstate(all="ignore"):
            mbg = mbg / np.float64(s)
        zbg = cdiv(zbg, s)
        if stage < 2:
            good = build_coverage_map(mreal.reshape(4, 4, 4096), ngenes)
            for ln in (5, 6):
                used = good[ln - 3].reshape(-1)[mreal.reshape(4, -1)[ln - 3] > 0]
                for v in (0, 1, 2):
                    c[("coverage_%d_at_length_%d" % (v, ln), None)] += int((used == v).sum())
        s = float(mreal.sum()) + zreal
        c[("motif_round_sum_zero", None)] += int(s == 0.0)
        c[("motif_round_sum_nonzero", None)] += int(s != 0.0)
        if s == 0.0:
            mot_wt = np.zeros(MT); no_mot = 0.0
        else:
            gflat = good.reshape(-1)
            for q in np.flatnonzero((gflat == 0) & (mreal != 0)).tolist():     # in table order: zbg is no integer any more
                zreal += mreal[q]; zbg += mreal[q]
            dead = gflat == 0
            mreal[dead] = 0.0; mbg[dead] = 0.0
            mreal = mreal / np.float64(s)
            new = np.full(MT, -4.0)                       # no background, or log(0) clamped
            for q in np.flatnonzero((mbg != 0) & (mreal != 0)).tolist():
                new[q] = clamp(clog(cdiv(mreal[q], mbg[q])), 4.0)
            mot_wt = new
        zreal = cdiv(zreal, s)
        no_mot = clamp(clog(cdiv(zreal, zbg)) if zbg != 0 else -4.0, 4.0)
        c[("no_mot_at_minus_four", None)] += int(no_mot == -4.0)
        type_wt = log_odds(treal, tbg, 3, c, "type")
        c[("halves_at_equality", None)] += int(sum(treal) * 2000.0 == I.n)
        c[("keeps_one_node_below_equality", None)] += int(sum(treal) * 2000.0 == I.n + 1)
        if sum(treal) * 2000.0 <= I.n and not ("halving_lt" in variant and sum(treal) * 2000.0 == I.n):
            sthresh /= 2.0; halved += 1
        else:
            kept += 1
    c[("motif_rounds_halve_and_keep", None)] += int(halved > 0 and kept > 0)
    c[("motif_rounds_all_halve", None)] += int(kept == 0)
    return type_wt, mot_wt, no_mot, ups


# ---- the whole training -----------------------------------------------------------------------------------------------------------

def _blob(I, uses_sd=1, **f):
    b = np.zeros(orc.TRAINING_SIZE, np.uint8)
    b[OFF_GC:OFF_GC + 8].view(np.float64)[0] = I.gc
    b[OFF_TT:OFF_TT + 4].view(np.int32)[0] = I.tt
    b[OFF_ST_WT:OFF_ST_WT + 8].view(np.float64)[0] = I.st_wt
    b[OFF_USES_SD:OFF_USES_SD + 4].view(np.int32)[0] = uses_sd
    for name, off, n in FIELDS:
        if name in f and f[name] is not None:
            b[off:off + 8 * n].view(np.float64)[:] = np.asarray(f[name], np.float64).reshape(-1)
    return b.tobytes()


def train(seq, translation_table=11, start_weight=4.35, force_nonsd=False, closed=False, min_gene=90, min_edge_gene=60, max_overlap=60,
          mask=False, inputs=None, variant=()):
    """({upto: blob} for upto = 1, 2, 3 and 0, populations) of one genome; (None, populations) if it has no node.  `variant` names
    a rule to restate wrongly ("halving_lt": no halving at equality): tests/test_train_cpu.py asserts that the series hold a genome
    whose model it changes, on either strand."""
    c = Counter()
    I = inputs or Inputs(seq, translation_table, start_weight, closed, min_gene, min_edge_gene, max_overlap, mask)
    if I.n == 0:
        c[("genome_without_nodes", None)] += 1
        return None, c
    c[("nodes_at_least_2000", None)] += int(I.n >= 2000)
    c[("nodes_below_2000", None)] += int(I.n < 2000)
    out = {}
    gp = gc_frame_plot(gc_totals_windowed(I.dig), c)
    bias = record_gc_bias(I, gp, c)
    out[1] = _blob(I, bias=bias)
    genes = path_genes(I, c)
    dc = gene_dc(I, genes)
    out[2] = _blob(I, bias=bias, gene_dc=dc)
    type_wt, rbs_wt, tbg, ups = train_starts_sd(I, c, variant)
    uses_sd = determine_sd_usage(rbs_wt, c)
    c[("forced_nonsd_against_the_rule", None)] += int(bool(force_nonsd) and uses_sd == 1)
    if force_nonsd:
        uses_sd = 0
    c[("uses_sd_%d" % uses_sd, None)] += 1
    out[3] = _blob(I, uses_sd, bias=bias, gene_dc=dc, type_wt=type_wt, rbs_wt=rbs_wt, ups_comp=ups_to_log(ups, I.gc, c))
    if uses_sd:
        out[0] = out[3]
    else:
        type_wt, mot_wt, no_mot, ups = train_starts_nonsd(I, tbg, c, variant)
        out[0] = _blob(I, 0, bias=bias, gene_dc=dc, type_wt=type_wt, rbs_wt=rbs_wt, ups_comp=ups_to_log(ups, I.gc, c), mot_wt=mot_wt,
                       no_mot=[no_mot])
    return out, c


def differing_fields(a, b):
    """[] if the blobs are byte-identical; else the names of the fields that differ, with "(nan)" appended where the two sides
    differ only in the sign or payload of NaNs at the same places."""
    if a == b:
        return []
    x, y = np.frombuffer(a, np.uint8), np.frombuffer(b, np.uint8)
    out = []
    for name, off, n in (("trans_table", OFF_TT, 0), ("uses_sd", OFF_USES_SD, 0)) + FIELDS:
        if n == 0:
            if x[off:off + 4].tobytes() != y[off:off + 4].tobytes():
                out.append(name)
            continue
        u, v = x[off:off + 8 * n], y[off:off + 8 * n]
        if u.tobytes() == v.tobytes():
            continue
        fu, fv = u.view(np.float64), v.view(np.float64)
        same = (u.view(np.uint64) == v.view(np.uint64)) | (np.isnan(fu) & np.isnan(fv))
        out.append(name + "(nan)" if same.all() else name)
    return out or ["padding"]
