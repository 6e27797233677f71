"""Gene and contig records that put the device renderer (pyrodigal_amd/csrc/render.hip, render_fmt.h) and the host splice of its
flagged lines (_cabi._splice_fallback) at their edges: the inputs of tests/test_render_shapes_cpu.py, which proves from the records
and the host writers' text what they contain, and of tests/test_render_shapes_gpu.py, which compares the device on them.  A helper
module, not a test.

`Context.render_genes` takes its records from host arrays, so nothing here runs the finder: a case is sequences, models and a
GENE_DTYPE array tiled by a CONTIG_DTYPE array, and `lib._genes_from_records` hands the host writers the same records.  Everything
is deterministic.  The families: numbers, confidence, record bodies, circular, layout, ORIGIN, RBS, flags; and the
contigs of the scores family, whose rows come from the finder's nodes."""
import dataclasses
import datetime
import functools
import io
import math
import warnings

import numpy as np

from oracle import oracle as orc
from pyrodigal_amd import _cabi
from tests.util import golden_path

WRITERS = {"gff": "write_gff", "faa": "write_translations", "fna": "write_genes", "gbk": "write_genbank"}
MARGIN = 1e-9                                     # render_genes' default fallback_margin
MIDPOINTS = (50.005, 62.505, 73.125, 99.985, 99.995)
GBK_DATE = datetime.date(2024, 2, 29)
MODEL = "SRR492066.training.bin.gz"               # st_wt 4.35, table 11, uses_sd
MODEL_TT4 = "models/synth_gc50_tt4.tinf.bin.gz"
HALVES = (0.125, 2.675, 1.005, 0.0005, 0.5, 1.5, 2.5, 0.25, 0.75, 0.05, 0.15, 0.35, 99.995, 99.985, 12.345, 1e-3, 5e-4)
SIGNED_ZEROS = (0.0, -0.0, -1e-300, -5e-324, -0.04, -0.004, -0.0004, -0.049999, -0.0049999, -0.00049999, -0.05, -0.005, -0.0005,
                5e-324, 1e-300, 2.2250738585072014e-308, -2.2250738585072014e-308)
MORE_HALVES = (0.375, -0.375, 0.625, 0.875, -0.875, 99.375,                 # '%.2f' halves that round up
               9.995, math.nextafter(9.995, math.inf), 9.996, -9.996, 0.995, 0.996, 99.996)     # carries: 9.995.. -> 10.00
SCORE_FIELDS = ("cscore", "sscore", "rscore", "uscore", "tscore")
PARTIALS = ((0, 0), (1, 0), (0, 1), (1, 1))       # (partial_begin, partial_end), in sequence orientation


@dataclasses.dataclass(eq=False)
class Case:
    name: str
    seqs: list
    ids: list
    blobs: list                   # the models, as bytes
    moc: np.ndarray               # model_of_contig
    genes: np.ndarray             # GENE_DTYPE
    contigs: np.ndarray           # CONTIG_DTYPE, tiling `genes`
    formats: dict                 # {format: writer options}
    circular: list = None         # one flag per contig, or None: all linear
    meta: bool = False
    descriptions: list = None
    first_seqnum: int = 1
    seqnums: list = None
    built_flagged: bool = False   # holds lines built to be flagged

    def seqnum(self, c):
        return int(self.seqnums[c]) if self.seqnums is not None else self.first_seqnum + c


@dataclasses.dataclass
class Records:
    """What render_genes reads of a find_genes result."""
    contigs: np.ndarray
    genes: np.ndarray


# ---- sequences, models, records -----------------------------------------------------------------------------------------------------------

def make_seq(n, seed, last_block=None):
    """n random bases with runs of N, lower-case stretches and single IUPAC letters: one other letter every 97 bases (97 = 1 mod 3,
    so they fall on every codon position of every frame), five N every 1 500, forty lower-case bases every 700.  `last_block`: the
    last (up to) ten bases are "N", "lower" or "iupac"."""
    rng = np.random.default_rng(seed)
    s = bytearray(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)].tobytes())
    for p in range(700, n, 700):
        s[p:p + 40] = bytes(s[p:p + 40]).lower()
    for k, p in enumerate(range(31, n, 97)):
        s[p] = b"RYKMSWBDHVN"[k % 11]
    for p in range(211, n, 1500):
        s[p:p + 5] = b"N" * len(s[p:p + 5])
    if last_block:
        lo = 10 * ((n - 1) // 10)
        tail = {"N": b"N" * 10, "lower": bytes(s[lo:]).lower().replace(b"n", b"a"), "iupac": b"RYKMSWBDHV"}[last_block]
        s[lo:] = tail[:n - lo]
    assert len(s) == n
    return bytes(s)


@functools.lru_cache(maxsize=None)
def base_model():
    return orc.Training.load(golden_path(MODEL))


@functools.lru_cache(maxsize=None)
def tt4_model():
    t = orc.Training.load(golden_path(MODEL_TT4))
    assert t.trans_table == 4
    return t


def rbs_model(uses_sd, no_mot, st_wt=None):
    """The fixture model with rounded RBS weights (so that different bins tie: r1 == r2), `uses_sd` and `no_mot` as given."""
    t = base_model().copy()
    t.rbs_wt[:] = np.round(t.rbs_wt)
    t._i32(72)[0] = uses_sd
    t._f64(525616)[0] = no_mot
    if st_wt is not None:
        t._f64(16)[0] = st_wt
    return t


def rec(begin, end, strand=1, partial=(0, 0), **fields):
    d = dict(begin=begin, end=end, strand=strand, partial_begin=partial[0], partial_end=partial[1], cscore=12.5, sscore=3.25, gc_cont=0.5)
    d.update(fields)
    return d


def tile(per_contig, moc):
    """(genes, contigs): the records of every contig back to back, and the contig records that tile them."""
    genes = np.zeros(sum(len(g) for g in per_contig), _cabi.GENE_DTYPE)
    contigs = np.zeros(len(per_contig), _cabi.CONTIG_DTYPE)
    k = 0
    for c, recs in enumerate(per_contig):
        contigs[c]["gene_begin"], contigs[c]["n_genes"], contigs[c]["model"] = k, len(recs), moc[c]
        for r in recs:
            genes[k]["contig"] = c
            for name, v in r.items():
                genes[k][name] = v
            k += 1
    return genes, contigs


def make_case(name, seqs, per_contig, formats, blobs=None, moc=None, ids=None, **kw):
    nc = len(seqs)
    blobs = [base_model().tobytes()] if blobs is None else [b if isinstance(b, bytes) else b.tobytes() for b in blobs]
    moc = np.zeros(nc, np.int32) if moc is None else np.ascontiguousarray(moc, np.int32)
    genes, contigs = tile(per_contig, moc)
    fm = {f: dict(o) for f, o in formats.items()}
    if "gbk" in fm:
        fm["gbk"].setdefault("date", GBK_DATE)
    return Case(name, list(seqs), ["ctg%d" % c for c in range(nc)] if ids is None else list(ids), blobs, moc, genes, contigs, fm, **kw)


# ---- the host's text and the rule of the flags -------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def host_text(case, fmt):
    """(per contig, joined): the bytes the host writers write for the case's records."""
    from pyrodigal_amd import lib
    tinfs = [lib.TrainingInfo(raw=b) for b in case.blobs]
    out = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # a translation table with other stop codons warns on the host
        for c, seq in enumerate(case.seqs):
            m = int(case.moc[c])
            lo = int(case.contigs["gene_begin"][c]); hi = lo + int(case.contigs["n_genes"][c])
            circ = bool(case.circular is not None and case.circular[c])
            g = lib._genes_from_records(seq, case.genes[lo:hi].tobytes(), tinfs[m], case.seqnum(c), meta=case.meta,
                                        metagenomic_bin=lib.MetagenomicBin(tinfs[m], case.descriptions[m]) if case.meta else None,
                                        circular=circ, cut=0 if circ else None)
            f = io.StringIO()
            getattr(g, WRITERS[fmt])(f, case.ids[c], **case.formats[fmt])
            out.append(f.getvalue().encode("utf-8"))
    return tuple(out), b"".join(out)


def unprintable(x):
    """A value the exact printer does not cover: non-finite, or at least 2^53 in magnitude."""
    x = float(x)
    return not math.isfinite(x) or abs(x) >= 2.0 ** 53


def confidence(score, st_wt):
    """(r, conf) as Gene.confidence computes it."""
    r = score / st_wt
    if r < 41:
        e = math.exp(r)
        conf = (e / (e + 1)) * 100.0
    else:
        conf = 99.99
    return r, max(conf, 50.0)


def midpoint_distance(conf):
    """|frac(conf * 100) - 0.5|: how far conf is from a rounding midpoint of '%.2f', in hundredths."""
    t = conf * 100.0
    return abs(t - math.floor(t) - 0.5)


def expected_flags(case, fmt, margin=MARGIN):
    """The gene indices whose line (GFF) or record header (FASTA) the device must leave to the host."""
    out = []
    st_of = [orc.Training(b).st_wt for b in case.blobs]
    G = case.genes
    cols = [G[name].astype(np.float64).tolist() for name in ("gc_cont",) + SCORE_FIELDS]
    contig = G["contig"].tolist()
    for k, (gc, cs, ss, rs, us, ts) in enumerate(zip(*cols)):
        bad = unprintable(gc)
        if fmt == "gff" and not bad:
            bad = any(unprintable(x) for x in (ss + cs, cs, ss, rs, us, ts))
            if not bad:
                r, conf = confidence(cs + ss, st_of[int(case.moc[contig[k]])])
                bad = r < 41 and conf != 50.0 and midpoint_distance(conf) < margin * 100
        if bad:
            out.append(k)
    return out


# ---- number family -----------------------------------------------------------------------------------------------------------------------

def number_values():
    """The values of tests/test_render_format_cpu.py's hand lists, 20 000 doubles of its random generator, the edges of the exact path."""
    xs = []
    for h in HALVES:
        for v in (h, -h):
            xs += [v, math.nextafter(v, math.inf), math.nextafter(v, -math.inf)]
    xs += list(SIGNED_ZEROS) + list(MORE_HALVES)
    rng = np.random.default_rng(1002)
    n = 20_000
    mant = rng.random(n) + 1.0
    ex = rng.integers(-30, 21, n)
    xs += (np.ldexp(mant, ex) * np.where(rng.random(n) < 0.5, -1.0, 1.0)).tolist()
    return xs + [2.0 ** 53 - 1, 2.0 ** 53, math.inf, -math.inf, math.nan]


SUM_PAIRS = ((0.1, 0.2), (7.25, -7.25), (0.5, 0.25), (-0.5, -0.25), (9.5, 0.45), (9.5, 0.46), (-0.0, -0.0), (0.0, -0.0), (0.1, 0.15), (0.2, 0.15), (0.125, 0.125), (-0.3, 0.05),
             (1e16, 1.0), (1e308, 1e308), (2.0 ** 52, 2.0 ** 52))           # (sscore, cscore); the last two sums are flagged


def gc_values():
    """float32: the nearest to every k / 1000 and its two neighbours, the exact binary halves of '%.3f', inf and nan."""
    grid = (np.arange(1001) / 1000.0).astype(np.float32)
    halves = (np.arange(1, 16, 2) / 16.0).astype(np.float32)
    xs = np.concatenate([grid, np.nextafter(grid, np.float32(2)), np.nextafter(grid, np.float32(-1)), halves,
                         np.array([0.0005 + 2.0 ** -11, 1.5, 3.0e38], np.float32)])
    return np.concatenate([xs, np.array([np.inf, -np.inf, np.nan], np.float32)])


@functools.lru_cache(maxsize=None)
def number_cases():
    seq = make_seq(400, 11)
    xs = number_values()
    cases = []
    for field in SCORE_FIELDS:
        recs = [rec(1 + k % 390, 6 + k % 390, 1 if k % 2 else -1, **{field: x}) for k, x in enumerate(xs)]
        cases.append(make_case("numbers_" + field, [seq], [recs], {"gff": {}}, built_flagged=True))
    recs = [rec(3 + k, 11 + k, 1 if k % 2 else -1, sscore=s, cscore=c) for k, (s, c) in enumerate(SUM_PAIRS)]
    cases.append(make_case("numbers_sums", [seq], [recs], {"gff": {}}, built_flagged=True))
    recs = [rec(1 + k % 390, 6 + k % 390, 1 if k % 2 else -1, gc_cont=x) for k, x in enumerate(gc_values())]
    cases.append(make_case("numbers_gc", [seq], [recs], {"gff": {}, "faa": {}, "fna": {}}, built_flagged=True))
    return tuple(cases)


# ---- confidence family -------------------------------------------------------------------------------------------------------------------

def score_at_41(st):
    """The smallest score whose r = score / st is not below 41."""
    s = 41 * st
    while s / st >= 41:
        s = math.nextafter(s, -math.inf)
    while s / st < 41:
        s = math.nextafter(s, math.inf)
    return s


def score_near(mid, st):
    """The score whose confidence lies nearest to `mid`, among the doubles around st * logit(mid / 100)."""
    p = mid / 100.0
    s0 = st * math.log(p / (1 - p))
    lo = s0
    for _ in range(300):
        lo = math.nextafter(lo, -math.inf)
    best, s = None, lo
    for _ in range(600):
        d = abs(confidence(s, st)[1] - mid)
        if best is None or d < best[0]:
            best = (d, s)
        s = math.nextafter(s, math.inf)
    return best[1]


@functools.lru_cache(maxsize=None)
def confidence_scores():
    """{name: score} under the fixture model's start weight."""
    st = base_model().st_wt
    at = score_at_41(st)
    out = {"at_41": at, "below_41": math.nextafter(at, -math.inf), "zero": 0.0, "tiny": 1e-300, "small": 1e-9, "huge_negative": -1e308,
           "inf": math.inf, "-inf": -math.inf, "nan": math.nan}
    for mid in MIDPOINTS:
        out["on_%s" % mid] = score_near(mid, st)
        out["off_%s" % mid] = score_near(mid + 0.002, st)
    return out


@functools.lru_cache(maxsize=None)
def confidence_case():
    seq = make_seq(400, 12)
    recs = []
    for k, (name, s) in enumerate(confidence_scores().items()):
        for strand in (1, -1):
            recs.append(rec(2 + k, 13 + k, strand, cscore=s, sscore=0.0))
    return make_case("confidence", [seq], [recs], {"gff": {}}, built_flagged=True)


# ---- record-body family ------------------------------------------------------------------------------------------------------------------

BODY_WIDTHS = (1, 2, 59, 60, 63, 64, 65, 70, 128, 13_001)
BODY_LEN = 13_000
GBK_BODIES = (0, 43, 44, 45, 48, 49, 50, 103, 104)         # 15 + L = 15, 58, 59, 60, 63, 64, 65, 118, 119


def body_targets(w):
    """The letter counts a record body must hit at width w."""
    t = {0, 1, w - 1, w, w + 1, 2 * w, 63, 64, 65, 127, 128, 129}
    if w <= 128:
        t.add(math.lcm(64, w))
    return sorted(x for x in t if 0 <= x and 3 * x + 5 <= BODY_LEN)


def body_records(slen, lengths, seed):
    """For every interval length: the four partial-flag combinations on both strands, at begins that walk through the contig; then
    genes with begin = 1, end = slen, and both."""
    recs, k = [], seed
    for n in sorted(set(lengths)):
        if not 1 <= n <= slen:
            continue
        for strand in (1, -1):
            for partial in PARTIALS:
                b = 1 + (k * 101) % (slen - n + 1)
                recs.append(rec(b, b + n - 1, strand, partial, start_type=k % 4))
                k += 1
    for strand in (1, -1):
        for n in (1, 2, 3, 7, 64):
            recs.append(rec(1, n, strand, PARTIALS[n % 4]))
            recs.append(rec(slen - n + 1, slen, strand, PARTIALS[(n + 1) % 4]))
        recs.append(rec(1, slen, strand))
    return recs


def interval_lengths(targets):
    """Interval lengths whose gene FASTA body (n letters) and protein body (n / 3 letters, one fewer without its stop) hit the targets,
    with every n mod 3."""
    ns = {1, 2, 3, 4, 5, 6, 7, 8}
    for L in targets:
        ns |= {L} | {3 * L + r for r in range(3)} | {3 * (L + 1) + r for r in range(3)}
    return ns


@functools.lru_cache(maxsize=None)
def body_cases():
    seqs = [make_seq(BODY_LEN, 21), make_seq(700, 22)]
    blobs = [base_model(), tt4_model()]
    cases = []
    for i, w in enumerate(BODY_WIDTHS):
        for include_stop in (True, False):
            big = body_records(BODY_LEN, interval_lengths(body_targets(w)), 3 * i)
            small = body_records(700, interval_lengths([0, 1, 2, 20, 63, 64, 65]), 5 * i)
            faa = {"width": w, "include_stop": include_stop, "strict_translation": bool((i + include_stop) % 2),
                   "translation_table": (None, 4, 11)[i % 3]}
            cases.append(make_case("body_w%d_stop%d" % (w, include_stop), seqs, [big, small], {"faa": faa, "fna": {"width": w}},
                                   blobs=blobs, moc=[0, 1]))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def gbk_body_cases():
    seqs = [make_seq(1_000, 23), make_seq(700, 24)]
    blobs = [base_model(), tt4_model()]
    ns = {1, 2, 3, 4, 5, 6}
    for b in GBK_BODIES:
        ns |= {3 * b + r for r in range(3)} | {3 * (b + 1) + r for r in range(3)}
    cases = []
    for i, (strict, tt) in enumerate(((True, None), (False, None), (True, 4), (False, 11))):
        per = [body_records(1_000, ns, i), body_records(700, ns, i + 7)]
        cases.append(make_case("gbk_body_strict%d_tt%s" % (strict, tt), seqs, per,
                               {"gbk": {"strict_translation": strict, "translation_table": tt}, "gff": {}}, blobs=blobs, moc=[0, 1]))
    return tuple(cases)


# ---- circular family ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def circular_case():
    """A circular contig with genes across its origin, beside a linear one."""
    seqs = [make_seq(601, 31), make_seq(700, 32)]
    n = len(seqs[0])
    recs = []
    for strand in (1, -1):
        for partial in (PARTIALS[0], PARTIALS[3]):
            recs += [rec(n, n + k, strand, partial) for k in (1, 2, 3)]                 # begin = len
            recs += [rec(n - 8 + ph, n - 8 + ph + 29, strand, partial) for ph in range(3)]   # a codon across the origin, every phase
            recs += [rec(2, n + 1, strand, partial), rec(n, 2 * n - 1, strand, partial)]     # the longest wrap: end - begin = len - 1
            recs += [rec(1, n, strand, partial), rec(n - 100, n, strand, partial), rec(5, 300, strand, partial)]
    linear = body_records(700, (1, 3, 30, 64), 1)
    fm = {"gff": {}, "faa": {"width": 7}, "fna": {"width": 64}}
    return make_case("circular", seqs, [recs, linear], fm, circular=[1, 0])


# ---- layout family -----------------------------------------------------------------------------------------------------------------------

def small_records(slen, count, seed=0):
    return [rec(1 + (7 * (k + seed)) % (slen - 12), 1 + (7 * (k + seed)) % (slen - 12) + 1 + k % 12, 1 if k % 3 else -1, PARTIALS[k % 4],
                start_type=k % 4) for k in range(count)]


ID_CHARS = ("x", "é", "€", "\U0001f9ec")           # 1, 2, 3 and 4 bytes in UTF-8
ALL_FORMATS = {"gff": {}, "faa": {}, "fna": {}, "gbk": {}}


@functools.lru_cache(maxsize=None)
def layout_cases():
    cases = []
    seqs6 = [make_seq(400 + 13 * c, 40 + c) for c in range(6)]
    for counts in ([0, 3, 0, 0, 1, 0], [0] * 6):
        cases.append(make_case("layout_counts_%s" % "".join(map(str, counts)), seqs6, [small_records(400, k, c) for c, k in enumerate(counts)],
                               ALL_FORMATS))
    # unit counts of 255, 256 and 257: contigs + genes (GFF) and 2 contigs + genes (GenBank), with empty contigs in between
    for total in (243, 244, 245, 249, 250, 251):
        counts = [0, 100, 0, 0, total - 101, 1]
        cases.append(make_case("layout_units_%d" % total, seqs6, [small_records(400, k, c) for c, k in enumerate(counts)], ALL_FORMATS))
    # four-digit gene indices
    one = [rec(1 + k % 400, 1 + k % 400, 1 if k % 2 else -1) for k in range(1001)]
    cases.append(make_case("layout_1001_genes", [seqs6[0], seqs6[1]], [small_records(400, 2), one], ALL_FORMATS))
    # sequence numbers
    four = [seqs6[c] for c in range(4)]
    per4 = [small_records(400, 3, c) for c in range(4)]
    off_id = {"gff": {"full_id": False}, "faa": {"full_id": False}, "fna": {"full_id": False}, "gbk": {}}
    cases.append(make_case("layout_first_seqnum", four, per4, off_id, first_seqnum=999_999_999))
    cases.append(make_case("layout_seqnums", four, per4, off_id, seqnums=[0, 7, 2 ** 40, -3]))
    # ids: empty, and 22, 23 and 24 code points of 1 to 4 bytes each (LOCUS pads to 23 code points)
    ids = [""] + [("id" + ch * n)[-n:] if ch == "x" else "i" + ch * (n - 1) for ch in ID_CHARS for n in (22, 23, 24)]
    seqs = [make_seq(400 + c, 60 + c) for c in range(len(ids))]
    per = [small_records(400, 2, c) for c in range(len(ids))]
    on_id = {"gff": {"full_id": True}, "faa": {"full_id": True}, "fna": {"full_id": True}, "gbk": {}}
    cases.append(make_case("layout_ids_full", seqs, per, on_id, ids=ids))
    cases.append(make_case("layout_ids_seqnum", seqs, per, off_id, ids=ids))
    # writer options
    cases.append(make_case("layout_gff_options", four, per4, {"gff": {"header": False, "include_translation_table": True, "version_separator": "-"}}))
    cases.append(make_case("layout_gff_tt", four, per4, {"gff": {"include_translation_table": True}}, blobs=[base_model(), tt4_model()], moc=[0, 1, 1, 0]))
    # positions of one to six digits
    n = 100_001
    ends = (1, 9, 10, 99, 100, 999, 1000, 9999, 10_000, 99_999, 100_000, 100_001)
    recs = [rec(max(1, e - k % 5), e, 1 if k % 2 else -1) for k, e in enumerate(ends)] + [rec(e, min(n, e + 31), -1 if k % 2 else 1) for k, e in enumerate(ends)]
    cases.append(make_case("layout_positions", [make_seq(n, 70)], [recs], {"gff": {}, "fna": {"width": 70}}))
    return tuple(cases)


# ---- ORIGIN family -----------------------------------------------------------------------------------------------------------------------

ORIGIN_LENGTHS = (1, 9, 10, 11, 59, 60, 61, 119, 120, 121, 20_479, 20_480, 20_481, 40_960, 40_961)


@functools.lru_cache(maxsize=None)
def origin_case():
    seqs = [make_seq(n, 80 + k, ("N", "lower", "iupac")[k % 3]) for k, n in enumerate(ORIGIN_LENGTHS)]
    return make_case("origin", seqs, [[] for _ in seqs], {"gbk": {}})


# ---- RBS family --------------------------------------------------------------------------------------------------------------------------

def beside(x, st, up):
    """The double nearest to x on the given side whose product with st differs from x * st."""
    y = x
    while y * st == x * st:
        y = math.nextafter(y, math.inf if up else -math.inf)
    return y


def rbs_site(t, k0, k1, mot_score):
    """Gene._rbs' four-way rule, restated: (branch, the site whose motif prints or -1)."""
    st = t.st_wt
    r1, r2, ms = float(t.rbs_wt[k0]) * st, float(t.rbs_wt[k1]) * st, mot_score * st
    if t.uses_sd:
        return ("sd_first" if r1 > r2 else "sd_second"), (k0 if r1 > r2 else k1)
    if t.no_mot > -0.5 and r1 > r2 and r1 > ms:
        return "first", k0
    if t.no_mot > -0.5 and r2 >= r1 and r2 > ms:
        return "second", k1
    return "motif", -1


@functools.lru_cache(maxsize=None)
def rbs_models():
    return (base_model(), rbs_model(1, -0.4), rbs_model(0, -0.4), rbs_model(0, -0.5), rbs_model(0, -0.6),
            rbs_model(0, math.nextafter(-0.5, 0.0)), rbs_model(0, -0.4, st_wt=-4.35))


def rbs_records(t, slen, seed):
    st, w = t.st_wt, t.rbs_wt
    pairs = [(k, 0) for k in range(28)] + [(0, k) for k in range(28)] + [(k, 27 - k) for k in range(28)] + [(k, k) for k in range(0, 28, 5)]
    ties = [(a, b) for a in range(28) for b in range(a + 1, 28) if w[a] == w[b]][:6]
    pairs += ties + [(b, a) for a, b in ties]
    recs = []
    motifs = ((0, 0, 0), (3, 0b100111, 0), (4, -1, 255), (5, 0x3ff, 7), (6, -0x7fffffff - 1, 15), (16, 0x7fffffff, 3), (17, -2, 254), (17, -1, 1))
    k = seed
    for k0, k1 in pairs:
        r1, r2 = float(w[k0]), float(w[k1])
        scores = {-100.0, 100.0, r1, r2, beside(r1, st, True), beside(r1, st, False), beside(r2, st, True), beside(r2, st, False)}
        for ms in sorted(scores):
            mot_len, mot_ndx, mot_spacer = motifs[k % len(motifs)]
            b = 1 + (13 * k) % (slen - 40)
            recs.append(rec(b, b + 5 + k % 30, 1 if (k // 3) % 2 else -1, start_type=k % 4, rbs=(k0, k1), mot_score=ms, mot_len=mot_len,
                            mot_ndx=mot_ndx, mot_spacer=mot_spacer))
            k += 1
    return recs


@functools.lru_cache(maxsize=None)
def rbs_cases():
    models = rbs_models()
    seqs = [make_seq(450 + c, 90 + c) for c in range(len(models))]
    per = [rbs_records(t, 450, 3 * c) for c, t in enumerate(models)]
    fm = {"gff": {}, "faa": {}, "fna": {}}
    single = make_case("rbs_models", seqs, per, fm, blobs=models, moc=list(range(len(models))))
    meta = make_case("rbs_meta", seqs, per, fm, blobs=models, moc=list(range(len(models))), meta=True,
                     descriptions=["", "bin one", "Café 7", "x" * 80, "5|tt11", 'q"uote', "last"])
    return single, meta


# ---- flag and splice family --------------------------------------------------------------------------------------------------------------

LONGER = (1e300, -1e300, 2.0 ** 53)            # the host prints more characters than the device's guess ("0.00")
SHORTER_SCORE = (math.inf, math.nan)           # ... fewer than "0.00"
SHORTER_GC = (math.inf, -math.inf, math.nan)   # ... fewer than "0.000" / "-0.000"
LONGER_GC = (3.0e38, -3.0e38, 2.0 ** 53)


def flag_layout(bad):
    """Gene lists of nine contigs: `bad(k)` gives the k-th flagged record.  Flagged records as the first and the last of a contig,
    several in a row, alone, and in contigs that follow one and several contigs without genes."""
    ok = lambda k: rec(5 + k, 16 + k, 1 if k % 2 else -1)      # noqa: E731
    it = iter(range(100))
    B = lambda: bad(next(it))                                    # noqa: E731
    return [[ok(0), ok(1)], [B(), ok(2), ok(3), B()], [], [B()], [], [], [B(), B(), B(), ok(4)], [ok(5), B(), B(), ok(6), B()], []]


@functools.lru_cache(maxsize=None)
def flag_cases():
    seqs = [make_seq(400 + 3 * c, 100 + c) for c in range(9)]
    cases = []
    for name, vals in (("longer", LONGER), ("shorter", SHORTER_SCORE), ("mixed", LONGER + SHORTER_SCORE)):
        def bad(k, vals=vals):
            return rec(7 + k, 40 + k, -1 if k % 2 else 1, **{SCORE_FIELDS[k % 5]: vals[k % len(vals)]})
        cases.append(make_case("flags_gff_" + name, seqs, flag_layout(bad), {"gff": {}}, built_flagged=True))
    for name, vals in (("longer", LONGER_GC), ("shorter", SHORTER_GC), ("mixed", LONGER_GC + SHORTER_GC)):
        def bad(k, vals=vals):
            return rec(7 + k, 40 + k, -1 if k % 2 else 1, gc_cont=np.float32(vals[k % len(vals)]))
        cases.append(make_case("flags_gc_" + name, seqs, flag_layout(bad), {"gff": {}, "faa": {"width": 5}, "fna": {"width": 64}}, built_flagged=True))
    # midpoint flags only (no unprintable value): the text the device guessed has the host's length
    on = [confidence_scores()["on_%s" % m] for m in MIDPOINTS]
    cases.append(make_case("flags_midpoints", seqs, flag_layout(lambda k: rec(7 + k, 40 + k, 1, cscore=on[k % 5], sscore=0.0)), {"gff": {}},
                           built_flagged=True))
    return tuple(cases)


# ---- scores family -----------------------------------------------------------------------------------------------------------------------
# The rows of the start-score file come from the nodes the finder keeps on the device, so these are sequences, not records.

@functools.lru_cache(maxsize=None)
def scores_contigs():
    """(sequences, ids): the contigs of tests/start_shapes.py that put starts at open ends -- ORFs that run off either end of the
    contig on either strand, edge nodes -- between two contigs without a node."""
    from tests import start_shapes as ss
    seqs = [b"ACGT"]
    seqs += [ss.scan_contig(v, s) for v in ("edge", "conv0") for s in (1, -1)]
    seqs += [ss.end_contig(kind, u, s) for kind in ("sd", "mot") for u in (0, 2, 21) for s in (1, -1)]
    seqs += [ss.length_contig(1499, s) for s in (1, -1)]
    seqs += [ss.edge_contig(900, 150, 0.35, s) for s in (1, -1)]
    seqs.append(b"ACGT")
    return tuple(seqs), tuple("sc%d" % i for i in range(len(seqs)))


def scores_text(nd, t, seqnum, seqlen, sid, header):
    """Genes.write_scores restated over node arrays `nd` (by field name) and the model `t`."""
    from pyrodigal_amd import __version__
    out = []
    if header:
        out.append('# Sequence Data: seqnum=%d;seqlen=%d;seqhdr="%s"\n' % (seqnum, seqlen, sid))
        out.append("# Run Data: version=pyrodigal_amd.v%s;gc_cont=%.2f;transl_table=%d;uses_sd=%d\n" % (__version__, t.gc * 100, t.trans_table, int(t.uses_sd)))
        out.append("Beg\tEnd\tStd\tTotal\tCodPot\tStrtSc\tCodon\tRBSMot\tSpacer\tRBSScr\tUpsScr\tTypeScr\tGCCont\n")
    motif_of = ["None"] + orc.RBS_MOTIF[1:]
    spacer_of = ["None"] + orc.RBS_SPACER[1:]
    order = np.lexsort((nd["ndx"], -nd["strand"].astype(np.int32), nd["stop_val"]))
    prev = None
    for i in order:
        if nd["type"][i] == 3:
            continue
        ndx, sv, strand = int(nd["ndx"][i]), int(nd["stop_val"][i]), int(nd["strand"][i])
        if (sv, strand) != prev:
            prev = (sv, strand)
            out.append("\n")
        out.append("%d\t%d\t+\t" % (ndx + 1, sv + 3) if strand == 1 else "%d\t%d\t-\t" % (sv - 1, ndx + 1))
        cs, ss = float(nd["cscore"][i]), float(nd["sscore"][i])
        out.append("%.2f\t%.2f\t%.2f\t%s\t" % (cs + ss, cs, ss, ("ATG", "GTG", "TTG", "Edge")[3 if nd["edge"][i] else int(nd["type"][i])]))
        k0, k1 = int(nd["rbs"][i][0]), int(nd["rbs"][i][1])
        _, site = rbs_site(t, k0, k1, float(nd["mot_score"][i]))
        if site >= 0:
            out.append("%s\t%s\t" % (motif_of[site], spacer_of[site]))
        elif nd["mot_len"][i] == 0:
            out.append("None\tNone\t")
        else:
            out.append("%s\t%dbp\t" % ("".join("AGCT"[(int(nd["mot_ndx"][i]) >> (2 * q)) & 3] for q in range(int(nd["mot_len"][i]))), int(nd["mot_spacer"][i])))
        out.append("%.2f\t%.2f\t%.2f\t%.3f\n" % (float(nd["rscore"][i]), float(nd["uscore"][i]), float(nd["tscore"][i]), float(nd["gc_cont"][i])))
    out.append("\n")
    return "".join(out)


# ---- all of them -------------------------------------------------------------------------------------------------------------------------

def all_cases():
    return (number_cases() + (confidence_case(),) + body_cases() + gbk_body_cases() + (circular_case(),) + layout_cases()
            + (origin_case(),) + rbs_cases() + flag_cases())


def case_names():
    """Names without building anything but the cheap parts (for parametrising)."""
    return [c.name for c in all_cases()]


def case_by_name(name):
    return next(c for c in all_cases() if c.name == name)
