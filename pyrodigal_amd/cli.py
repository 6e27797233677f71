"""Prodigal-compatible command line, with the options of pyrodigal's (ref: cli.py:64-323).

Every output -- GFF or GenBank (``-f``), protein FASTA (``-a``), gene FASTA (``-d``) and the start file (``-s``) -- is rendered
on the device (``pipeline.render_fasta``).  Argument parsing and ``--help`` do not load the HIP library."""
import argparse
import contextlib
import os
import shutil
import sys
import tempfile

from . import __version__

# ref: lib.pyx TRANSLATION_TABLES (restated so that parsing needs no compiled module)
TRANSLATION_TABLES = frozenset(set(range(1, 7)) | set(range(9, 17)) | set(range(21, 27)) | {29, 30, 32, 33})


def _table_arg(value):
    return "auto" if value == "auto" else int(value)


def argument_parser(prog="pyrodigal_amd"):
    p = argparse.ArgumentParser(prog=prog, add_help=False, formatter_class=argparse.ArgumentDefaultsHelpFormatter,
                                description="Prodigal gene calling on an AMD Instinct MI355X.")
    p.add_argument("-a", metavar="trans_file", help="Write protein translations to the selected file.")
    p.add_argument("-c", action="store_true", default=False, help="Closed ends. Do not allow genes to run off edges.")
    p.add_argument("-d", metavar="nuc_file", help="Write nucleotide sequences of genes to the selected file.")
    p.add_argument("-f", metavar="output_type", choices=("gff", "gbk"), default="gff",
                   help="Select output format.")
    p.add_argument("-g", metavar="tr_table", type=_table_arg, choices=sorted(TRANSLATION_TABLES) + ["auto"], default=11,
                   help="Specify a translation table to use; auto: 11, or 4 when its genes cover clearly more of the genome "
                        "(single mode, before training).")
    p.add_argument("-i", metavar="input_file", help="Specify FASTA input file (plain, .gz, .bz2 or .xz; default: stdin).")
    p.add_argument("-m", action="store_true", default=False, help="Treat runs of N as masked sequence; don't build genes across them.")
    p.add_argument("-n", action="store_true", default=False, help="Bypass Shine-Dalgarno trainer and force a full motif scan.")
    p.add_argument("-o", metavar="output_file", help="Specify output file (default: stdout).")
    p.add_argument("-p", metavar="mode", choices=("single", "meta"), default="single", help="Select procedure.")
    p.add_argument("-s", metavar="start_file", help="Write all potential genes (with scores) to the selected file.")
    p.add_argument("-t", metavar="training_file",
                   help="Write a training file (if none exists); otherwise, read and use the specified training file.")
    p.add_argument("-j", "--jobs", type=int, default=2, metavar="jobs",
                   help="The number of device contexts working side by side (not threads).")
    p.add_argument("-h", "--help", action="help", help="Show this help message and exit.")
    p.add_argument("-V", "--version", action="version", version="{} v{}".format(prog, __version__), help="Show version number and exit.")
    p.add_argument("--min-gene", type=int, default=90, help="The minimum gene length.")
    p.add_argument("--min-edge-gene", type=int, default=60, help="The minimum edge gene length.")
    p.add_argument("--max-overlap", type=int, default=60,
                   help="The maximum number of nucleotides that can overlap between two genes on the same strand. "
                        "This must be lower or equal to the minimum gene length.")
    p.add_argument("--no-stop-codon", action="store_true", default=False,
                   help="Disables translation of stop codons into star characters (*) for complete genes.")
    p.add_argument("--meta-bins", metavar="FILE", nargs="+",
                   help="TrainingInfo dumps to use as the metagenomic bins of -p meta (this build ships none). The GFF header of a "
                        "contig without genes reports the sixth bin, as Prodigal does (the last one when fewer are given).")
    p.add_argument("--batch-bases", type=int, default=64 << 20, metavar="N", help="Bases per device call.")
    p.add_argument("--mask-lowercase", action="store_true", default=False,
                   help="Treat runs of lower-case letters (soft-masked sequence) as masked sequence; don't build genes across them.")
    p.add_argument("--mask-regions", metavar="FILE",
                   help="Don't build genes across the regions of this BED-like file: tab-separated seqid, start, end (0-based, "
                        "half-open; seqid is the first word of the FASTA header); further columns, # lines and track lines are ignored.")
    p.add_argument("--circular", action="store_true", default=False,
                   help="Every record is a circular sequence cut open at an arbitrary base: genes are called across the origin "
                        "(a gene across it ends beyond the sequence length).")
    p.add_argument("--circular-ids", metavar="FILE",
                   help="The records whose id (first word of the FASTA header) is listed in this file, one per line, are circular.")
    p.add_argument("--circular-from-header", action="store_true", default=False,
                   help="The records whose header says circular=true or topology=circular (any letter case) are circular.")
    p.add_argument("--circular-detect", action="store_true", default=False,
                   help="Look for a direct terminal repeat in every record: a record whose first bases are also its last (what an "
                        "assembler writes for a circular contig) loses the second copy and is called as a circular sequence. "
                        "A record --circular, --circular-ids or --circular-from-header names stays circular either way.")
    p.add_argument("--min-repeat", type=int, default=20, metavar="N", help="The shortest terminal repeat --circular-detect accepts.")
    p.add_argument("--max-repeat", type=int, default=65536, metavar="N",
                   help="The longest terminal repeat --circular-detect looks for (at most half of the record).")
    p.add_argument("--circular-report", metavar="FILE",
                   help="With --circular-detect: write seqid, length, match, trim and status (trimmed, low_complexity or none) of "
                        "every record to this file, tab-separated, in input order.")
    p.add_argument("--bin-map", metavar="FILE",
                   help="With -p meta: choose one model per set of contigs. Tab-separated seqid, bin -- the contig-to-bin table a "
                        "binner writes (seqid is the first word of the FASTA header); # lines are ignored, a sequence that is not "
                        "listed is on its own. The input is read whole: a set must sit in one device call.")
    return p


def parse_bin_map(lines, name="<bin map>"):
    """``{seqid: bin}`` of a contig-to-bin table (an iterable of lines): tab-separated ``seqid  bin``; blank lines and ``#`` lines
    are ignored.  A malformed line, or a sequence listed under two bins, is a ``ValueError`` that names the line."""
    bins = {}
    for no, line in enumerate(lines, 1):
        if isinstance(line, bytes):
            line = line.decode("utf-8", "replace")
        text = line.rstrip("\r\n")
        if not text.strip() or text.startswith("#"):
            continue
        cols = text.split("\t")
        if len(cols) != 2 or not cols[0].strip() or not cols[1].strip():
            raise ValueError("%s, line %d: expected seqid<TAB>bin, found %r" % (name, no, text))
        seqid, label = cols[0].strip(), cols[1].strip()
        if bins.setdefault(seqid, label) != label:
            raise ValueError("%s, line %d: sequence %r is listed under bin %r and bin %r" % (name, no, seqid, bins[seqid], label))
    return bins


def read_bin_map(path):
    with open(path, "r", encoding="utf-8", errors="replace") as fh:
        return parse_bin_map(fh, path)


def parse_circular_ids(lines):
    """The set of sequence ids of a text (an iterable of lines), one id per line: the first word counts, blank lines and
    ``#`` lines are ignored."""
    ids = set()
    for line in lines:
        if isinstance(line, bytes):
            line = line.decode("utf-8", "replace")
        words = line.split()
        if words and not words[0].startswith("#"):
            ids.add(words[0])
    return ids


def circular_option(args):
    """What ``pipeline.render_fasta(circular=...)`` takes for the three options (None: no record is circular).  With several of
    them a record is circular when any says so."""
    if args.circular:
        return True
    ids = None
    if args.circular_ids is not None:
        with open(args.circular_ids, "r", encoding="utf-8", errors="replace") as fh:
            ids = parse_circular_ids(fh)
    if args.circular_from_header:
        from .pipeline import header_says_circular
        if ids is None:
            return header_says_circular
        return _ListedOrHeader(ids)
    return ids


class _ListedOrHeader:
    """``--circular-ids`` and ``--circular-from-header`` together: a predicate that also remembers the listed ids it met."""

    def __init__(self, ids):
        self.ids, self.seen = ids, set()

    def __call__(self, seq_id, description):
        from .pipeline import header_says_circular
        if seq_id in self.ids:
            self.seen.add(seq_id)
            return True
        return header_says_circular(seq_id, description)


class TerminalRepeatOption:
    """The parameters of ``--circular-detect`` as ``pipeline.render_fasta(trim_terminal_repeats=...)`` takes them."""

    def __init__(self, min_length=20, max_length=65536, max_base_percent=75):
        self.min_length, self.max_length, self.max_base_percent = min_length, max_length, max_base_percent

    def __eq__(self, other):
        return (self.min_length, self.max_length, self.max_base_percent) == (other.min_length, other.max_length, other.max_base_percent)

    def __repr__(self):
        return "TerminalRepeatOption(%d, %d, %d)" % (self.min_length, self.max_length, self.max_base_percent)


def terminal_repeat_option(args):
    """What ``pipeline.render_fasta(trim_terminal_repeats=...)`` takes for ``--circular-detect`` (None: not asked for)."""
    if not args.circular_detect:
        return None
    return TerminalRepeatOption(args.min_repeat, args.max_repeat)


def write_circular_report(file, records):
    """``--circular-report``: one line per record, ``seqid  length  match  trim  status``, tab-separated.  ``records``: the
    ``"terminal_repeat_records"`` of ``pipeline.render_fasta``, ``(seqid, length, match, trim)`` in input order; ``file`` takes text."""
    from .pipeline import terminal_repeat_status
    for seqid, length, match, trim in records:
        file.write("%s\t%d\t%d\t%d\t%s\n" % (seqid, length, match, trim, terminal_repeat_status(match, trim)))


def parse_mask_regions(lines, name="<regions>"):
    """``{seqid: [(start, end), ...]}`` of a BED-like text (an iterable of lines): tab-separated ``seqid  start  end``, 0-based and
    half-open; further columns, blank lines, ``#`` lines and ``track`` / ``browser`` lines are ignored.  A malformed line is a
    ``ValueError`` that names it."""
    regions = {}
    for no, line in enumerate(lines, 1):
        if isinstance(line, bytes):
            line = line.decode("utf-8", "replace")
        text = line.rstrip("\r\n")
        if not text.strip() or text.startswith("#") or text.split(None, 1)[0] in ("track", "browser"):
            continue
        cols = text.split("\t")
        try:
            if len(cols) < 3 or not cols[0]:
                raise ValueError
            start, end = int(cols[1]), int(cols[2])
        except ValueError:
            raise ValueError("%s, line %d: expected seqid<TAB>start<TAB>end, found %r" % (name, no, text)) from None
        if start < 0 or end <= start:
            raise ValueError("%s, line %d: not a region (0 <= start < end): %r" % (name, no, text))
        regions.setdefault(cols[0], []).append((start, end))
    return regions


def read_mask_regions(path):
    with open(path, "r", encoding="utf-8", errors="replace") as fh:
        return parse_mask_regions(fh, path)


# A contig without genes wins no bin in meta mode; its GFF header reports bin 5, as Prodigal's does (ref: lib.pyx:3584-3592), or
# the last bin when fewer are given.  Its start file is that bin's header and an empty body.
UNBINNED_BIN = 5


def _check(args):
    """The option combinations the command line refuses (message, or None)."""
    if args.p == "meta" and args.t is not None:
        return "cannot specify metagenomic sequence with a training file."
    if args.p == "meta" and not args.meta_bins:
        return "-p meta needs --meta-bins: this build has no built-in metagenomic models."
    if args.jobs < 1:
        return "-j must be at least 1."
    if args.batch_bases < 1:
        return "--batch-bases must be at least 1."
    if args.s is not None and (args.circular or args.circular_ids is not None or args.circular_from_header):
        return "-s cannot be combined with --circular, --circular-ids or --circular-from-header: the start file is not written for circular sequences."
    if args.s is not None and args.circular_detect:
        return "-s cannot be combined with --circular-detect: the start file is not written for circular sequences."
    if not args.circular_detect and args.circular_report is not None:
        return "--circular-report needs --circular-detect."
    if args.circular_detect and not (1 <= args.min_repeat <= args.max_repeat <= 1048576):
        return "--min-repeat and --max-repeat must satisfy 1 <= min <= max <= 1048576."
    if args.bin_map is not None and args.p != "meta":
        return "--bin-map needs -p meta: one model per set of contigs is a choice among the metagenomic bins."
    if args.bin_map is not None and (args.circular or args.circular_ids is not None or args.circular_from_header):
        return ("--bin-map cannot be combined with --circular, --circular-ids or --circular-from-header: the second pass of a circular "
                "call holds only the circular members of a set.")
    if args.bin_map is not None and args.circular_detect:
        return ("--bin-map cannot be combined with --circular-detect: the second pass of a circular call holds only the circular "
                "members of a set.")
    return None


def _records(path):
    from . import _cabi
    with _cabi.FastaReader(path) as r:
        for batch in r.batches():
            yield from batch


def main(argv=None, stdout=None, stderr=None):
    parser = argument_parser()
    args = parser.parse_args(argv)
    stderr = sys.stderr if stderr is None else stderr
    stdout = sys.stdout.buffer if stdout is None else stdout
    err = _check(args)
    if err:
        print("Error: " + err, file=stderr)
        return 1
    regions = None
    if args.mask_regions is not None:
        try:
            regions = read_mask_regions(args.mask_regions)
        except (OSError, ValueError) as e:
            print("Error: --mask-regions: %s" % e, file=stderr)
            return 1
    try:
        circular = circular_option(args)
    except OSError as e:
        print("Error: --circular-ids: %s" % e, file=stderr)
        return 1
    mask_kw = dict(regions_by_id=regions, mask_lowercase=args.mask_lowercase, circular=circular)
    detect = terminal_repeat_option(args)
    if detect is not None:
        mask_kw["trim_terminal_repeats"] = detect
    if args.bin_map is not None:
        try:
            mask_kw["sets_by_id"] = read_bin_map(args.bin_map)
        except (OSError, ValueError) as e:
            print("Error: --bin-map: %s" % e, file=stderr)
            return 1
    with contextlib.ExitStack() as stack:
        path = args.i
        if path is None:                        # stdin: the reader needs a file it can sniff and map
            tmp = stack.enter_context(tempfile.TemporaryDirectory())
            path = os.path.join(tmp, "stdin.fa")
            with open(path, "wb") as f:
                shutil.copyfileobj(sys.stdin.buffer, f)
        from . import lib
        out = stdout if args.o is None else stack.enter_context(open(args.o, "wb"))
        faa = None if args.a is None else stack.enter_context(open(args.a, "wb"))
        fna = None if args.d is None else stack.enter_context(open(args.d, "wb"))
        find_kw = dict(closed=args.c, mask=args.m, min_gene=args.min_gene, min_edge_gene=args.min_edge_gene, max_overlap=args.max_overlap)
        meta = args.p == "meta"
        if meta:
            bins = []
            for f in args.meta_bins:
                with open(f, "rb") as fh:
                    bins.append(lib.MetagenomicBin(lib.TrainingInfo.load(fh), os.path.basename(f)))
            blobs = [b.training_info.raw for b in bins]
            descriptions = [b.description for b in bins]
            unbinned = min(UNBINNED_BIN, len(bins) - 1)
        else:
            tinf = None
            if args.t is not None and os.path.exists(args.t):
                with open(args.t, "rb") as fh:
                    tinf = lib.TrainingInfo.load(fh)
            if tinf is None:
                records = [(rid, s) for rid, _, s in _records(path)]
                seqs = [s for _, s in records]
                train_regions = None            # the training honours the masks too: per contig, through the join
                if regions:
                    per = [regions.get(rid) for rid, _ in records]
                    train_regions = per if len(per) > 1 else per[0]
                finder = lib.GeneFinder(mask_lowercase=args.mask_lowercase, **find_kw)
                tinf = finder.train(*seqs, force_nonsd=args.n, translation_table=args.g, regions=train_regions)
                del seqs, records
                if args.t is not None:
                    with open(args.t, "wb") as fh:
                        tinf.dump(fh)
            blobs, descriptions, unbinned = [tinf.raw], None, None
        scores = None if args.s is None else stack.enter_context(open(args.s, "wb"))
        report = None
        if args.circular_report is not None:
            try:
                report = stack.enter_context(open(args.circular_report, "w", encoding="utf-8"))
            except OSError as e:
                print("Error: --circular-report: %s" % e, file=stderr)
                return 1
        from .pipeline import render_fasta
        stats = render_fasta(path, blobs, gff=out if args.f == "gff" else None, gbk=out if args.f == "gbk" else None, faa=faa, fna=fna,
                             scores=scores, n_contexts=args.jobs, max_bases=args.batch_bases, meta=meta, descriptions=descriptions,
                             faa_options={"include_stop": not args.no_stop_codon}, unbinned_model=unbinned, **mask_kw, **find_kw)
        if report is not None:
            write_circular_report(report, stats.get("terminal_repeat_records", ()))
        for rid in stats.get("regions_unmatched", ()):
            print("Warning: --mask-regions: no sequence %r in the input" % rid, file=stderr)
        for rid in stats.get("sets_unmatched", ()):
            print("Warning: --bin-map: no sequence %r in the input" % rid, file=stderr)
        unmatched = stats.get("circular_unmatched", ())
        if isinstance(circular, _ListedOrHeader):
            unmatched = sorted(circular.ids - circular.seen)
        for rid in unmatched:
            print("Warning: --circular-ids: no sequence %r in the input" % rid, file=stderr)
    return 0
