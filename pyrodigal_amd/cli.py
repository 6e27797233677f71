"""Prodigal-compatible command line, with the options of pyrodigal's (ref: cli.py:64-323).

GFF, protein FASTA (``-a``) and gene FASTA (``-d``) are rendered on the device (``pipeline.render_fasta``).  GenBank output
(``-f gbk``) and the start file (``-s``) go through the host writers (``Genes.write_genbank`` / ``write_scores``): correct
but much slower.  Argument parsing and ``--help`` do not load the HIP library."""
import argparse
import contextlib
import os
import shutil
import sys
import tempfile

from . import __version__

# ref: lib.pyx TRANSLATION_TABLES (restated so that parsing needs no compiled module)
TRANSLATION_TABLES = frozenset(set(range(1, 7)) | set(range(9, 17)) | set(range(21, 27)) | {29, 30, 32, 33})


def argument_parser(prog="pyrodigal_amd"):
    p = argparse.ArgumentParser(prog=prog, add_help=False, formatter_class=argparse.ArgumentDefaultsHelpFormatter,
                                description="Prodigal gene calling on an AMD Instinct MI355X.")
    p.add_argument("-a", metavar="trans_file", help="Write protein translations to the selected file.")
    p.add_argument("-c", action="store_true", default=False, help="Closed ends. Do not allow genes to run off edges.")
    p.add_argument("-d", metavar="nuc_file", help="Write nucleotide sequences of genes to the selected file.")
    p.add_argument("-f", metavar="output_type", choices=("gff", "gbk"), default="gff",
                   help="Select output format. gbk is written by the host writer: correct but much slower than gff.")
    p.add_argument("-g", metavar="tr_table", type=int, choices=sorted(TRANSLATION_TABLES), default=11,
                   help="Specify a translation table to use.")
    p.add_argument("-i", metavar="input_file", help="Specify FASTA input file (plain, .gz, .bz2 or .xz; default: stdin).")
    p.add_argument("-m", action="store_true", default=False, help="Treat runs of N as masked sequence; don't build genes across them.")
    p.add_argument("-n", action="store_true", default=False, help="Bypass Shine-Dalgarno trainer and force a full motif scan.")
    p.add_argument("-o", metavar="output_file", help="Specify output file (default: stdout).")
    p.add_argument("-p", metavar="mode", choices=("single", "meta"), default="single", help="Select procedure.")
    p.add_argument("-s", metavar="start_file",
                   help="Write all potential genes (with scores) to the selected file. Written by the host writer: slow.")
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
    return p


# A contig without genes wins no bin in meta mode; its GFF header reports bin 5, as Prodigal's does (ref: lib.pyx:3584-3592), or
# the last bin when fewer are given.
UNBINNED_BIN = 5


def _unbinned_gff(genes, seq_id, fallback):
    """write_gff's text for a meta-mode contig without genes: the header lines, the fallback bin's model data."""
    t = fallback.training_info
    return ('##gff-version  3\n# Sequence Data: seqnum=%d;seqlen=%d;seqhdr="%s"\n'
            '# Model Data: version=pyrodigal_amd.v%s;run_type=Metagenomic;model="%s";gc_cont=%.2f;transl_table=%d;uses_sd=%d\n'
            % (genes._num_seq, len(genes.sequence), seq_id, __version__, fallback.description, t.gc * 100, t.translation_table,
               int(t.uses_sd)))


def _unbinned_scores(genes, seq_id, fallback):
    """write_scores' text for a meta-mode contig without genes: no model won, so there are no scored nodes to list."""
    t = fallback.training_info
    return ('# Sequence Data: seqnum=%d;seqlen=%d;seqhdr="%s"\n'
            '# Run Data: version=pyrodigal_amd.v%s;gc_cont=%.2f;transl_table=%d;uses_sd=%d\n'
            'Beg\tEnd\tStd\tTotal\tCodPot\tStrtSc\tCodon\tRBSMot\tSpacer\tRBSScr\tUpsScr\tTypeScr\tGCCont\n\n'
            % (genes._num_seq, len(genes.sequence), seq_id, __version__, t.gc * 100, t.translation_table, int(t.uses_sd)))


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
            finder = lib.GeneFinder(meta=True, metagenomic_bins=lib.MetagenomicBins(bins), keep_nodes=args.s is not None, **find_kw)
            blobs = [b.training_info.raw for b in bins]
            descriptions = [b.description for b in bins]
            unbinned = min(UNBINNED_BIN, len(bins) - 1)
        else:
            tinf = None
            if args.t is not None and os.path.exists(args.t):
                with open(args.t, "rb") as fh:
                    tinf = lib.TrainingInfo.load(fh)
            finder = lib.GeneFinder(tinf, keep_nodes=args.s is not None, **find_kw)
            if tinf is None:
                seqs = [s for _, _, s in _records(path)]
                tinf = finder.train(*seqs, force_nonsd=args.n, translation_table=args.g)
                del seqs
                if args.t is not None:
                    with open(args.t, "wb") as fh:
                        tinf.dump(fh)
            blobs, descriptions, unbinned = [tinf.raw], None, None
        host_main = args.f == "gbk" or args.s is not None
        if not host_main:
            from .pipeline import render_fasta
            render_fasta(path, blobs, gff=out, faa=faa, fna=fna, n_contexts=args.jobs, max_bases=args.batch_bases, meta=meta,
                         descriptions=descriptions, faa_options={"include_stop": not args.no_stop_codon}, unbinned_model=unbinned,
                         **find_kw)
            return 0
        # GenBank / start file: the host writers, record by record (ref: cli.py:304-321)
        import io
        scores = None if args.s is None else stack.enter_context(open(args.s, "w"))
        text = io.TextIOWrapper(out, encoding="utf-8", write_through=True)
        faa_t = None if faa is None else io.TextIOWrapper(faa, encoding="utf-8", write_through=True)
        fna_t = None if fna is None else io.TextIOWrapper(fna, encoding="utf-8", write_through=True)
        for seq_id, _, seq in _records(path):
            genes = finder.find_genes(seq)
            fallback = bins[unbinned] if meta and genes.metagenomic_bin is None else None
            if args.f == "gbk":
                genes.write_genbank(text, sequence_id=seq_id)
            elif fallback is not None:
                text.write(_unbinned_gff(genes, seq_id, fallback))
            else:
                genes.write_gff(text, sequence_id=seq_id)
            if fna_t is not None:
                genes.write_genes(fna_t, sequence_id=seq_id)
            if faa_t is not None:
                genes.write_translations(faa_t, sequence_id=seq_id, include_stop=not args.no_stop_codon)
            if scores is not None and fallback is not None:
                scores.write(_unbinned_scores(genes, seq_id, fallback))
            elif scores is not None:
                genes.write_scores(scores, sequence_id=seq_id)
        for t in (text, faa_t, fna_t):
            if t is not None:
                t.flush()
                t.detach()
    return 0
