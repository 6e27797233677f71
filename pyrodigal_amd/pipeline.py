"""Keeping the device busy across batches: N contexts (one HIP stream and one set of scratch buffers each), one host
thread per context.  While one batch is in a host-side phase of its call (upload, chain planning, result unpacking)
the other contexts' kernels run; batches come back in input order.

One pool does this for every entry point (:func:`_in_order`): it hands the items of a lazy source to the contexts' threads, a
bounded number ahead of the consumer, and yields the results in the order of the source.  :func:`find_genes_stream` runs lists
of contigs through it, :func:`find_genes_fasta` and :func:`render_fasta` the batches of a file, each through the one step that
makes a parsed batch resident (:func:`_resident`); contexts and readers belong to these functions, not to the pool.

Measured on one MI355X with BASELINE config 3 batches (1000 x 50 kbp): 1 context 19.3 ms per batch (2.6 Gbp/s),
2 contexts 15.0 ms per batch (3.3 Gbp/s)."""
import contextlib
import io
import queue
import threading

from . import _cabi


def _in_order(items, ctxs, work, ahead):
    """Yield ``work(ctx, item)`` for every item of ``items``, in the order of ``items``, from one daemon thread per context of
    ``ctxs``.  ``items`` is pulled lazily, never more than ``ahead`` items beyond the one the consumer waits for.

    An exception of ``work`` is raised at its item's place in the order, after the results before it.  Once one is known nothing
    more is pulled; what was pulled is still handed to ``work`` (which hands a file's arenas back).  However the generator ends
    -- ``items`` exhausted, an exception of ``work`` or of ``items``, ``close()`` -- the threads are told to stop and joined
    before control leaves.  Contexts and sources are the caller's: the pool neither configures nor closes them."""
    ahead = max(1, ahead)                           # (with none ahead nothing would ever be pulled)
    todo = queue.Queue()                            # (index, item), or None: stop
    done, failed = {}, []
    cv = threading.Condition()

    def worker(ctx):
        for i, item in iter(todo.get, None):
            try:
                res = work(ctx, item)
            except BaseException as e:              # handed to the consumer, which raises it at place i
                res = e
                failed.append(e)
            with cv:
                done[i] = res
                cv.notify_all()

    threads = [threading.Thread(target=worker, args=(c,), daemon=True) for c in ctxs]
    for t in threads:
        t.start()
    try:
        it = iter(items)
        nxt = pulled = 0
        exhausted = False
        while True:
            while not exhausted and pulled - nxt < ahead and not failed:
                try:
                    item = next(it)
                except StopIteration:
                    exhausted = True
                    break
                todo.put((pulled, item))
                pulled += 1
            if nxt == pulled and exhausted:
                return
            with cv:
                while nxt not in done:
                    cv.wait()
                res = done.pop(nxt)
            nxt += 1
            if isinstance(res, BaseException):
                raise res
            yield res
    finally:
        for _ in threads:
            todo.put(None)
        for t in threads:
            t.join()


def _fresh_contexts(n_contexts, device, model_blobs):
    """``n_contexts`` (at least one) new contexts on ``device`` with the models loaded; whoever makes them closes them."""
    ctxs = [_cabi.Context(device) for _ in range(max(1, n_contexts))]
    for c in ctxs:
        c.set_models(list(model_blobs))
    return ctxs


def _close_all(ctxs):
    for c in ctxs:
        c.close()


def find_genes_stream(batches, model_blobs, n_contexts=2, device=0, **find_kw):
    """Yield ``(batch, BatchResult)`` for every batch of ``batches`` (an iterable of lists of contigs), in order.

    ``model_blobs``: the ``struct _training`` blobs to load in every context; ``find_kw`` goes to
    ``Context.find_genes_batch`` (meta, closed, mask, ...).  The batches go through the pool (:func:`_in_order`) on
    ``n_contexts`` fresh contexts; at most ``2 * n_contexts`` batches are in flight."""
    ctxs = _fresh_contexts(n_contexts, device, model_blobs)
    try:
        yield from _in_order(batches, ctxs, lambda ctx, batch: (batch, ctx.find_genes_batch(batch, **find_kw)), 2 * len(ctxs))
    finally:
        _close_all(ctxs)


def _attach_masks(batch, ids, lens, regions_by_id, mask_lowercase, seen):
    """The mask sources of one resident batch of a FASTA file: the regions of the records whose id is a key of ``regions_by_id``
    (checked against the record's length: ``ValueError`` names the record) and the lower-case rule.  ``seen`` collects the keys met."""
    regions = None
    if regions_by_id:
        regions = []
        for i, rid in enumerate(ids):
            iv = regions_by_id.get(rid)
            if iv is not None:
                seen.add(rid)
                for b, e in iv:
                    if not (0 <= b < e <= int(lens[i])):
                        raise ValueError("sequence %r: region [%d, %d) is not a non-empty part of the sequence [0, %d)" % (rid, b, e, int(lens[i])))
            regions.append(iv)
    if regions is not None or mask_lowercase:
        batch.set_masks(regions, mask_lowercase)


def circular_flags(circular, ids, descriptions, seen=None):
    """One flag per record from ``circular``: ``None`` / ``False`` (none), ``True`` (every record), a collection of sequence ids,
    or a predicate ``f(id, description)``.  ``seen`` collects the ids of a collection that were met.  Returns None when no
    record of the batch is circular."""
    if circular is None or circular is False:
        return None
    if circular is True:
        return [True] * len(ids)
    if callable(circular):
        flags = [bool(circular(i, d)) for i, d in zip(ids, descriptions)]
    else:
        flags = [i in circular for i in ids]
        if seen is not None:
            seen.update(i for i, f in zip(ids, flags) if f)
    return flags if any(flags) else None


def trim_terminal_repeats_of(batch, option):
    """The terminal-repeat step of one resident batch of a file.  ``option``: ``None`` / ``False``, ``True`` (the default parameters)
    or an object with ``min_length`` / ``max_length`` / ``max_base_percent`` (``lib.TerminalRepeats``); every record is searched.
    Returns ``(batch to call, match, trim)``: the batch itself and ``None, None`` when nothing was asked for; the batch itself when
    no record has a repeat; else its trimmed copy, which the caller closes."""
    if not (option is None or isinstance(option, bool) or hasattr(option, "min_length")):
        raise TypeError("trim_terminal_repeats of a file is True or one TerminalRepeats for every record, not %r" % type(option).__name__)
    tr = _cabi.terminal_repeat_options(batch.n, option)
    if tr is None:
        return batch, None, None
    match, trim = batch.terminal_repeats(None, *tr[1])
    return batch.trim_terminal_repeats(trim), match, trim


def terminal_repeat_status(match, trim):
    """The last column of the command line's ``--circular-report``."""
    return "trimmed" if trim > 0 else "low_complexity" if match > 0 else "none"


def header_says_circular(seq_id, description):
    """The predicate of ``--circular-from-header``: the description holds ``circular=true`` or ``topology=circular``, any case."""
    d = (description or "").lower()
    return "circular=true" in d or "topology=circular" in d


@contextlib.contextmanager
def _resident(ctx, pb, circular, regions_by_id, mask_lowercase, seen, trim_option, seen_circular=None, keep_letters=False):
    """One parsed batch of a file (``PackedRecords``) while it is resident on ``ctx``: uploaded (which hands its arena back to the
    reader), its masks attached, its circular flags set and its terminal repeats trimmed.  Yields ``(batch to call, match, trim,
    flags, letters)``: the first three as :func:`trim_terminal_repeats_of` returns them, then the circular flags of the batch to
    call (None: no circle) and, with ``keep_letters`` and a record that is or may become a circle, a host copy of its letters
    (read before the upload; a trimmed record is a circle of the bases it keeps).  On exit the trimmed copy, if there is one, and
    the batch are closed; on any exception the arena goes back as well."""
    try:
        ids, n = pb.ids, pb.n
        lens = [int(x) for x in pb.lens[:n]]
        flags = circular_flags(circular, ids, pb.descriptions, seen_circular)
        letters = None
        if keep_letters and (flags is not None or trim_option is not None):
            letters = [pb.sequence(k) for k in range(n)]
        b = ctx.upload_packed(pb)                         # releases the arena
        try:
            _attach_masks(b, ids, lens, regions_by_id, mask_lowercase, seen)
            b.set_circular(flags)
            t, match, trim = trim_terminal_repeats_of(b, trim_option)
            try:
                if t is not b:
                    flags = [bool(x) for x in t.circular[:n]]
                    if letters is not None:
                        letters = [s[:len(s) - int(x)] for s, x in zip(letters, trim)]
                yield t, match, trim, flags, letters
            finally:
                if t is not b:
                    t.close()
        finally:
            b.close()
    except BaseException:
        pb.release()
        raise


def _packed_in_order(reader, ctxs, work, max_bases, items_of=iter):
    """The batches of ``reader`` through the pool: ``work(ctx, item)`` for every item of ``items_of(packed batches)``.  At most
    ``len(ctxs) + 1`` batches are in flight, and the reader gets one pinned arena more than that, for the batch it is parsing."""
    ahead = len(ctxs) + 1
    return _in_order(items_of(reader.packed_batches(max_bases=max_bases, n_arenas=ahead + 1)), ctxs, work, ahead)


def find_genes_fasta(path, model_blobs, n_contexts=2, device=0, max_bases=64 << 20, contexts=None, regions_by_id=None,
                     mask_lowercase=False, circular=None, trim_terminal_repeats=None, **find_kw):
    """Genes of every record of a (gzipped) FASTA file: yields ``(ids, descriptions, lengths, BatchResult)`` per batch, in file order.

    The reader (C, zlib) parses batch k + 1 into a pinned staging arena while batch k is uploaded from its own arena with one
    DMA (no host-side packing) and processed (:func:`_resident`); the pool (:func:`_in_order`) keeps the device busy across
    batches on ``n_contexts`` contexts (ref: what the reference's CLI does with a thread pool over records, cli.py:287-302).
    `contexts`: contexts the caller keeps across files (models loaded, device buffers grown) instead of `n_contexts` fresh ones;
    they are left open.

    ``regions_by_id``: ``{sequence id: [(begin, end), ...]}``, masked regions (0-based, half-open) of the records with that id (the
    first word of the header); ``mask_lowercase``: runs of lower-case letters are masked (``Batch.set_masks``).
    ``circular``: the records that are circles, as :func:`circular_flags` takes them; their genes may end beyond the record's
    length and ``BatchResult.cuts`` says where each was cut open.  ``trim_terminal_repeats``: ``True`` or a ``TerminalRepeats``: a
    record that ends in a copy of its first bases loses the copy on the device and is called as a circle
    (``BatchResult.terminal_repeats``: the bases each record lost; the yielded lengths are those of the file)."""
    own = contexts is None
    ctxs = _fresh_contexts(n_contexts, device, model_blobs) if own else list(contexts)
    seen = set()

    def work(ctx, pb):
        with _resident(ctx, pb, circular, regions_by_id, mask_lowercase, seen, trim_terminal_repeats) as (t, _, trim, _, _):
            r = ctx.find_genes(t, **find_kw)
        r.terminal_repeats = trim
        return pb.ids, pb.descriptions, pb.lens, r

    try:
        with _cabi.FastaReader(path) as reader:
            yield from _packed_in_order(reader, ctxs, work, max_bases)
    finally:
        if own:
            _close_all(ctxs)


def plan_set_calls(ids, lens, sets_by_id, max_bases):
    """The device calls of a file whose records come in sets (``sets_by_id``: ``{sequence id: label}``; a record that is not listed
    is a set of its own).  A set must sit in one device call: the sets, in order of first appearance, fill a call up to
    ``max_bases`` bases, and a larger set gets a call of its own.  Returns ``(labels, calls, unmatched)``: the label of every record
    (None: on its own), the record indices of every call in file order, and the listed ids that no record carried."""
    labels = [sets_by_id.get(rid) for rid in ids]
    members, order = {}, []
    for i, lab in enumerate(labels):
        key = ("own", i) if lab is None else ("set", lab)
        if key not in members:
            members[key] = []
            order.append(key)
        members[key].append(i)
    calls, cur, cur_bases = [], [], 0
    for key in order:
        bases = sum(int(lens[i]) for i in members[key])
        if cur and cur_bases + bases > max_bases:
            calls.append(sorted(cur))
            cur, cur_bases = [], 0
        cur.extend(members[key])
        cur_bases += bases
    if cur:
        calls.append(sorted(cur))
    return labels, calls, sorted(set(sets_by_id) - set(ids))


def _render_fasta_sets(path, ctxs, formats, sinks, stats, sets_by_id, *, max_bases, meta, descriptions, first_seqnum, unbinned_model,
                       regions_by_id, mask_lowercase, want_nodes, seen, find_kw):
    """:func:`render_fasta` with ``sets_by_id``: the file is read whole, the device calls are packed from whole sets
    (:func:`plan_set_calls`) and go through the pool (:func:`_in_order`) all at once, every call is rendered while it is resident,
    and the text is written in file order at the end.  When several calls fail, the first of them in call order is raised."""
    with _cabi.FastaReader(path) as reader:
        records = [rec for batch in reader.batches() for rec in batch]
    ids = [r[0] for r in records]
    lens = [len(r[2]) for r in records]
    labels, calls, unmatched = plan_set_calls(ids, lens, sets_by_id, max_bases)
    text = {name: [b""] * len(records) for name in formats}

    def work(ctx, call):
        b = ctx.upload([records[i][2] for i in call])
        try:
            cids = [ids[i] for i in call]
            _attach_masks(b, cids, [lens[i] for i in call], regions_by_id, mask_lowercase, seen)
            b.set_sets([labels[i] for i in call])
            r = ctx.find_genes(b, meta=meta, want_nodes=want_nodes, **find_kw)
            out = ctx.render_genes(b, r, cids, formats, meta=meta, descriptions=descriptions, unbinned_model=unbinned_model,
                                   seqnums=[first_seqnum + i for i in call])
        finally:
            b.close()
        return call, len(r.genes), out

    with contextlib.closing(_in_order(calls, ctxs, work, len(calls))) as results:
        for call, n_genes, out in results:
            for name, t in out.items():
                for k, i in enumerate(call):
                    text[name][i] = t.contig(k)
                stats["fallback"] += t.fallback
                stats["kernel_ms"][name] += t.kernel_ms
            stats["genes"] += n_genes
    for name in formats:
        for piece in text[name]:
            sinks[name].write(piece)
    stats["records"] = len(records); stats["bases"] = sum(lens); stats["device_calls"] = len(calls)
    stats["sets_unmatched"] = unmatched
    stats["regions_unmatched"] = sorted(set(regions_by_id or ()) - seen)
    stats["circular_unmatched"] = []
    return stats


def _host_genbank(ctx, result, ids, letters, flags, options, meta, first_seqnum):
    """The GenBank text of a batch that holds circular records, by the host writer (the device renderer does not write locations
    across the origin): one ``Genes.write_genbank`` per record."""
    from . import lib                   # not at module level: the command line's --help does not load the Cython layer
    tinfs = {}
    out = io.StringIO()
    offs = [0]
    for i, c in enumerate(result.contigs):
        m = int(c["model"]) if meta else 0
        tinf = None
        if m >= 0:
            if m not in tinfs:
                tinfs[m] = lib.TrainingInfo(raw=ctx._models[m].tobytes())
            tinf = tinfs[m]
        recs = result.genes[int(c["gene_begin"]):int(c["gene_begin"]) + int(c["n_genes"])].tobytes()
        circ = bool(flags[i])
        genes = lib._genes_from_records(letters[i], recs, tinf, first_seqnum + i, meta=meta, circular=circ,
                                        cut=int(result.cuts[i]) if circ else None)
        genes.write_genbank(out, ids[i], **options)
        offs.append(len(out.getvalue().encode("utf-8")))
    return _cabi.RenderedText(out.getvalue().encode("utf-8"), offs, 0, 0.0)


def render_fasta(path, model_blobs, *, gff=None, faa=None, fna=None, gbk=None, scores=None, n_contexts=2, device=0, max_bases=64 << 20,
                 meta=False, descriptions=None, first_seqnum=1, gff_options=None, faa_options=None, fna_options=None, gbk_options=None,
                 scores_options=None, unbinned_model=None, regions_by_id=None, mask_lowercase=False, circular=None, sets_by_id=None,
                 trim_terminal_repeats=None, **find_kw):
    """Call the genes of every record of a FASTA file and write them as text: GFF to ``gff``, protein FASTA to ``faa``, gene
    FASTA to ``fna``, GenBank to ``gbk``, the start-score file to ``scores`` (binary file objects, or None), in file order --
    what ``Genes.write_gff`` / ``write_translations`` / ``write_genes`` / ``write_genbank`` / ``write_scores`` write record after
    record.  With ``scores`` the genes are found with ``want_nodes="device"``: the node arrays stay on the device for the
    renderer.

    Runs like :func:`find_genes_fasta` (the C reader fills pinned arenas, the same pool over ``n_contexts`` fresh contexts, the
    same resident step per batch), but every batch is rendered on the device while it is still resident
    (``Context.render_genes``) and only its text comes back, to be written by the calling thread: memory stays bounded by the
    batch size.Sequence ids are the first word of the headers, seqnums count records from ``first_seqnum``.
    ``*_options``: the writer's keyword arguments of that format; ``unbinned_model``: see ``Context.render_genes``; ``find_kw``
    goes to ``Context.find_genes``.  ``regions_by_id`` / ``mask_lowercase``: more mask sources, as :func:`find_genes_fasta` takes
    them.  ``circular``: the records that are circles (:func:`circular_flags`): called across the origin, ``topology=circular``
    in their GFF header.  The start-score file cannot be written with them (``ValueError``); a GenBank batch that holds one is
    written by the host writer ``Genes.write_genbank`` (``join()`` locations, ``LOCUS ... circular``), byte for byte what the
    device writes for its linear records.  Returns ``{"records", "bases", "genes", "fallback", "kernel_ms": {format: ms},
    "regions_unmatched": [ids of regions_by_id that no record carried], "circular_unmatched": [ids of a ``circular`` collection
    that no record carried]}``.

    ``trim_terminal_repeats``: ``True`` or a ``TerminalRepeats``.  Every record is searched on the device for a copy of its first
    bases at its end; a record that has one loses it and is called, and written, as a circle of the remaining bases, whatever
    ``circular`` says of it.  Refused with ``scores`` and ``sets_by_id`` like ``circular``.  The result then holds
    ``"terminal_repeats": [(id, length, match, trim)]`` for the records with ``match > 0`` (``trim == 0``: a low-complexity repeat,
    left alone) and ``"terminal_repeat_records"``, the same for every record, both in file order; lengths are those of the file.

    ``sets_by_id`` (meta mode): ``{sequence id: label}``, the set of contigs a record belongs to -- the contig-to-bin table of a
    binner; a record that is not listed is on its own.  One model is chosen per set (``Batch.set_sets``).  A set must sit in one
    device call, so the file is then read whole and held in memory together with its output text until the last call is done;
    the calls are packed from whole sets up to ``max_bases`` (a larger set gets a call of its own) and the output stays in file
    order.  Not with ``circular``.  The result also holds ``"sets_unmatched"`` and ``"device_calls"`` then."""
    seen = set()
    seen_circular = set()
    if sets_by_id is not None:
        if not meta:
            raise ValueError("render_fasta: `sets_by_id` is a meta-mode option")
        if circular is not None and circular is not False:
            raise ValueError("render_fasta: `sets_by_id` cannot be combined with `circular`")
    trim_option = trim_terminal_repeats if trim_terminal_repeats is not None and trim_terminal_repeats is not False else None
    if sets_by_id is not None and trim_option is not None:
        raise ValueError("render_fasta: `sets_by_id` cannot be combined with `trim_terminal_repeats`")
    if scores is not None and ((circular is not None and circular is not False) or trim_option is not None):
        raise ValueError("render_fasta: the start-score file is not written for circular records")
    formats = {}
    for name, fh, opts in (("gff", gff, gff_options), ("faa", faa, faa_options), ("fna", fna, fna_options), ("gbk", gbk, gbk_options),
                           ("scores", scores, scores_options)):
        if fh is not None:
            formats[name] = dict(opts or {})
    stats = {"records": 0, "bases": 0, "genes": 0, "fallback": 0, "kernel_ms": {k: 0.0 for k in formats}}
    if trim_option is not None:
        stats["terminal_repeats"], stats["terminal_repeat_records"] = [], []
    if not formats:
        raise ValueError("render_fasta: no output requested")
    sinks = {"gff": gff, "faa": faa, "fna": fna, "gbk": gbk, "scores": scores}
    if "gbk" in formats and formats["gbk"].get("date") is None:
        import datetime
        formats["gbk"]["date"] = datetime.date.today()       # one date for the whole file
    want_nodes = "device" if scores is not None else False
    ctxs = _fresh_contexts(n_contexts, device, model_blobs)
    try:
        if sets_by_id is not None:
            return _render_fasta_sets(path, ctxs, formats, sinks, stats, dict(sets_by_id), max_bases=max_bases, meta=meta,
                                      descriptions=descriptions, first_seqnum=first_seqnum, unbinned_model=unbinned_model,
                                      regions_by_id=regions_by_id, mask_lowercase=mask_lowercase, want_nodes=want_nodes, seen=seen,
                                      find_kw=find_kw)

        def numbered(batches):              # (seqnum of its first record, batch)
            seqnum = first_seqnum
            for pb in batches:
                yield seqnum, pb
                seqnum += pb.n

        def work(ctx, item):
            seqnum, pb = item
            ids, n = pb.ids, pb.n
            lens = [int(x) for x in pb.lens[:n]]
            with _resident(ctx, pb, circular, regions_by_id, mask_lowercase, seen, trim_option, seen_circular,
                           keep_letters="gbk" in formats) as (t, match, trim, flags, letters):
                found = None
                if match is not None:
                    found = [(ids[k], lens[k], int(match[k]), int(trim[k])) for k in range(n)]
                host_gbk = "gbk" in formats and flags is not None
                r = ctx.find_genes(t, meta=meta, want_nodes=want_nodes, **find_kw)
                dev_formats = {k: v for k, v in formats.items() if not (host_gbk and k == "gbk")}
                text = {}
                if dev_formats:
                    text = ctx.render_genes(t, r, ids, dev_formats, meta=meta, descriptions=descriptions, first_seqnum=seqnum,
                                            unbinned_model=unbinned_model)
                if host_gbk:
                    text["gbk"] = _host_genbank(ctx, r, ids, letters, flags, formats["gbk"], meta, seqnum)
            return n, pb.total, len(r.genes), text, found

        with _cabi.FastaReader(path) as reader, contextlib.closing(_packed_in_order(reader, ctxs, work, max_bases, numbered)) as results:
            for n, total, n_genes, text, found in results:
                if found is not None:
                    stats["terminal_repeat_records"].extend(found)
                    stats["terminal_repeats"].extend(x for x in found if x[2] > 0)
                for name, t in text.items():
                    sinks[name].write(t.data)
                    stats["fallback"] += t.fallback
                    stats["kernel_ms"][name] += t.kernel_ms
                stats["records"] += n; stats["bases"] += total; stats["genes"] += n_genes
        stats["regions_unmatched"] = sorted(set(regions_by_id or ()) - seen)
        listed = circular if circular is not None and not isinstance(circular, bool) and not callable(circular) else ()
        stats["circular_unmatched"] = sorted(set(listed) - seen_circular)
        return stats
    finally:
        _close_all(ctxs)
