# cython: language_level=3, boundscheck=False, wraparound=False, cdivision=True
"""Cython host layer: pyrodigal's `GeneFinder.find_genes()` / `Genes` API over the HIP C-ABI.

Same names, arguments, defaults, validation and error types as the reference
(/root/reference/src/pyrodigal/lib.pyx; citations below are into that file), but every
per-base / per-node computation happens in `libpyrodigal_amd.so` on an MI355X.  There is no
CPU path: without the library or a gfx950 device, calls raise `RuntimeError`.

`Nodes.extract / sort / reset_scores / score` and `ConnectionScorer` are the stage-level calls of the
reference (lib.pyx:2501-2595, 1315-1357) over `pga_nodes_stage` / `pga_score_connections`; the scorer
works on whole node arrays, not node by node (SURVEY 8b: per-node granularity is useless for a GPU).

`Gene.translate` and the `Genes.write_*` writers are host-side formatting, as in the reference.
`GeneFinder.train` runs on the device too (`pga_train`).
"""
import ctypes
import gzip
import threading

import numpy as np

from cpython.bytes cimport PyBytes_FromStringAndSize, PyBytes_AS_STRING
from libc.stdint cimport int8_t, uint8_t, int32_t, int64_t
from libc.stdlib cimport malloc, free
from libc.string cimport memcpy, memset
from libc.math cimport exp, fmax

cdef extern from "pyrodigal_amd.h" nogil:
    ctypedef struct pga_ctx
    ctypedef struct pga_batch
    ctypedef struct pga_training
    ctypedef struct pga_params:
        int32_t closed
        int32_t min_gene
        int32_t min_edge_gene
        int32_t max_overlap
        int32_t meta
        int32_t want_nodes
        int32_t mask
        int32_t min_mask
    ctypedef struct pga_gene:
        int32_t contig
        int32_t begin
        int32_t end
        int32_t start_ndx
        int32_t stop_ndx
        int8_t strand
        uint8_t partial_begin
        uint8_t partial_end
        uint8_t start_type
        uint8_t rbs[2]
        uint8_t mot_len
        uint8_t mot_spacer
        int32_t mot_ndx
        float gc_cont
        double cscore
        double sscore
        double rscore
        double uscore
        double tscore
        double mot_score
    ctypedef struct pga_nodes:
        int32_t n
        int32_t* ndx
        int32_t* stop_val
        int32_t* traceb
        int32_t* tracef
        int32_t* star_ptr
        uint8_t* type
        uint8_t* edge
        uint8_t* elim
        uint8_t* rbs
        int8_t* strand
        int8_t* ov_mark
        float* gc_cont
        double* cscore
        double* sscore
        double* rscore
        double* uscore
        double* tscore
        double* score
        double* mot_score
        int32_t* mot_ndx
        uint8_t* mot_len
        uint8_t* mot_spacer
        uint8_t* mot_spacendx
    ctypedef struct pga_contig_result:
        int32_t model
        int32_t n_nodes
        int64_t gene_begin
        int32_t n_genes
        int32_t n_unknown
        double gc
        double score
    ctypedef struct pga_result:
        int32_t n_contigs
        int64_t n_genes
        pga_contig_result* contigs
        pga_gene* genes
        pga_nodes* nodes
        double t_total_ms
        double t_dp_ms
        int64_t node_passes
        int32_t n_chains
        int32_t* mask_off
        int32_t* masks
    int PGA_OK, PGA_EINVAL, PGA_ENOMEM, PGA_EDEVICE, PGA_ENODEVICE
    int pga_create(int device, pga_ctx** out)
    void pga_destroy(pga_ctx*)
    const char* pga_last_error(const pga_ctx*)
    int pga_set_models(pga_ctx*, const pga_training* const* models, int n_models)
    int pga_find_genes_batch(pga_ctx*, int32_t n, const char* const* seqs, const int64_t* lens,
                             const pga_params*, pga_result** out)
    void pga_result_free(pga_result*)
    int pga_find_genes(pga_ctx*, const pga_batch*, const pga_params*, pga_result** out)
    int pga_find_genes_models(pga_ctx*, const pga_batch*, const pga_params*, const int32_t* model_of_contig, pga_result** out)
    int pga_translate_genes(pga_ctx*, const pga_batch*, int64_t n_genes, const pga_gene* genes, const int32_t* table_of_contig,
                            int unknown_residue, int include_stop, int strict, const int64_t* offsets, char* out)
    int pga_batch_create(pga_ctx*, int32_t n, const char* const* seqs, const int64_t* lens, pga_batch** out)
    int pga_batch_create_device(pga_ctx*, int32_t n, const void* d_data, int64_t n_elems, int32_t elem_bytes, const int64_t* elem_off,
                                const int64_t* lens, const uint8_t* alphabet, int32_t n_alphabet, void* producer_stream, pga_batch** out)
    int pga_batch_read(pga_ctx*, const pga_batch*, int32_t contig, char* out)
    void pga_batch_free(pga_batch*)
    int pga_batch_set_regions(pga_batch*, const int32_t* off, const int32_t* iv)
    int pga_batch_set_mask_case(pga_batch*, int lower_case)
    int pga_batch_set_circular(pga_batch*, const uint8_t* circular)
    int pga_circular_cuts(const pga_ctx*, int32_t n, int32_t* out)
    int pga_batch_set_sets(pga_batch*, const int32_t* set_of_contig)
    int pga_set_choice(const pga_ctx*, int32_t n, int32_t* model, double* score)
    int pga_model_scores(const pga_ctx*, int32_t n_contigs, int32_t n_models, double* out)
    int pga_circular_cut(int32_t L, int32_t n, const int32_t* begin, const int32_t* end)
    int pga_batch_terminal_repeats(pga_ctx*, const pga_batch*, const uint8_t* search, int32_t min_length, int32_t max_length,
                                   int32_t max_base_percent, int32_t* match_out, int32_t* trim_out)
    int pga_batch_trim_terminal_repeats(pga_ctx*, const pga_batch* src, const int32_t* trim, pga_batch** out)
    int pga_terminal_repeat_chunk()
    int pga_batch_replicate(pga_ctx*, const pga_batch* src, int32_t n, const int32_t* contig_of_entry, pga_batch** out)
    int pga_find_coding_bases(pga_ctx*, const pga_batch*, const pga_params*, const int32_t* model_of_contig, int64_t* coding_bases,
                              int32_t* n_genes, double* score)
    int PGA_STAGE_EXTRACT, PGA_STAGE_SCORE, PGA_STAGE_OVERLAP, PGA_STAGE_SEQUENCE
    int pga_nodes_stage(pga_ctx*, const pga_batch*, const pga_params*, int stage, int translation_table, pga_result** out)
    int pga_train(pga_ctx*, const pga_batch*, const pga_params*, int translation_table, double start_weight, int force_nonsd,
                  int upto, pga_training* out)
    int pga_train_batch(pga_ctx*, const pga_batch*, const pga_params*, const int32_t* translation_table, const double* start_weight,
                        const int32_t* force_nonsd, int upto, pga_training* out, int32_t* status)
    int pga_score_connections(pga_ctx*, int32_t n, const int32_t* ndx, const int32_t* stop_val, const uint8_t* type,
                              const int8_t* strand, const double* cscore, const double* sscore, const double* rscore,
                              const double* uscore, const int32_t* star_ptr, double st_wt, int final,
                              double* score, int32_t* traceb, int8_t* ov_mark, int32_t* max_index, double* kernel_ms)
    int pga_score_connections_training(pga_ctx*, int32_t n, const int32_t* ndx, const int32_t* stop_val, const uint8_t* type,
                                       const int8_t* strand, const double* gc_score, const double* bias, const int32_t* star_ptr,
                                       double st_wt, double* score, int32_t* traceb, int8_t* ov_mark, int32_t* max_index,
                                       double* kernel_ms)

# --- constants (ref: lib.pyx:166-228) ------------------------------------------------------
MIN_SINGLE_GENOME = 20000
IDEAL_SINGLE_GENOME = 100000
TRANSLATION_TABLES = frozenset(set(range(1, 7)) | set(range(9, 17)) | set(range(21, 27)) | {29, 30, 32, 33})
PRODIGAL_VERSION = "v2.6.3+c1e2d36"
from pyrodigal_amd import __version__ as _VERSION      # one definition: the package's
from pyrodigal_amd import tables as _tables
from pyrodigal_amd.tables import TableSelection
from pyrodigal_amd._cabi import DeviceSequences as _DeviceSequences     # sequences that already lie in device memory
from pyrodigal_amd import _cabi                                          # proteins left there as token ids (ProteinTokens, tokens_into)
TRAINING_INFO_SIZE = 558392
# select_translation_table: the most models (TrainingInfo, 558 392 bytes each) one device call loads
_SELECT_MAX_MODELS = 256

_RBS_MOTIF = [
    None, "GGA/GAG/AGG", "3Base/5BMM", "4Base/6BMM", "AGxAG", "AGxAG", "GGA/GAG/AGG", "GGxGG", "GGxGG",
    "AGxAG", "AGGAG(G)/GGAGG", "AGGA/GGAG/GAGG", "AGGA/GGAG/GAGG", "GGA/GAG/AGG", "GGxGG", "AGGA",
    "GGAG/GAGG", "AGxAGG/AGGxGG", "AGxAGG/AGGxGG", "AGxAGG/AGGxGG", "AGGAG/GGAGG", "AGGAG", "AGGAG",
    "GGAGG", "GGAGG", "AGGAGG", "AGGAGG", "AGGAGG",
]
_RBS_SPACER = [
    None, "3-4bp", "13-15bp", "13-15bp", "11-12bp", "3-4bp", "11-12bp", "11-12bp", "3-4bp", "5-10bp",
    "13-15bp", "3-4bp", "11-12bp", "5-10bp", "5-10bp", "5-10bp", "5-10bp", "11-12bp", "3-4bp", "5-10bp",
    "11-12bp", "3-4bp", "5-10bp", "3-4bp", "5-10bp", "11-12bp", "3-4bp", "5-10bp",
]
_NODE_TYPE = ["ATG", "GTG", "TTG", "Edge"]

# NCBI genetic codes in TCAG order: one definition, shared with the pure-Python rules (tables.NCBI_CODES)
_NCBI_CODES = _tables.NCBI_CODES


def _digit_order_table(str code):
    """Re-index a TCAG-ordered code by the digit alphabet used on the device (A0 G1 C2 T3)."""
    ncbi = (2, 3, 1, 0)     # digit -> position in TCAG
    return "".join(code[ncbi[a] * 16 + ncbi[b] * 4 + ncbi[c]] for a in range(4) for b in range(4) for c in range(4)).encode("ascii")

_CODE_BY_DIGITS = {tt: _digit_order_table(code) for tt, code in _NCBI_CODES.items()}
_DIGIT_OF = bytes(0 if c in b"Aa" else 1 if c in b"Gg" else 2 if c in b"Cc" else 3 if c in b"Tt" else 6 for c in range(256))


cdef bint _codon_is_stop(int x0, int x1, int x2, int tt) noexcept nogil:       # ref: _sequence.h:19-43
    if x0 == 0 and tt == 2:
        return x1 == 1 and (x2 == 0 or x2 == 1)                                  # AGA / AGG
    if x0 != 3:
        return False
    if x1 == 0 and x2 == 1:                                                      # TAG
        return tt in (1, 2, 3, 4, 5, 9, 10, 11, 12, 13, 14, 21, 23, 24, 25, 26, 33)
    if x1 == 1 and x2 == 0:                                                      # TGA
        return tt in (1, 6, 11, 12, 15, 16, 22, 23, 26, 29, 30, 32)
    if x1 == 0 and x2 == 0:                                                      # TAA
        return tt in (1, 2, 3, 4, 5, 9, 10, 11, 12, 13, 15, 16, 21, 22, 23, 24, 25, 26, 32)
    if tt == 22:
        return x1 == 2 and x2 == 0                                               # TCA
    if tt == 23:
        return x1 == 3 and x2 == 0                                               # TTA
    return False


cdef bint _codon_is_start(int x0, int x1, int x2, int tt) noexcept nogil:      # ref: _sequence.h:45-73
    if x1 != 3 or x2 != 1:
        return False
    if x0 == 0:
        return True
    if tt in (6, 10, 14, 15, 16, 2):
        return False
    if x0 == 1:
        return not (tt == 1 or tt == 3 or tt == 12 or tt == 2)
    if x0 == 3:
        return not (tt < 4 or tt == 9 or (21 <= tt < 25))
    return False


def _stop_codon_set(int tt):
    return frozenset((a, b, c) for a in range(4) for b in range(4) for c in range(4) if _codon_is_stop(a, b, c, tt))

_STOP_CODONS = {tt: _stop_codon_set(tt) for tt in _NCBI_CODES}
_COMPLEMENT = bytes.maketrans(b"ACGTN", b"TGCAN")
_COMPLEMENT_ANY = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


cdef object _raise_for(pga_ctx* ctx, int rc, str what):
    cdef bytes msg = pga_last_error(ctx) if ctx != NULL else b""
    text = "%s: %s" % (what, msg.decode("utf-8", "replace"))
    if rc == PGA_EINVAL:
        raise ValueError(text)
    if rc == PGA_ENOMEM:
        raise MemoryError(text)
    if rc == PGA_ENODEVICE:
        raise RuntimeError(what + ": no gfx950 (MI355X) device visible; pyrodigal_amd has no CPU fallback")
    raise RuntimeError(text)


# --- TrainingInfo / MetagenomicBins (ref: lib.pyx:3898-4282, 4888-5069) -------------------
cdef class TrainingInfo:
    """The parameters of one gene model: the reference's 558 392-byte ``struct _training``."""
    cdef object _raw              # numpy uint8[558392]; `raw` hands out a read-only view
    cdef readonly unsigned long long _version   # bumped by every setter: device copies of the model are reloaded when it moves

    def __init__(self, double gc=0.5, *, int translation_table=11, double start_weight=4.35, object raw=None):
        if raw is not None:
            arr = np.frombuffer(bytes(raw), dtype=np.uint8).copy()
            if arr.size != TRAINING_INFO_SIZE:
                raise ValueError("a raw training info must be %d bytes (got %d)" % (TRAINING_INFO_SIZE, arr.size))
            self._raw = arr
        else:
            if translation_table not in TRANSLATION_TABLES:
                raise ValueError("%d is not a valid translation table index" % translation_table)
            self._raw = np.zeros(TRAINING_INFO_SIZE, dtype=np.uint8)
            self._f64(0)[0] = gc
            self._i32(8)[0] = translation_table
            self._f64(16)[0] = start_weight
            self._i32(72)[0] = 1

    @classmethod
    def load(cls, fp):
        """Load a training info from a file object or path (raw dump, optionally gzipped) -- ref: lib.pyx:3910-3953."""
        if hasattr(fp, "read"):
            data = fp.read()
        else:
            opener = gzip.open if str(fp).endswith(".gz") else open
            with opener(fp, "rb") as f:
                data = f.read()
        if len(data) != TRAINING_INFO_SIZE:
            raise EOFError("Expected %d bytes, only read %d" % (TRAINING_INFO_SIZE, len(data)))
        return cls(raw=data)

    def dump(self, fp):
        """Write the raw structure to a file object -- ref: lib.pyx:4865-4885."""
        fp.write(self._raw.tobytes())

    @property
    def raw(self):
        """The 558 392 bytes of the structure, read-only: the setters are what tells a device copy of the model that it is stale."""
        v = self._raw.view()
        v.setflags(write=False)
        return v

    def _f64(self, int off, int n=1):
        return self._raw[off:off + 8 * n].view(np.float64)

    def _i32(self, int off):
        return self._raw[off:off + 4].view(np.int32)

    def __repr__(self):
        return "<pyrodigal_amd.lib.TrainingInfo gc=%r start_weight=%r translation_table=%r uses_sd=%r>" % (
            self.gc, self.start_weight, self.translation_table, self.uses_sd)

    @property
    def gc(self):
        return float(self._f64(0)[0])

    @gc.setter
    def gc(self, double v):
        self._version += 1
        if v < 0 or v > 1:
            raise ValueError("Invalid GC percent: %r" % v)
        self._f64(0)[0] = v

    @property
    def translation_table(self):
        return int(self._i32(8)[0])

    @translation_table.setter
    def translation_table(self, int v):
        self._version += 1
        if v not in TRANSLATION_TABLES:
            raise ValueError("%d is not a valid translation table index" % v)
        self._i32(8)[0] = v

    @property
    def start_weight(self):
        return float(self._f64(16)[0])

    @property
    def bias(self):
        return tuple(self._f64(24, 3))

    @property
    def type_weights(self):
        return tuple(self._f64(48, 3))

    @property
    def uses_sd(self):
        return bool(self._i32(72)[0])

    @property
    def rbs_weights(self):
        return self._f64(80, 28).copy()

    @property
    def missing_motif_weight(self):
        return float(self._f64(525616)[0])

    @property
    def coding_statistics(self):
        return self._f64(525624, 4096).copy()

    # the remaining fields and the setters of the reference (ref: lib.pyx:4067-4213)
    @start_weight.setter
    def start_weight(self, double v):
        self._version += 1
        self._f64(16)[0] = v

    @bias.setter
    def bias(self, object v):
        self._version += 1
        self._f64(24, 3)[:] = np.asarray(v, np.float64)

    @type_weights.setter
    def type_weights(self, object v):
        self._version += 1
        self._f64(48, 3)[:] = np.asarray(v, np.float64)

    @uses_sd.setter
    def uses_sd(self, bint v):
        self._version += 1
        self._i32(72)[0] = 1 if v else 0

    @rbs_weights.setter
    def rbs_weights(self, object v):
        self._version += 1
        self._f64(80, 28)[:] = np.asarray(v, np.float64)

    @property
    def upstream_compositions(self):
        return self._f64(304, 128).reshape(32, 4).copy()

    @upstream_compositions.setter
    def upstream_compositions(self, object v):
        self._version += 1
        self._f64(304, 128)[:] = np.asarray(v, np.float64).reshape(-1)

    @property
    def motif_weights(self):
        return self._f64(1328, 65536).reshape(4, 4, 4096).copy()

    @motif_weights.setter
    def motif_weights(self, object v):
        self._version += 1
        self._f64(1328, 65536)[:] = np.asarray(v, np.float64).reshape(-1)

    @missing_motif_weight.setter
    def missing_motif_weight(self, double v):
        self._version += 1
        self._f64(525616)[0] = v

    @coding_statistics.setter
    def coding_statistics(self, object v):
        self._version += 1
        self._f64(525624, 4096)[:] = np.asarray(v, np.float64).reshape(-1)

    def __eq__(self, other):
        return isinstance(other, TrainingInfo) and np.array_equal(self._raw, (<TrainingInfo> other)._raw)

    def __reduce__(self):           # pickling (ref: lib.pyx:4024-4035)
        return _training_info_from_bytes, (self._raw.tobytes(),)


def _training_info_from_bytes(bytes raw):
    return TrainingInfo(raw=raw)


cdef class MetagenomicBin:
    """A pre-trained model with a description (ref: lib.pyx:4888-4946)."""
    cdef readonly TrainingInfo training_info
    cdef readonly str description

    def __init__(self, TrainingInfo training_info not None, str description=""):
        self.training_info = training_info
        self.description = description

    def __repr__(self):
        return "<pyrodigal_amd.lib.MetagenomicBin description=%r>" % self.description

    def __reduce__(self):
        return MetagenomicBin, (self.training_info, self.description)


cdef class MetagenomicBins:
    """An immutable collection of `MetagenomicBin` (ref: lib.pyx:4950-5066)."""
    cdef readonly tuple _bins

    def __init__(self, object iterable=()):
        bins = tuple(iterable)
        for b in bins:
            if not isinstance(b, MetagenomicBin):
                raise TypeError("expected MetagenomicBin, got %s" % type(b).__name__)
        self._bins = bins

    def __len__(self):
        return len(self._bins)

    def __getitem__(self, index):
        if isinstance(index, slice):
            return MetagenomicBins(self._bins[index])
        return self._bins[index]

    def __iter__(self):
        return iter(self._bins)

    def __reduce__(self):
        return MetagenomicBins, (list(self._bins),)


# Prodigal's 50 built-in models are not part of the reference checkout (un-vendored submodule), so the
# default collection is empty: meta mode needs `metagenomic_bins=`.
METAGENOMIC_BINS = MetagenomicBins()


# --- Sequence / Nodes / Gene / Genes ----------------------------------------------------------

cdef class _StageContext:
    """One lazily created device context for the stage-level calls (`Nodes.*`, `ConnectionScorer`, `Sequence`)."""
    cdef pga_ctx* ctx
    cdef object loaded        # the TrainingInfo blob currently loaded as model 0
    cdef unsigned long long loaded_version

    def __cinit__(self):
        self.ctx = NULL
        self.loaded = None

    def __dealloc__(self):
        if self.ctx != NULL:
            pga_destroy(self.ctx)
            self.ctx = NULL

    cdef int ensure(self) except -1:
        cdef int rc
        if self.ctx == NULL:
            rc = pga_create(0, &self.ctx)
            if rc != PGA_OK:
                self.ctx = NULL
                _raise_for(NULL, rc, "pga_create")
        return 0

    cdef int load(self, TrainingInfo tinf) except -1:
        cdef const pga_training* ptr
        cdef int rc
        if self.loaded is tinf._raw and self.loaded_version == tinf._version:
            return 0
        ptr = <const pga_training*> <size_t> tinf._raw.ctypes.data
        rc = pga_set_models(self.ctx, &ptr, 1)
        if rc != PGA_OK:
            _raise_for(self.ctx, rc, "pga_set_models")
        self.loaded = tinf._raw
        self.loaded_version = tinf._version
        return 0


cdef class _StagePool:
    """The stage-level calls are re-entrant like the reference's (each builds private state, ref: lib.pyx:2528-2595): a caller takes
    a context of its own for the duration of its device call -- up to `limit` contexts (one HIP stream and one set of scratch
    buffers each), created on demand -- so that concurrent callers overlap instead of queueing behind one lock."""
    cdef list idle
    cdef int created, limit
    cdef object cv

    def __cinit__(self):
        self.idle = []
        self.created = 0
        self.limit = 3
        self.cv = threading.Condition(threading.Lock())

    cdef _StageContext take(self, TrainingInfo want=None):
        cdef _StageContext s
        cdef ssize_t k
        with self.cv:
            while True:
                if self.idle:
                    # prefer a context that already holds the model the caller is about to use
                    k = len(self.idle) - 1
                    if want is not None:
                        for j in range(len(self.idle)):
                            s = self.idle[j]
                            if s.loaded is want._raw and s.loaded_version == want._version:
                                k = j
                                break
                    return self.idle.pop(k)
                if self.created < self.limit:
                    self.created += 1
                    return _StageContext()
                self.cv.wait()

    cdef void give(self, _StageContext s):
        with self.cv:
            self.idle.append(s)
            self.cv.notify()

cdef _StagePool _STAGES = _StagePool()

cdef class _StageLease:
    """`with _StageLease(tinf) as S:` -- a stage context of the caller's own for one device call."""
    cdef _StageContext s
    cdef TrainingInfo want

    def __cinit__(self, TrainingInfo want=None):
        self.want = want
        self.s = None

    def __enter__(self):
        self.s = _STAGES.take(self.want)
        return self.s

    def __exit__(self, *exc):
        _STAGES.give(self.s)
        self.s = None
        return False



cdef class Mask:
    """A masked region `[begin, end)` of a sequence (ref: lib.pyx:283-340)."""
    cdef readonly int begin
    cdef readonly int end

    def __init__(self, int begin, int end):
        self.begin = begin
        self.end = end

    def __repr__(self):
        return "<pyrodigal_amd.lib.Mask begin=%d end=%d>" % (self.begin, self.end)

    def __eq__(self, other):
        return isinstance(other, Mask) and (self.begin, self.end) == ((<Mask> other).begin, (<Mask> other).end)

    cpdef bint intersects(self, int begin, int end):
        """Whether the mask intersects the sequence coordinates `[begin, end)` (ref: lib.pyx:344-365)."""
        return self.begin < end and begin < self.end


cdef tuple _interval_of(object m):
    """`(begin, end)` of a `Mask` or of a pair."""
    if isinstance(m, Mask):
        return ((<Mask> m).begin, (<Mask> m).end)
    b, e = m
    return (int(b), int(e))


cdef class Masks:
    """A list of masked regions `[begin, end)` of a sequence (ref: lib.pyx:368-560): what `Sequence.masks` returns, and the type
    regions are handed over in (`Sequence(..., regions=)`, `GeneFinder.find_genes(..., regions=)`).  Built from any iterable of
    `Mask` objects or `(begin, end)` pairs; equal to a `Masks`, list or tuple of the same intervals in the same order."""
    cdef list _items            # (begin, end) tuples

    def __cinit__(self):
        self._items = []

    def __init__(self, object iterable=()):
        self._items = [_interval_of(m) for m in iterable]

    def __len__(self):
        return len(self._items)

    def __getitem__(self, index):
        if isinstance(index, slice):
            return Masks(self._items[index])
        cdef ssize_t i = index
        if i < 0:
            i += len(self._items)
        if i < 0 or i >= len(self._items):
            raise IndexError("masks index out of range")
        return Mask(self._items[i][0], self._items[i][1])

    def __iter__(self):
        for b, e in self._items:
            yield Mask(b, e)

    def __bool__(self):
        return len(self._items) > 0

    def __eq__(self, other):
        if isinstance(other, Masks):
            return self._items == (<Masks> other)._items
        if isinstance(other, (list, tuple)):
            try:
                return self._items == [_interval_of(m) for m in other]
            except (TypeError, ValueError):
                return False
        return NotImplemented

    def __repr__(self):
        return "pyrodigal_amd.lib.Masks(%r)" % (self._items,)

    def __copy__(self):
        return self.copy()

    def __reduce__(self):
        return Masks, (list(self._items),)

    cpdef Masks copy(self):
        """A copy of the list."""
        return Masks(self._items)

    def clear(self):
        """Remove every mask."""
        self._items = []

    def intersects(self, int begin, int end):
        """Whether any mask of the list intersects `[begin, end)`."""
        for b, e in self._items:
            if b < end and begin < e:
                return True
        return False


cdef object _check_regions(object regions, ssize_t length, str which):
    """The caller's regions of one sequence as an int32 array [k][2], or None for none: every interval must satisfy
    0 <= begin < end <= length (`which` names the sequence in the message)."""
    if regions is None:
        return None
    cdef list iv = [_interval_of(m) for m in regions]
    if not iv:
        return None
    for b, e in iv:
        if not (0 <= b < e <= length):
            raise ValueError("%sregion [%d, %d) is not a non-empty part of the sequence [0, %d)" % (which, b, e, length))
    return np.array(iv, dtype=np.int32).reshape(-1, 2)


cdef int _attach_masks(pga_ctx* ctx, pga_batch* batch, list seqs, bint lower_case) except -1:
    """The regions the sequences carry and the lower-case rule go to the resident batch (nothing to do: no call at all)."""
    cdef Py_ssize_t n = len(seqs), i
    cdef bint any_regions = False
    cdef size_t p_off, p_iv
    cdef int rc
    for i in range(n):
        if (<Sequence> seqs[i])._regions is not None:
            any_regions = True
            break
    if any_regions:
        off = np.zeros(n + 1, np.int32)
        parts = []
        for i in range(n):
            r = (<Sequence> seqs[i])._regions
            off[i + 1] = off[i] + (0 if r is None else len(r))
            if r is not None:
                parts.append(r)
        iv = np.ascontiguousarray(np.concatenate(parts), dtype=np.int32)
        p_off = off.ctypes.data; p_iv = iv.ctypes.data
        rc = pga_batch_set_regions(batch, <const int32_t*> p_off, <const int32_t*> p_iv)
        if rc != PGA_OK:
            _raise_for(ctx, rc, "pga_batch_set_regions")
    if lower_case:
        rc = pga_batch_set_mask_case(batch, 1)
        if rc != PGA_OK:
            _raise_for(ctx, rc, "pga_batch_set_mask_case")
    return 0


def _sequence_from_state(data, mask, mask_size, regions, mask_lowercase):
    return Sequence(data, mask, mask_size, regions=regions, mask_lowercase=mask_lowercase)


cdef class Sequence:
    """The input as ASCII bytes.  Digitising, GC content, the unknown-base count and the masked regions are
    computed on the device (ref: lib.pyx:664-713), on first use.

    Masked regions come from up to three sources, and `masks` is their union (sorted, disjoint, touching intervals joined): runs
    of unknown bases of at least `mask_size` (`mask=True`), runs of lower-case letters by the same rule (`mask_lowercase=True`),
    and `regions`, the caller's own `[begin, end)` intervals (0-based; any order, overlaps allowed, no minimum length).  A region
    takes part in the mask test exactly as a masked run of `N` at the same coordinates would; its bases keep their identity for
    everything else."""
    cdef readonly bytes data
    cdef readonly bint mask
    cdef readonly size_t mask_size
    cdef readonly bint mask_lowercase
    cdef object _regions        # int32 [k][2] (k > 0) or None
    cdef double _gc
    cdef ssize_t _unknown
    cdef list _masks

    def __init__(self, object sequence, bint mask=False, size_t mask_size=50, *, object regions=None, bint mask_lowercase=False):
        if isinstance(sequence, Sequence):
            self.data = (<Sequence> sequence).data
        elif type(sequence) is bytes:
            self.data = sequence                      # immutable: no copy
        elif isinstance(sequence, str):
            self.data = sequence.encode("ascii", "replace")
        else:
            self.data = bytes(memoryview(sequence))
        self.mask = mask
        self.mask_size = mask_size
        self.mask_lowercase = mask_lowercase
        if regions is None and isinstance(sequence, Sequence):
            self._regions = (<Sequence> sequence)._regions
        else:
            self._regions = _check_regions(regions, len(self.data), "")
        self._gc = -1.0
        self._unknown = -1
        self._masks = None

    def __len__(self):
        return len(self.data)

    def __str__(self):
        up = self.data.upper()
        return "".join(chr(c) if c in b"ACGT" else "N" for c in up)

    cdef int _build(self) except -1:
        cdef pga_params p
        cdef pga_batch* batch = NULL
        cdef pga_result* res = NULL
        cdef const char* ptr = PyBytes_AS_STRING(self.data)
        cdef int64_t length = len(self.data)
        cdef int rc, k
        cdef _StageContext S
        if self._unknown >= 0:
            return 0
        p.closed = 0; p.min_gene = 90; p.min_edge_gene = 60; p.max_overlap = 60; p.meta = 0; p.want_nodes = 0
        p.mask = self.mask; p.min_mask = <int32_t> self.mask_size
        with _StageLease() as S:
            S.ensure()
            rc = pga_batch_create(S.ctx, 1, &ptr, &length, &batch)
            if rc != PGA_OK:
                _raise_for(S.ctx, rc, "pga_batch_create")
            try:
                _attach_masks(S.ctx, batch, [self], self.mask_lowercase)
                with nogil:
                    rc = pga_nodes_stage(S.ctx, batch, &p, PGA_STAGE_SEQUENCE, 11, &res)
                if rc != PGA_OK:
                    _raise_for(S.ctx, rc, "pga_nodes_stage")
                try:
                    self._gc = res.contigs[0].gc
                    self._unknown = res.contigs[0].n_unknown
                    self._masks = []
                    if res.mask_off != NULL:
                        for k in range(res.mask_off[0], res.mask_off[1]):
                            self._masks.append(Mask(res.masks[2 * k], res.masks[2 * k + 1]))
                finally:
                    pga_result_free(res)
            finally:
                pga_batch_free(batch)
        return 0

    @property
    def gc(self):
        """GC fraction over all bases (ref: lib.pyx:596-600)."""
        self._build()
        return self._gc

    @property
    def unknown(self):
        """Number of bases that are not A, C, G or T (ref: lib.pyx:602-606)."""
        self._build()
        return self._unknown

    @property
    def gc_known(self):
        """GC fraction over the known bases (ref: lib.pyx:608-614)."""
        self._build()
        cdef ssize_t n = len(self.data)
        cdef double gc_count = round(self._gc * <double> n)      # the device returns count / length; the count is recovered exactly
        return gc_count / (<double> n - <double> self._unknown) if n > self._unknown else 0.0

    @property
    def masks(self):
        """The masked regions: the union of every source, empty when none is set (ref: lib.pyx:616-620)."""
        self._build()
        return Masks(self._masks)

    @property
    def regions(self):
        """The caller's own regions as they were given (`Masks`), or None."""
        return None if self._regions is None else Masks(self._regions.tolist())

    def __reduce__(self):
        if self._regions is None and not self.mask_lowercase:
            return Sequence, (self.data, self.mask, self.mask_size)
        return _sequence_from_state, (self.data, self.mask, self.mask_size,
                                      None if self._regions is None else [tuple(x) for x in self._regions.tolist()], self.mask_lowercase)


cdef class Node:
    """A read-only view of one node (ref: lib.pyx:1437-1552)."""
    cdef readonly Nodes owner
    cdef readonly ssize_t i

    def __getattr__(self, name):
        arr = self.owner._f.get(name)
        if arr is None:
            raise AttributeError(name)
        v = arr[self.i]
        return v.item() if hasattr(v, "item") and getattr(v, "ndim", 0) == 0 else v

    @property
    def index(self):
        return int(self.owner._f["ndx"][self.i])

    @property
    def type(self):
        return _NODE_TYPE[3 if self.owner._f["edge"][self.i] else int(self.owner._f["type"][self.i])] if self.owner._f["type"][self.i] != 3 else "Stop"


cdef class Nodes:
    """The nodes of one sequence as struct-of-arrays (ref: lib.pyx:1652-1795, 2501-2595)."""
    cdef readonly dict _f
    cdef dict _extract_kw      # the arguments of the last extract(), which score() has to repeat

    def __init__(self):
        self._f = {}
        self._extract_kw = None

    def __len__(self):
        return len(self._f["ndx"]) if "ndx" in self._f else 0

    def __getitem__(self, ssize_t i):
        cdef ssize_t n = len(self)
        if i < 0:
            i += n
        if i < 0 or i >= n:
            raise IndexError("node index out of range")
        cdef Node nd = Node.__new__(Node)
        nd.owner = self
        nd.i = i
        return nd

    def array(self, str name):
        """The numpy array of one field (ndx, stop_val, type, strand, edge, cscore, sscore, ...)."""
        return self._f[name]

    def copy(self):
        """A deep copy (ref: lib.pyx:2514-2526)."""
        cdef Nodes out = Nodes()
        out._f = {k: v.copy() for k, v in self._f.items()}
        out._extract_kw = None if self._extract_kw is None else dict(self._extract_kw)
        return out

    def clear(self):
        """Remove all nodes (ref: lib.pyx:2501-2512)."""
        self._f = {}
        self._extract_kw = None

    cdef object _run_stage(self, Sequence seq, int stage, TrainingInfo tinf, bint is_meta):
        cdef pga_params p
        cdef pga_batch* batch = NULL
        cdef pga_result* res = NULL
        cdef const char* ptr = PyBytes_AS_STRING(seq.data)
        cdef int64_t length = len(seq.data)
        cdef int rc, tt
        cdef _StageContext S
        kw = self._extract_kw
        p.closed = kw["closed"]; p.min_gene = kw["min_gene"]; p.min_edge_gene = kw["min_edge_gene"]
        p.max_overlap = 60; p.meta = is_meta; p.want_nodes = 1
        p.mask = seq.mask; p.min_mask = <int32_t> seq.mask_size
        tt = kw["translation_table"]
        with _StageLease(tinf) as S:
            S.ensure()
            if tinf is not None:
                S.load(tinf)
            rc = pga_batch_create(S.ctx, 1, &ptr, &length, &batch)
            if rc != PGA_OK:
                _raise_for(S.ctx, rc, "pga_batch_create")
            try:
                _attach_masks(S.ctx, batch, [seq], seq.mask_lowercase)
                with nogil:
                    rc = pga_nodes_stage(S.ctx, batch, &p, stage, tt, &res)
                if rc != PGA_OK:
                    _raise_for(S.ctx, rc, "pga_nodes_stage")
                try:
                    return _copy_nodes(&res.nodes[0])
                finally:
                    pga_result_free(res)
            finally:
                pga_batch_free(batch)

    def extract(self, Sequence sequence not None, *, bint closed=False, int min_gene=90, int min_edge_gene=60,
                int translation_table=11):
        """Extract the nodes of `sequence`, in sorted order (ref: lib.pyx:2528-2560); returns how many were added."""
        if translation_table not in TRANSLATION_TABLES:
            raise ValueError("%d is not a valid translation table index" % translation_table)
        self._extract_kw = dict(closed=closed, min_gene=min_gene, min_edge_gene=min_edge_gene, translation_table=translation_table)
        cdef Nodes got = self._run_stage(sequence, PGA_STAGE_EXTRACT, None, False)
        self._f = got._f
        return len(self)

    def sort(self):
        """Sort by position then strand (ref: lib.pyx:2575-2580): the device extraction already emits that order."""
        return None

    def reset_scores(self):
        """Reset every score and DP field (ref: lib.pyx:2562-2573)."""
        cdef ssize_t n = len(self)
        for k in ("cscore", "sscore", "rscore", "uscore", "tscore", "score", "mot_score"):
            self._f[k] = np.zeros(n, np.float64)
        self._f["star_ptr"] = np.zeros((n, 3), np.int32)
        self._f["rbs"] = np.zeros((n, 2), np.uint8)
        for k in ("traceb", "tracef"):
            self._f[k] = np.full(n, -1, np.int32)
        self._f["ov_mark"] = np.full(n, -1, np.int8)
        self._f["elim"] = np.zeros(n, np.uint8)
        self._f["mot_ndx"] = np.zeros(n, np.int32)
        for k in ("mot_len", "mot_spacer", "mot_spacendx"):
            self._f[k] = np.zeros(n, np.uint8)

    def score(self, Sequence sequence not None, TrainingInfo training_info not None, *, bint closed=False, bint is_meta=False):
        """Score the start nodes with `training_info` (ref: lib.pyx:2582-2595).

        The device scores the nodes it extracts itself, so `sequence` and the extraction options must be
        the ones `extract` was called with (the reference has the same precondition)."""
        if self._extract_kw is None:
            raise RuntimeError("Nodes.score needs nodes from Nodes.extract")
        if self._extract_kw["translation_table"] != training_info.translation_table:
            raise ValueError("nodes were extracted with translation table %d, the training info uses %d"
                             % (self._extract_kw["translation_table"], training_info.translation_table))
        if self._extract_kw["closed"] != closed:
            raise ValueError("`closed` differs from the value used by Nodes.extract")
        cdef Nodes got = self._run_stage(sequence, PGA_STAGE_SCORE, training_info, is_meta)
        if len(got) != len(self) or not np.array_equal(got._f["ndx"], self._f["ndx"]):
            raise ValueError("sequence does not match the nodes held by this object")
        keep = {k: self._f[k] for k in ("traceb", "tracef", "ov_mark", "score", "elim", "star_ptr") if k in self._f}
        self._f = got._f
        self._f.update(keep)


cdef class ConnectionScorer:
    """Connection scoring of a whole sorted node list on the device (ref: lib.pyx:1297-1435).

    The reference scores one node at a time (`compute_skippable(min, i)` + `score_connections(nodes, min,
    i, tinf, final)`); a GPU needs the whole array, so `score_connections(nodes, tinf, final=True)` runs the
    complete dynamic-programming pass with the reference's window rule and writes `score`, `traceb` and
    `ov_mark` of every node.  `index` and `compute_skippable` are kept so that call sites read the same."""
    cdef readonly str backend
    cdef Nodes _indexed

    def __init__(self, str backend="detect"):
        if backend not in ("detect", "hip"):
            raise ValueError("unsupported backend %r: this build only has the HIP (gfx950) backend" % backend)
        self.backend = "hip"
        self._indexed = None

    def index(self, Nodes nodes not None):
        self._indexed = nodes

    def compute_skippable(self, int min, int i):
        return None     # the skip conditions (impl/generic.h:29-36) are folded into the device scorer

    def score_connections(self, Nodes nodes not None, TrainingInfo training_info not None, bint final=False):
        cdef ssize_t n = len(nodes)
        cdef int rc
        cdef int32_t mi = -1
        f = nodes._f
        if "cscore" not in f:
            nodes.reset_scores()
        if not final:
            return self._score_connections_training(nodes, training_info)
        cdef object ndx = np.ascontiguousarray(f["ndx"], np.int32), stop_val = np.ascontiguousarray(f["stop_val"], np.int32)
        cdef object typ = np.ascontiguousarray(f["type"], np.uint8), strand = np.ascontiguousarray(f["strand"], np.int8)
        cdef object cs = np.ascontiguousarray(f["cscore"], np.float64), ss = np.ascontiguousarray(f["sscore"], np.float64)
        cdef object rs = np.ascontiguousarray(f["rscore"], np.float64), us = np.ascontiguousarray(f["uscore"], np.float64)
        cdef object sp = np.ascontiguousarray(f["star_ptr"], np.int32)
        cdef object score = np.zeros(n, np.float64), traceb = np.full(n, -1, np.int32), ov = np.full(n, -1, np.int8)
        cdef size_t p_ndx = ndx.ctypes.data, p_stop = stop_val.ctypes.data, p_typ = typ.ctypes.data, p_strand = strand.ctypes.data
        cdef size_t p_cs = cs.ctypes.data, p_ss = ss.ctypes.data, p_rs = rs.ctypes.data, p_us = us.ctypes.data, p_sp = sp.ctypes.data
        cdef size_t p_score = score.ctypes.data, p_tb = traceb.ctypes.data, p_ov = ov.ctypes.data
        cdef double st_wt = training_info.start_weight
        cdef _StageContext S
        with _StageLease() as S:
            S.ensure()
            with nogil:
                rc = pga_score_connections(S.ctx, <int32_t> n, <const int32_t*> p_ndx, <const int32_t*> p_stop,
                                           <const uint8_t*> p_typ, <const int8_t*> p_strand, <const double*> p_cs,
                                           <const double*> p_ss, <const double*> p_rs, <const double*> p_us,
                                           <const int32_t*> p_sp, st_wt, 1, <double*> p_score, <int32_t*> p_tb,
                                           <int8_t*> p_ov, &mi, NULL)
            if rc != PGA_OK:
                _raise_for(S.ctx, rc, "pga_score_connections")
        f["score"] = score; f["traceb"] = traceb; f["ov_mark"] = ov
        return int(mi)

    cdef object _score_connections_training(self, Nodes nodes, TrainingInfo training_info):
        # final = False (the reference's default, ref: lib.pyx:1336-1357): a connection is worth its length times the
        # frame-bias factor bias . gc_score of one of its nodes (ref: _connection.h, `final == false` branches).  Nodes that
        # never went through the training carry gc_score = 0, as in the reference after reset_scores().
        cdef ssize_t n = len(nodes)
        cdef int rc
        cdef int32_t mi = -1
        f = nodes._f
        cdef object ndx = np.ascontiguousarray(f["ndx"], np.int32), stop_val = np.ascontiguousarray(f["stop_val"], np.int32)
        cdef object typ = np.ascontiguousarray(f["type"], np.uint8), strand = np.ascontiguousarray(f["strand"], np.int8)
        cdef object gcs = np.ascontiguousarray(f["gc_score"] if "gc_score" in f else np.zeros((n, 3)), np.float64).reshape(-1)
        cdef object bias = np.ascontiguousarray(training_info.bias, np.float64)
        cdef object sp = np.ascontiguousarray(f["star_ptr"], np.int32)
        cdef object score = np.zeros(n, np.float64), traceb = np.full(n, -1, np.int32), ov = np.full(n, -1, np.int8)
        if gcs.size != 3 * n:
            raise ValueError("`gc_score` must hold three frame scores per node")
        cdef size_t p_ndx = ndx.ctypes.data, p_stop = stop_val.ctypes.data, p_typ = typ.ctypes.data, p_strand = strand.ctypes.data
        cdef size_t p_gcs = gcs.ctypes.data, p_bias = bias.ctypes.data, p_sp = sp.ctypes.data
        cdef size_t p_score = score.ctypes.data, p_tb = traceb.ctypes.data, p_ov = ov.ctypes.data
        cdef double st_wt = training_info.start_weight
        cdef _StageContext S
        with _StageLease() as S:
            S.ensure()
            with nogil:
                rc = pga_score_connections_training(S.ctx, <int32_t> n, <const int32_t*> p_ndx, <const int32_t*> p_stop,
                                                    <const uint8_t*> p_typ, <const int8_t*> p_strand, <const double*> p_gcs,
                                                    <const double*> p_bias, <const int32_t*> p_sp, st_wt, <double*> p_score,
                                                    <int32_t*> p_tb, <int8_t*> p_ov, &mi, NULL)
            if rc != PGA_OK:
                _raise_for(S.ctx, rc, "pga_score_connections_training")
        f["score"] = score; f["traceb"] = traceb; f["ov_mark"] = ov
        return int(mi)


cdef double _confidence(double score, double st_wt) noexcept nogil:   # Prodigal gene.c calculate_confidence
    cdef double r = score / st_wt, conf
    if r < 41:
        conf = exp(r)
        conf = (conf / (conf + 1)) * 100.0
    else:
        conf = 99.99
    return fmax(conf, 50.0)


cdef class Gene:
    """A single predicted gene (ref: lib.pyx:2610-3047)."""
    cdef readonly Genes owner
    cdef pga_gene g
    cdef ssize_t _index        # position in the owner's list (-1: unknown), for the owner's device-side translations

    def __cinit__(self):
        self._index = -1

    @property
    def begin(self):
        return self.g.begin

    @property
    def end(self):
        return self.g.end

    @property
    def strand(self):
        return self.g.strand

    @property
    def partial_begin(self):
        return bool(self.g.partial_begin)

    @property
    def partial_end(self):
        return bool(self.g.partial_end)

    @property
    def start_type(self):
        return _NODE_TYPE[self.g.start_type]

    cdef tuple _rbs(self):
        cdef TrainingInfo t = self.owner.training_info
        w = t._f64(80, 28)
        cdef double st = t.start_weight
        cdef double r1 = w[self.g.rbs[0]] * st, r2 = w[self.g.rbs[1]] * st
        cdef double ms = self.g.mot_score * st
        if t.uses_sd:
            k = self.g.rbs[0] if r1 > r2 else self.g.rbs[1]
            return _RBS_MOTIF[k], _RBS_SPACER[k]
        elif t.missing_motif_weight > -0.5 and r1 > r2 and r1 > ms:
            return _RBS_MOTIF[self.g.rbs[0]], _RBS_SPACER[self.g.rbs[0]]
        elif t.missing_motif_weight > -0.5 and r2 >= r1 and r2 > ms:
            return _RBS_MOTIF[self.g.rbs[1]], _RBS_SPACER[self.g.rbs[1]]
        elif self.g.mot_len == 0:
            return None, None
        else:
            motif = "".join("AGCT"[(self.g.mot_ndx >> (2 * i)) & 3] for i in range(self.g.mot_len))
            return motif, "%dbp" % self.g.mot_spacer

    @property
    def rbs_motif(self):
        return self._rbs()[0]

    @property
    def rbs_spacer(self):
        return self._rbs()[1]

    @property
    def gc_cont(self):
        return self.g.gc_cont

    @property
    def translation_table(self):
        return self.owner.training_info.translation_table

    @property
    def cscore(self):
        return self.g.cscore

    @property
    def rscore(self):
        return self.g.rscore

    @property
    def sscore(self):
        return self.g.sscore

    @property
    def tscore(self):
        return self.g.tscore

    @property
    def uscore(self):
        return self.g.uscore

    @property
    def score(self):
        return self.g.cscore + self.g.sscore

    @property
    def start_node(self):
        return self.owner.nodes[self.g.start_ndx] if self.owner.nodes is not None else None

    @property
    def stop_node(self):
        return self.owner.nodes[self.g.stop_ndx] if self.owner.nodes is not None else None

    cpdef double confidence(self):
        return _confidence(self.g.cscore + self.g.sscore, self.owner.training_info.start_weight)

    cdef bytes _span(self):
        """The letters begin .. end of the record; a gene across the origin of a circular sequence (end > length) reads on at
        the record's first base."""
        cdef bytes data = self.owner.sequence.data
        cdef ssize_t L = len(data)
        if self.g.end > L and self.owner.circular:
            return data[self.g.begin - 1:] + data[:self.g.end - L]
        return data[self.g.begin - 1:self.g.end]

    def sequence(self):
        """The nucleotide sequence of the gene, reverse-complemented on the reverse strand; unknown bases read N
        (ref: lib.pyx:2874-2930)."""
        cdef bytes s = self._span().upper()
        s = bytes(c if c in b"ACGT" else 78 for c in s)
        if self.g.strand != 1:
            s = s.translate(_COMPLEMENT)[::-1]
        return s.decode("ascii")

    def translate(self, object translation_table=None, object unknown_residue="X", bint include_stop=True, bint strict=True):
        """Translate the gene into a protein sequence (ref: lib.pyx:2932-3047, `Sequence._amino` 770-789).

        The first codon of a gene that does not start at an edge reads M when it is a start codon of the table;
        a stop codon of the table reads `*`; a codon with an unknown base reads `unknown_residue`, unless
        `strict=False` and every completion of the codon gives the same residue."""
        cdef int tt, owner_tt = self.owner.training_info.translation_table
        if translation_table is None:
            tt = owner_tt
        elif translation_table not in _CODE_BY_DIGITS:
            raise ValueError("%r is not a valid translation table index" % (translation_table,))
        else:
            tt = translation_table
            if _STOP_CODONS[tt] != _STOP_CODONS[owner_tt]:
                import warnings
                warnings.warn("requested translation table (%r) has different STOP codons than the one these genes "
                              "were called with (%r), consider calling genes with the proper translation table instead."
                              % (translation_table, owner_tt), stacklevel=2)
        cdef bytes unk = unknown_residue.encode("ascii") if isinstance(unknown_residue, str) else bytes(unknown_residue)
        if len(unk) != 1:
            raise ValueError("`unknown_residue` must be a single character")
        if (self.owner._prot is not None and self._index >= 0 and tt == self.owner._prot_tt and unk == b"X" and include_stop and strict):
            # translated on the device together with the gene calls (GeneFinder.find_genes_batch(..., translate=True))
            return self.owner._prot[self.owner._prot_off[self._index]:self.owner._prot_off[self._index + 1]].decode("ascii")
        cdef bytes nuc = self._span()
        if self.g.strand != 1:
            nuc = nuc.translate(_COMPLEMENT_ANY)[::-1]
        cdef bytes dig = nuc.translate(_DIGIT_OF)
        cdef const unsigned char* d = <const unsigned char*> PyBytes_AS_STRING(dig)
        cdef const char* table = PyBytes_AS_STRING(_CODE_BY_DIGITS[tt])
        cdef ssize_t n = len(dig) // 3, i, k
        # partial flags are in sequence orientation; the gene's own first / last codon follow its strand
        cdef bint start_edge = self.g.partial_begin if self.g.strand == 1 else self.g.partial_end
        cdef bint stop_edge = self.g.partial_end if self.g.strand == 1 else self.g.partial_begin
        if not stop_edge and not include_stop:
            n -= 1
        cdef bytearray out = bytearray(max(n, 0))
        cdef int x0, x1, x2, y
        cdef char aa, c2
        for i in range(n):
            x0 = d[3 * i]; x1 = d[3 * i + 1]; x2 = d[3 * i + 2]
            if x0 <= 3 and x1 <= 3 and x2 <= 3:
                if _codon_is_stop(x0, x1, x2, tt):
                    aa = 42                                                      # '*'
                elif i == 0 and not start_edge and _codon_is_start(x0, x1, x2, tt):
                    aa = 77                                                      # 'M'
                else:
                    aa = table[(x0 << 4) + (x1 << 2) + x2]
            else:
                aa = 88                                                          # 'X'
                if not strict and x0 <= 3 and (x1 <= 3) != (x2 <= 3):
                    # one unknown base in second or third position: unambiguous when all four completions agree
                    aa = table[(x0 << 4) + ((x1 if x1 <= 3 else 0) << 2) + (x2 if x2 <= 3 else 0)]
                    for y in range(1, 4):
                        c2 = table[(x0 << 4) + ((x1 if x1 <= 3 else y) << 2) + (x2 if x2 <= 3 else y)]
                        if c2 != aa:
                            aa = 88
                            break
            out[i] = unk[0] if aa == 88 else aa
        return out.decode("ascii")

    cpdef str _gene_data(self, object sequence_id, ssize_t index):
        motif, spacer = self._rbs()
        return "ID={}_{};partial={}{};start_type={};rbs_motif={};rbs_spacer={};gc_cont={:.3f}".format(
            sequence_id, index + 1, int(self.g.partial_begin), int(self.g.partial_end),
            _NODE_TYPE[self.g.start_type], motif, spacer, self.g.gc_cont)

    cpdef str _score_data(self):
        return "conf={:.2f};score={:.2f};cscore={:.2f};sscore={:.2f};rscore={:.2f};uscore={:.2f};tscore={:.2f};".format(
            self.confidence(), self.score, self.cscore, self.sscore, self.rscore, self.uscore, self.tscore)


cdef class Genes:
    """The genes of one sequence (ref: lib.pyx:3049-3186)."""
    cdef readonly Sequence sequence
    cdef readonly object training_info
    cdef readonly object metagenomic_bin
    cdef readonly bint meta
    cdef readonly double score
    cdef readonly ssize_t _num_seq
    cdef readonly bint circular   # the sequence was called as a circle (find_genes(..., circular=True)): a gene may end beyond its length
    cdef readonly object cut      # ... and where the finder cut it open for its second pass (0-based; node indices and `Node.index`
                                  # are those of sequence[cut:] + sequence[:cut]); None for a linear sequence
    cdef readonly object set_score     # find_genes_batch(..., sets=...): the summed score of the model chosen for this sequence's set
                                       # (None: the set has no model); None for a call without sets
    cdef readonly object model_scores  # ... and {model index: path score} of this sequence under every model of its set's GC window
                                       # it has a path under; None for a call without sets
    cdef readonly object terminal_repeat        # find_genes(..., trim_terminal_repeats=...): the bases taken off the end of the record
                                                # because they repeat its first bases (0: none, or a low-complexity one); `sequence` is
                                                # the record without them; None when the sequence was not searched
    cdef readonly object terminal_repeat_match  # ... and the length of the longest such repeat, low-complexity or not
    cdef list _genes           # the Gene objects, built from _recs when first asked for
    cdef bytes _recs           # the packed gene records of this sequence as the device call returned them
    cdef ssize_t _n
    cdef bytes _node_blob      # the node arrays of the winning model, field after field (None: keep_nodes=False)
    cdef ssize_t _node_n
    cdef object _nodes
    cdef object _prot          # proteins of all genes back to back, translated on the device with the default arguments, or None
    cdef object _prot_off      # int64[len + 1] offsets into _prot
    cdef int _prot_tt          # the translation table the device translated with

    cdef list _list(self):
        cdef ssize_t j
        cdef Gene gene
        cdef const pga_gene* g
        if self._genes is None:
            out = []
            if self._n > 0:
                g = <const pga_gene*> PyBytes_AS_STRING(self._recs)
                for j in range(self._n):
                    gene = Gene.__new__(Gene)
                    gene.owner = self
                    gene.g = g[j]
                    gene._index = j
                    out.append(gene)
            self._genes = out
        return self._genes

    @property
    def nodes(self):
        """The scored nodes of the sequence (`Nodes`), or None when the finder was created with keep_nodes=False."""
        if self._nodes is None and self._node_blob is not None:
            self._nodes = _nodes_from_blob(self._node_blob, self._node_n)
        return self._nodes

    def __len__(self):
        return self._n

    def __getitem__(self, index):
        return self._list()[index]

    def __iter__(self):
        return iter(self._list())

    def __bool__(self):
        return self._n > 0

    # --- writers (ref: lib.pyx:3405-3894): host-side formatting of the results, byte-compatible with the
    #     reference except for the tool name and version strings -------------------------------------------

    cdef tuple _model(self):
        """(TrainingInfo, description) the header lines report (ref: lib.pyx:3575-3583)."""
        if self.meta:
            if self.metagenomic_bin is None:
                raise RuntimeError("no metagenomic model was selected for this sequence")
            return self.training_info, self.metagenomic_bin.description
        return self.training_info, "Ab initio"

    def write_gff(self, object file, str sequence_id, bint header=True, bint include_translation_table=False,
                  bint full_id=True, str version_separator="_v"):
        """Write the genes to `file` in General Feature Format (ref: lib.pyx:3534-3644)."""
        cdef ssize_t n = 0, i
        cdef Gene gene
        tinf, desc = self._model()
        run = "Metagenomic" if self.meta else "Single"
        if header:
            n += file.write("##gff-version  3\n")
        n += file.write('# Sequence Data: seqnum=%d;seqlen=%d;seqhdr="%s"%s\n' % (self._num_seq, len(self.sequence), sequence_id,
                                                                                   ";topology=circular" if self.circular else ""))
        n += file.write('# Model Data: version=pyrodigal_amd.v%s;run_type=%s;model="%s";gc_cont=%.2f;transl_table=%d;uses_sd=%d\n'
                        % (_VERSION, run, desc, tinf.gc * 100, tinf.translation_table, int(tinf.uses_sd)))
        for i, gene in enumerate(self._list()):
            ident = gene._gene_data(sequence_id if full_id else self._num_seq, i)
            n += file.write("%s\tpyrodigal_amd%s%s\tCDS\t%d\t%d\t%.1f\t%s\t0\t%s;" % (
                sequence_id, version_separator, _VERSION, gene.g.begin, gene.g.end, gene.g.sscore + gene.g.cscore,
                "+" if gene.g.strand > 0 else "-", ident))
            if include_translation_table:
                n += file.write("transl_table=%d;" % tinf.translation_table)
            n += file.write(gene._score_data())
            n += file.write("\n")
        return n

    def write_genes(self, object file, str sequence_id, object width=70, bint full_id=False):
        """Write the nucleotide sequences of the genes to `file` in FASTA format (ref: lib.pyx:3646-3706)."""
        cdef ssize_t n = 0, i, k
        cdef Gene gene
        for i, gene in enumerate(self._list()):
            n += file.write(">%s_%d # %d # %d # %d # %s\n" % (sequence_id, i + 1, gene.g.begin, gene.g.end, gene.g.strand,
                                                              gene._gene_data(sequence_id if full_id else self._num_seq, i)))
            seq = gene.sequence()
            for k in range(0, len(seq), width):
                n += file.write(seq[k:k + width])
                n += file.write("\n")
        return n

    def write_translations(self, object file, str sequence_id, object width=60, object translation_table=None,
                           bint include_stop=True, bint strict_translation=True, bint full_id=False):
        """Write the protein translations of the genes to `file` in FASTA format (ref: lib.pyx:3708-3792)."""
        cdef ssize_t n = 0, i, k
        cdef Gene gene
        if translation_table is not None and translation_table not in _CODE_BY_DIGITS:
            raise ValueError("%r is not a valid translation table index" % (translation_table,))
        for i, gene in enumerate(self._list()):
            n += file.write(">%s_%d # %d # %d # %d # %s\n" % (sequence_id, i + 1, gene.g.begin, gene.g.end, gene.g.strand,
                                                              gene._gene_data(sequence_id if full_id else self._num_seq, i)))
            prot = gene.translate(translation_table, include_stop=include_stop, strict=strict_translation)
            for k in range(0, len(prot), width):
                n += file.write(prot[k:k + width])
                n += file.write("\n")
        return n

    def write_genbank(self, object file, str sequence_id, str division="BCT", object date=None, object translation_table=None,
                      bint strict_translation=True):
        """Write the genes and the sequence to `file` as a complete GenBank record (ref: lib.pyx:3405-3532)."""
        import datetime
        import textwrap
        cdef ssize_t n = 0, i, j
        cdef Gene gene
        if translation_table is None:
            if self.training_info is not None:
                translation_table = self.training_info.translation_table
        elif translation_table not in _CODE_BY_DIGITS:
            raise ValueError("%r is not a valid translation table index" % (translation_table,))
        if date is None:
            date = datetime.date.today()
        elif not isinstance(date, datetime.date):
            raise TypeError("Expected datetime.date, found %s" % type(date).__name__)
        slen = len(self.sequence)
        n += file.write("LOCUS       {:<23} {} bp    DNA     {} {} {}\n".format(sequence_id, slen, "circular" if self.circular else "linear  ", division,
                                                                            date.strftime("%d-%b-%y").upper()))
        n += file.write("REFERENCE   1  (bases 1 to %d)\n" % slen)
        n += file.write("  AUTHORS   Hyatt,D., Chen,G-L., LoCascio,P.F., Land,M.L., Larimer,F.W.\n")
        n += file.write("            Hauser,L.J.\n")
        n += file.write("  TITLE     Prodigal: prokaryotic gene recognition and translation initiation\n")
        n += file.write("            site identification\n")
        n += file.write("  JOURNAL   BMC Bioinformatics. 2010;11:119.\n")
        n += file.write("   PUBMED   20211023\n")
        n += file.write("FEATURES             Location/Qualifiers\n")
        for i, gene in enumerate(self._list()):
            start_edge = gene.g.partial_begin if gene.g.strand == 1 else gene.g.partial_end
            stop_edge = gene.g.partial_end if gene.g.strand == 1 else gene.g.partial_begin
            begin = "<%d" % gene.g.begin if start_edge else "%d" % gene.g.begin
            end = ">%d" % gene.g.end if stop_edge else "%d" % gene.g.end
            loc = "%s..%s" % (begin, end)
            if self.circular and gene.g.end > slen:          # across the origin: two spans in the record's coordinates
                loc = "join(%d..%d,1..%d)" % (gene.g.begin, slen, gene.g.end - slen)
            n += file.write("     CDS             %s\n" % (loc if gene.g.strand == 1 else "complement(%s)" % loc))
            pad = " " * 21
            n += file.write('%s/codon_start=1\n' % pad)
            n += file.write('%s/inference="ab initio prediction:pyrodigal_amd:%s"\n' % (pad, _VERSION))
            n += file.write('%s/locus_tag="%s_%d"\n' % (pad, sequence_id, i + 1))
            n += file.write('%s/transl_table=%s\n' % (pad, translation_table))
            tr = '/translation="%s"' % gene.translate(translation_table=translation_table, include_stop=False, strict=strict_translation)
            for block in textwrap.wrap(tr, 59):
                n += file.write(pad + block + "\n")
        seq = str(self.sequence).lower()
        n += file.write("ORIGIN\n")
        for i in range(0, len(seq), 60):
            n += file.write("{:>9}".format(i + 1))
            for j in range(i, min(i + 60, len(seq)), 10):
                n += file.write(" " + seq[j:j + 10])
            n += file.write("\n")
        n += file.write("//\n")
        return n

    def write_scores(self, object file, str sequence_id, bint header=True):
        """Write the scores of every start node, grouped by stop codon, to `file` (ref: lib.pyx:3794-3894)."""
        cdef ssize_t n = 0
        if self.circular:
            raise ValueError("write_scores is not available for a circular sequence: its nodes live in the coordinates of the "
                             "rotated sequence (Genes.cut)")
        if self.nodes is None:
            raise RuntimeError("write_scores needs the nodes: create the GeneFinder with keep_nodes=True")
        tinf, _ = self._model()
        f = self.nodes._f
        rbs_wt = tinf._f64(80, 28)
        cdef double st_wt = tinf.start_weight, no_mot = tinf.missing_motif_weight, rbs1, rbs2
        cdef bint uses_sd = tinf.uses_sd
        # Prodigal's stopcmp_nodes: stop_val ascending, then strand descending, then ndx ascending
        order = np.lexsort((f["ndx"], -f["strand"].astype(np.int32), f["stop_val"]))
        if header:
            n += file.write('# Sequence Data: seqnum=%d;seqlen=%d;seqhdr="%s"\n' % (self._num_seq, len(self.sequence), sequence_id))
            n += file.write("# Run Data: version=pyrodigal_amd.v%s;gc_cont=%.2f;transl_table=%d;uses_sd=%d\n"
                            % (_VERSION, tinf.gc * 100, tinf.translation_table, int(uses_sd)))
            n += file.write("Beg\tEnd\tStd\tTotal\tCodPot\tStrtSc\tCodon\tRBSMot\tSpacer\tRBSScr\tUpsScr\tTypeScr\tGCCont\n")
        prev_stop, prev_strand = -1, 0
        for i in order:
            if f["type"][i] == 3:
                continue
            ndx = int(f["ndx"][i]); stop_val = int(f["stop_val"][i]); strand = int(f["strand"][i])
            if stop_val != prev_stop or strand != prev_strand:
                prev_stop, prev_strand = stop_val, strand
                n += file.write("\n")
            if strand == 1:
                n += file.write("%d\t%d\t+\t" % (ndx + 1, stop_val + 3))
            else:
                n += file.write("%d\t%d\t-\t" % (stop_val - 1, ndx + 1))
            cs = float(f["cscore"][i]); ss = float(f["sscore"][i]); rs = float(f["rscore"][i])
            n += file.write("%.2f\t%.2f\t%.2f\t%s\t" % (cs + ss, cs, ss, ["ATG", "GTG", "TTG", "Edge"][3 if f["edge"][i] else int(f["type"][i])]))
            r0 = int(f["rbs"][i][0]); r1 = int(f["rbs"][i][1])
            rbs1 = rbs_wt[r0] * st_wt; rbs2 = rbs_wt[r1] * st_wt
            mot = float(f["mot_score"][i]) * st_wt
            if uses_sd:
                k = r0 if rbs1 > rbs2 else r1
                n += file.write("%s\t%s\t%.2f\t" % (_RBS_MOTIF[k], _RBS_SPACER[k], rs))
            elif no_mot > -0.5 and rbs1 > rbs2 and rbs1 > mot:
                n += file.write("%s\t%s\t%.2f\t" % (_RBS_MOTIF[r0], _RBS_SPACER[r0], rs))
            elif no_mot > -0.5 and rbs2 >= rbs1 and rbs2 > mot:
                n += file.write("%s\t%s\t%.2f\t" % (_RBS_MOTIF[r1], _RBS_SPACER[r1], rs))
            elif f["mot_len"][i] == 0:
                n += file.write("None\tNone\t%.2f\t" % rs)
            else:
                motif = "".join("AGCT"[(int(f["mot_ndx"][i]) >> (2 * q)) & 3] for q in range(int(f["mot_len"][i])))
                n += file.write("%s\t%dbp\t%.2f\t" % (motif, int(f["mot_spacer"][i]), rs))
            n += file.write("%.2f\t%.2f\t%.3f\n" % (float(f["uscore"][i]), float(f["tscore"][i]), float(f["gc_cont"][i])))
        n += file.write("\n")
        return n


# --- GeneFinder (ref: lib.pyx:5073-5575) ------------------------------------------------------
cdef class _FinderSlot:
    """One device context of a finder: its own HIP stream, scratch buffers and copy of the models."""
    cdef pga_ctx* ctx
    cdef bint busy
    cdef bint models_loaded
    cdef object models_sig      # (id(raw), version) of every model as loaded: a TrainingInfo changed in place is reloaded

    def __cinit__(self):
        self.ctx = NULL
        self.busy = False
        self.models_loaded = False
        self.models_sig = None

    def __dealloc__(self):
        if self.ctx != NULL:
            pga_destroy(self.ctx)
            self.ctx = NULL


cdef class TerminalRepeats:
    """How `find_genes(..., trim_terminal_repeats=...)` looks for a direct terminal repeat: the longest `r` in
    `min_length .. min(max_length, len(sequence) // 2)` for which the first `r` bases of the sequence are also its last `r`; a repeat
    in which one base makes up more than `max_base_percent` percent is low-complexity and is left alone (100: no such filter)."""
    cdef readonly int min_length
    cdef readonly int max_length
    cdef readonly int max_base_percent

    def __init__(self, int min_length=20, int max_length=65536, int max_base_percent=75):
        if not (1 <= min_length <= max_length <= 1048576):
            raise ValueError("1 <= min_length <= max_length <= 1048576 does not hold for %d, %d" % (min_length, max_length))
        if not (25 <= max_base_percent <= 100):
            raise ValueError("`max_base_percent` must lie in 25 .. 100, not %d" % max_base_percent)
        self.min_length = min_length
        self.max_length = max_length
        self.max_base_percent = max_base_percent

    def _key(self):
        return (self.min_length, self.max_length, self.max_base_percent)

    def __eq__(self, other):
        return isinstance(other, TerminalRepeats) and self._key() == (<TerminalRepeats> other)._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return "pyrodigal_amd.lib.TerminalRepeats(min_length=%d, max_length=%d, max_base_percent=%d)" % self._key()

    def __reduce__(self):
        return TerminalRepeats, self._key()


cdef tuple _terminal_repeat_option(object option, Py_ssize_t n):
    """`trim_terminal_repeats=` of a call over n sequences -> (one bool per sequence, (min_length, max_length, max_base_percent)),
    or (None, None) when no sequence is to be searched."""
    cdef TerminalRepeats shared = None
    cdef list search
    if option is None or option is False:
        return None, None
    if option is True:
        return [True] * n, TerminalRepeats()._key()
    if isinstance(option, TerminalRepeats):
        return [True] * n, (<TerminalRepeats> option)._key()
    entries = list(option)
    if len(entries) != n:
        raise ValueError("`trim_terminal_repeats` has %d entries for %d sequences" % (len(entries), n))
    search = []
    for i, e in enumerate(entries):
        if e is None or e is False:
            search.append(False)
            continue
        search.append(True)
        if e is True:
            continue
        if not isinstance(e, TerminalRepeats):
            raise TypeError("trim_terminal_repeats[%d] is neither a bool nor a TerminalRepeats (%r)" % (i, type(e).__name__))
        if shared is not None and e is not shared and e != shared:
            raise ValueError("`trim_terminal_repeats` names two different TerminalRepeats in one call (sequence %d): a call has one "
                             "set of parameters" % i)
        if shared is None:
            shared = <TerminalRepeats> e
    if not any(search):
        return None, None
    return search, (TerminalRepeats() if shared is None else shared)._key()


cdef pga_batch* _trimmed_batch(pga_ctx* ctx, pga_batch* whole, size_t p_search, tuple params, size_t p_match, size_t p_trim) except? NULL:
    """The terminal-repeat step of a device call: the search on the resident batch (`p_search`: a flag per sequence; match and trim go
    to `p_match` / `p_trim`) and the batch without the repeats, or NULL when no sequence has one to take off."""
    cdef pga_batch* out = NULL
    cdef int32_t min_length = params[0], max_length = params[1], max_base_percent = params[2]
    cdef int rc
    with nogil:
        rc = pga_batch_terminal_repeats(ctx, whole, <const uint8_t*> p_search, min_length, max_length, max_base_percent,
                                        <int32_t*> p_match, <int32_t*> p_trim)
        if rc == PGA_OK:
            rc = pga_batch_trim_terminal_repeats(ctx, whole, <const int32_t*> p_trim, &out)
    if rc != PGA_OK:
        _raise_for(ctx, rc, "pga_batch_terminal_repeats")
    return out


cdef int _refuse_device_input(object x, str what) except -1:
    if isinstance(x, _DeviceSequences):
        raise TypeError("`%s` does not take sequences in device memory (a DeviceSequences): `find_genes_batch` does" % what)
    return 0


cdef pga_batch* _device_batch(pga_ctx* ctx, object dev) except? NULL:
    """The resident batch of a `DeviceSequences`, packed on the device (`pga_batch_create_device`)."""
    cdef pga_batch* batch = NULL
    cdef int32_t n = len(dev), eb = dev.elem_bytes, n_alpha = 0
    cdef int64_t n_elems = dev.n_elems
    cdef size_t p_data = dev.ptr, p_off = dev.offsets.ctypes.data, p_len = dev.lengths.ctypes.data, p_stream = dev.stream
    cdef bytes table = dev.alphabet
    cdef const uint8_t* p_alpha = NULL
    cdef int rc
    if table is not None:
        p_alpha = <const uint8_t*> PyBytes_AS_STRING(table); n_alpha = len(table)
    with nogil:
        rc = pga_batch_create_device(ctx, n, <const void*> p_data, n_elems, eb, <const int64_t*> p_off, <const int64_t*> p_len, p_alpha, n_alpha,
                                     <void*> p_stream, &batch)
    if rc != PGA_OK:
        _raise_for(ctx, rc, "pga_batch_create_device")
    return batch


cdef int _one_call_for_tokens(object tokens, list calls) except -1:
    if tokens is not None and len(calls) > 1:
        raise ValueError("`training_infos` would split this request into %d device calls (more than `coalesce_bases` bases or four "
                         "translation tables in a row): %s writes one tensor per request" % (len(calls), tokens["method"]))
    return 0


cdef class _FindRequest:
    """The sequences of one `find_genes` / `find_genes_batch` call, waiting for a device call to ride."""
    cdef list seqs              # Sequence objects
    cdef list tr_search         # one bool per sequence: searched for a direct terminal repeat; None: none of them
    cdef object tr_params       # (min_length, max_length, max_base_percent) of that search: requests that ride one device call agree on it
    cdef list circ              # one bool per sequence: called as a circle; None: all linear
    cdef object sets            # int32 per sequence: dense set id, -1: on its own; None: no sets (such a request rides alone)
    cdef bint translate
    cdef object tokens          # find_proteins_batch / find_labels_batch: {"spec", "out", "stream", "method"} -- the rule's tensor is also
                                # written on the device, and the device call leaves the DeviceProteins / DeviceLabels under "result"
                                # (such a request rides alone); None: no tensor
    cdef ssize_t first_id
    cdef int64_t bases
    cdef list out               # one Genes per sequence, filled in by the thread that ran the device call
    cdef object error
    cdef bint done
    cdef object sem             # a lock used as a binary semaphore (C-level, no Python-side condition variable): released when the result
                                # is there, or when `lead` holds a context for this caller to run the next device call
    cdef bint signaled          # the semaphore was released and the owner has not looked yet (never released twice)
    cdef object lead


cdef object _new_lock = threading.Lock


cdef inline void _signal(_FindRequest r):
    """(finder lock held) Wake the owner of a request: at most one release per look of the owner."""
    if not r.signaled:
        r.signaled = True
        r.sem.release()


cdef class _CallState:
    """One device call: the options of the requests that ride it, per sequence of the call (`_call_options`), and what the call
    reports back per sequence (`_resident_call`), for `_genes_of_call` to read."""
    cdef list ids               # the number of every sequence
    cdef object flags, cuts     # uint8 / int32 per sequence: called as a circle, and where it was cut open; None: no request names a
                                # circle or searches for terminal repeats
    cdef object tr_params       # the terminal-repeat search of this call, or None: no request asks for one
    cdef object tr_flags, tr_match, tr_trim     # uint8 / int32 / int32 per sequence: searched, the longest repeat, the bases taken off
    cdef object set_ids         # the sets of a request that rides alone, or None
    cdef object tok             # the tokens of a request that rides alone, or None
    # reported by the call
    cdef int n_models           # with sets: the models, and per sequence the model and score of its set and [n_models] path scores
    cdef object set_model, set_score, model_scores
    cdef object prot, prot_off, tables          # with translate: the proteins of `_translate`


cdef _CallState _call_options(list take, int n):
    """The state of one device call over n sequences, with the options of the requests in `take`, which ride it."""
    cdef _CallState o = _CallState.__new__(_CallState)
    cdef _FindRequest r
    cdef Py_ssize_t i = 0, j
    cdef bint circles = False
    o.ids = []
    for r in take:
        for j in range(len(r.seqs)):
            o.ids.append(r.first_id + j)
        if r.circ is not None:
            circles = True
        if r.tr_params is not None:
            o.tr_params = r.tr_params
    if len(take) == 1:
        o.set_ids = (<_FindRequest> take[0]).sets
        o.tok = (<_FindRequest> take[0]).tokens
    if o.tr_params is not None:
        o.tr_flags = np.zeros(max(n, 1), np.uint8); o.tr_match = np.zeros(max(n, 1), np.int32); o.tr_trim = np.zeros(max(n, 1), np.int32)
    if circles or o.tr_params is not None:         # (a trimmed sequence is a circle: the flags are completed after the search)
        o.flags = np.zeros(max(n, 1), np.uint8)
        o.cuts = np.full(max(n, 1), -1, np.int32)
        for r in take:
            if r.circ is not None:
                o.flags[i:i + len(r.seqs)] = r.circ
            if r.tr_search is not None and o.tr_params is not None:
                o.tr_flags[i:i + len(r.seqs)] = r.tr_search
            i += len(r.seqs)
    return o


cdef class GeneFinder:
    """A configurable gene finder for genomes and metagenomes, running on one MI355X.

    Re-entrant like the reference's (lib.pyx:5424-5446, README "thread-safety"): `find_genes` may be called from any number
    of threads (the reference's own CLI maps it over a thread pool, cli.py:289-302).  Concurrent calls do not queue behind a
    lock: the finder owns up to `contexts` device contexts (one HIP stream each; two by default: with one contig per call more
    contexts only cut the same callers into smaller device calls), and the calls that are waiting when a context
    is free are packed into ONE device call (`pga_find_genes_batch` over all their sequences, at most `coalesce_bases` bases)
    by whichever caller finds the context -- so a pool of threads rides the batch path, and a lone caller pays no wait."""
    cdef readonly bint meta
    cdef readonly bint closed
    cdef readonly bint mask
    cdef readonly int min_mask
    cdef readonly bint mask_lowercase
    cdef readonly int min_gene
    cdef readonly int min_edge_gene
    cdef readonly int max_overlap
    cdef readonly str backend
    cdef readonly object training_info
    cdef readonly MetagenomicBins metagenomic_bins
    cdef readonly int device
    cdef readonly bint keep_nodes
    cdef readonly int contexts
    cdef readonly int64_t coalesce_bases
    cdef readonly dict stats    # device calls, sequences and the largest number of calls packed into one (diagnostics)
    cdef object lock            # kept for callers that serialise around a finder themselves (ref: lib.pyx:5196)
    cdef object _cv
    cdef object _lock
    cdef list _slots
    cdef list _pending
    cdef ssize_t _num_seq

    def __cinit__(self):
        self._num_seq = 1

    def __init__(self, TrainingInfo training_info=None, *, bint meta=False, MetagenomicBins metagenomic_bins=None,
                 bint closed=False, bint mask=False, int min_mask=50, int min_gene=90, int min_edge_gene=60,
                 int max_overlap=60, str backend="detect", int device=0, bint keep_nodes=True, int contexts=2,
                 int64_t coalesce_bases=64 << 20, bint mask_lowercase=False):
        # argument validation as in the reference (lib.pyx:5169-5181)
        if meta and training_info is not None:
            raise ValueError("cannot use a training info in meta mode.")
        if min_gene <= 0:
            raise ValueError("`min_gene` must be strictly positive")
        if min_edge_gene <= 0:
            raise ValueError("`min_edge_gene` must be strictly positive")
        if min_edge_gene < 4 and not closed:
            raise ValueError("`min_edge_gene` below 4 is not supported with open ends (one-codon edge genes)")
        if min_mask < 0:
            raise ValueError("`min_mask` must be positive")
        if max_overlap < 0:
            raise ValueError("`max_overlap` must be positive")
        elif max_overlap > min_gene:
            raise ValueError("`max_overlap` must be lower than `min_gene`")
        if backend not in ("detect", "hip"):
            raise ValueError("unsupported backend %r: this build only has the HIP (gfx950) backend" % backend)
        if contexts < 1 or contexts > 16:
            raise ValueError("`contexts` must be between 1 and 16")
        self.meta = meta
        self.closed = closed
        self.mask = mask
        self.min_mask = min_mask
        self.mask_lowercase = mask_lowercase
        self.min_gene = min_gene
        self.min_edge_gene = min_edge_gene
        self.max_overlap = max_overlap
        self.backend = backend
        self.training_info = training_info
        self.metagenomic_bins = METAGENOMIC_BINS if metagenomic_bins is None else metagenomic_bins
        self.device = device
        self.keep_nodes = keep_nodes
        self.contexts = contexts
        self.coalesce_bases = max(coalesce_bases, 1)
        self.lock = threading.Lock()
        self._lock = threading.Lock()
        self._cv = threading.Condition(self._lock)
        self._slots = [_FinderSlot() for _ in range(contexts)]
        self._pending = []
        self.stats = {"device_calls": 0, "sequences": 0, "max_calls_per_device_call": 0}

    def __reduce__(self):           # ref: lib.pyx:5219-5234
        cdef dict kw = dict(
            meta=self.meta, metagenomic_bins=self.metagenomic_bins if self.meta else None, closed=self.closed, mask=self.mask,
            min_mask=self.min_mask, min_gene=self.min_gene, min_edge_gene=self.min_edge_gene, max_overlap=self.max_overlap,
            backend=self.backend, device=self.device, keep_nodes=self.keep_nodes, contexts=self.contexts,
            coalesce_bases=self.coalesce_bases)
        if self.mask_lowercase:
            kw["mask_lowercase"] = True
        return _gene_finder_from_state, (self.training_info, kw)

    def __repr__(self):
        parts = []
        if self.training_info is not None:
            parts.append("training_info=%r" % self.training_info)
        if self.meta:
            parts.append("meta=True")
        if self.closed:
            parts.append("closed=True")
        if self.mask_lowercase:
            parts.append("mask_lowercase=True")
        return "pyrodigal_amd.lib.GeneFinder(%s)" % ", ".join(parts)

    cdef int _ensure_models(self, _FinderSlot slot) except -1:
        cdef int rc, n, i
        cdef const pga_training** ptrs
        cdef list blobs
        if slot.ctx == NULL:
            rc = pga_create(self.device, &slot.ctx)
            if rc != PGA_OK:
                slot.ctx = NULL
                _raise_for(NULL, rc, "pga_create")
        cdef list tinfs
        if self.meta:
            tinfs = [(<MetagenomicBin> b).training_info for b in self.metagenomic_bins]
        else:
            tinfs = [self.training_info]
        # the reference shares the struct by pointer, so a setter takes effect at the next call: reload when one moved
        cdef tuple sig = tuple([(id((<TrainingInfo> t)._raw), (<TrainingInfo> t)._version) for t in tinfs])
        if slot.models_loaded and sig == slot.models_sig:
            return 0
        blobs = [(<TrainingInfo> t)._raw for t in tinfs]
        n = len(blobs)
        ptrs = <const pga_training**> malloc(sizeof(void*) * max(n, 1))
        if ptrs == NULL:
            raise MemoryError()
        try:
            for i in range(n):
                ptrs[i] = <const pga_training*> <size_t> blobs[i].ctypes.data
            rc = pga_set_models(slot.ctx, ptrs, n)
        finally:
            free(ptrs)
        if rc != PGA_OK:
            _raise_for(slot.ctx, rc, "pga_set_models")
        slot.models_loaded = True
        slot.models_sig = sig
        return 0

    def find_genes(self, object sequence, object regions=None, bint circular=False, object trim_terminal_repeats=False):
        """Find all the genes in the input DNA sequence (ref: lib.pyx:5400-5469).

        `circular=True`: the record is a circle cut open at an arbitrary base (a closed chromosome, a plasmid, a phage genome).
        The linear call only serves to find the widest stretch without a gene in the record's middle half; the sequence is then
        called again, closed, rotated to start in the middle of that stretch (`genes.cut`), and its genes are reported in the
        record's coordinates: `1 <= begin <= len(sequence)`, and `end > len(sequence)` exactly for a gene across the origin, which
        ends at base `end - len(sequence)`.  No gene of a circular sequence is partial.  `genes.nodes`, `Gene.start_node` and
        `Gene.stop_node` are those of the rotated sequence.

        `trim_terminal_repeats`: `True` or a `TerminalRepeats`.  An assembler that closes a circle (or a phage genome with a direct
        terminal repeat) writes the first bases of the record once more at its end.  The finder looks for that repeat on the device,
        takes the second copy off and calls what is left as a circle, exactly as `find_genes(sequence[:-n], circular=True)` would:
        `genes.terminal_repeat` is `n` (0: no repeat, the sequence keeps the topology `circular` gives it), `genes.sequence` is the
        record without it.  A repeat that is mostly one base (`genes.terminal_repeat_match > 0` with `terminal_repeat == 0`) is
        not a topology and is left alone.

        `regions`: `[begin, end)` intervals of the sequence (0-based; a `Masks`, or any iterable of `Mask` objects or pairs) that no
        gene may run across, exactly as if they were masked runs of `N` -- while the bases keep their identity for the GC content,
        the model choice, every score and the printed sequence.  They join the runs of unknown bases (`mask=True`), the runs of
        lower-case letters (`mask_lowercase=True`) and the regions a `Sequence` already carries; `genes.sequence.masks` is the union."""
        _refuse_device_input(sequence, "find_genes")
        return self.find_genes_batch([sequence], regions=None if regions is None else [regions], circular=circular,
                                     trim_terminal_repeats=trim_terminal_repeats)[0]

    cdef _FinderSlot _free_slot(self):
        # a context that already exists first: a lone caller never makes a second one
        cdef _FinderSlot s, spare = None
        for s in self._slots:
            if not s.busy:
                if s.ctx != NULL:
                    return s
                if spare is None:
                    spare = s
        return spare

    cdef list _take_pending(self):
        """The waiting requests that ride the next device call: in arrival order, same options, up to the base budget."""
        cdef _FindRequest r, head = self._pending[0]
        cdef int64_t bases = 0
        cdef list take = []
        cdef ssize_t k = 0
        cdef object tr_params = None          # the terminal-repeat search of the call: its requests that search at all agree on it
        while k < len(self._pending):
            r = self._pending[k]
            if r.translate != head.translate or (take and bases + r.bases > self.coalesce_bases):
                break
            if r.tr_params is not None:
                if tr_params is not None and tr_params != r.tr_params:
                    break
                tr_params = r.tr_params
            take.append(r)
            bases += r.bases
            k += 1
        del self._pending[:k]
        return take

    def find_genes_batch(self, object sequences, *, bint translate=False, object training_infos=None, object regions=None,
                         object circular=None, object sets=None, object trim_terminal_repeats=None):
        """`find_genes` for many sequences in one device pass; returns one `Genes` per input, in order.

        `translate=True` also translates every gene on the device while the batch is resident (one thread per codon, the
        translation table of the model that called the gene): `Gene.translate()` with its default arguments and
        `Genes.write_translations` then read those proteins instead of translating codon by codon on the host.

        `training_infos` (single mode only): one `TrainingInfo` per sequence, sequence i is called with `training_infos[i]`
        -- the result is that of `GeneFinder(training_infos[i], <same options>).find_genes(sequences[i])`, for many genomes
        under their own models in a few device calls.  The finder's own `training_info` is not used (nor needed) then.

        `regions`: one entry per sequence, `None` or the regions of that sequence as `find_genes` takes them.

        `circular`: `None` / `False` (every sequence is linear), `True` (every sequence is a circle) or one flag per sequence;
        see `find_genes`.  Circular and linear sequences share a device call.

        `sets` (meta mode only): one label per sequence -- any hashable, `None` for a sequence on its own -- that names the set of
        sequences it belongs to: the contigs of a bin or a draft genome, the segments of a virus.  One metagenomic model is then
        chosen per set, from the GC content of the set as a whole and the summed scores of its members, instead of one per
        sequence; `Genes.set_score` and `Genes.model_scores` say how the choice came out.  A member without a gene path under
        the set's model has no genes.  The call is a device call of its own and cannot be combined with `circular`.

        `trim_terminal_repeats`: `None` / `False`, `True` (every sequence, the default parameters), a `TerminalRepeats` (every
        sequence) or one entry per sequence, each `False`, `True` or one shared `TerminalRepeats`; see `find_genes`.  Independent
        of `circular`: a sequence is called as a circle when either says so.

        `sequences` may be a `DeviceSequences`: sequences that already lie in device memory (a torch tensor of letters or token ids, a
        raw device pointer), with every option above.  The batch is packed on the device (`pga_batch_create_device`), the request is
        a device call of its own, and the packed letters come home once per device call (`pga_batch_read`: 1 byte per base, no Python
        decode, no upload) so that `Genes.sequence`, `Gene.sequence()` and the host writers behave exactly as after host input.  The
        zero-copy path, where only the gene records come home, is the raw layer: `_cabi.Context.upload_device` and
        `Context.find_genes`."""
        cdef list circ, tr_search
        cdef object dev, set_ids, tr_params
        dev, sequences, circ, set_ids, tr_search, tr_params = self._batch_options(sequences, training_infos, circular, sets, trim_terminal_repeats)
        if dev is not None:
            return self._find_genes_device(dev, translate, training_infos, regions, circ, set_ids, tr_search, tr_params)
        if training_infos is not None:
            return self._find_genes_models(sequences, translate, training_infos, regions, circ, tr_search, tr_params)
        if not self.meta and self.training_info is None:
            raise RuntimeError("cannot find genes without having trained in single mode")
        # the reference always re-wraps with the finder's masking rule (ref: lib.pyx:5433-5438); a Sequence that already
        # follows it is used as it is
        cdef list seqs = self._wrap_sequences(sequences, regions)
        cdef int64_t bases = 0
        for s in seqs:
            bases += len((<Sequence> s).data)
        if not seqs:
            return []
        cdef _FindRequest req = _FindRequest.__new__(_FindRequest)
        cdef _FindRequest r
        cdef _FinderSlot slot = None
        cdef list take
        if set_ids is not None:
            return self._find_genes_sets(seqs, translate, set_ids)
        req.seqs = seqs; req.translate = translate; req.bases = bases; req.out = None; req.error = None; req.done = False
        req.circ = circ
        req.tr_search = tr_search; req.tr_params = tr_params
        req.lead = None
        req.signaled = False
        req.sem = _new_lock()
        req.sem.acquire()
        lock = self._lock
        # Either a context is free: this caller runs a device call right away, for itself and for everyone who is waiting.  Or it
        # waits on a semaphore of its own -- woken when its result is there, or when a context came free and it is this caller's
        # turn to run the next device call over whatever is waiting by then (the baton goes to the oldest waiting request: one
        # wake-up per device call, not one per waiting thread).
        with lock:
            req.first_id = self._num_seq
            self._num_seq += len(seqs)
            self._pending.append(req)
            slot = self._free_slot()
            if slot is not None:
                slot.busy = True
        try:
            while True:
                if slot is None:
                    req.sem.acquire()                        # blocks without the GIL until somebody signals this request
                    with lock:
                        req.signaled = False
                        slot = <_FinderSlot> req.lead        # the baton: a context reserved for this caller (or None: the result is there)
                        req.lead = None
                    if slot is None:
                        if req.done:
                            break
                        continue
                with lock:
                    take = self._take_pending() if self._pending else []
                try:
                    if take:
                        self._run(slot, take)
                finally:
                    # whatever happened to this caller, the requests it took get their wake-up and the context moves on
                    with lock:
                        for r in take:
                            if not r.done and r.out is None and r.error is None:
                                r.error = RuntimeError("the device call this request rode was interrupted in another thread")
                            r.done = True
                            if r is not req:
                                _signal(r)
                        self._release_slot(slot)
                    slot = None
                if req.done:
                    break
        except BaseException:
            # a caller interrupted while it waits (KeyboardInterrupt in `acquire`) leaves nothing behind: its request leaves the queue,
            # a context that was handed to it in the meantime goes to the next waiting request
            with lock:
                if req in self._pending:
                    self._pending.remove(req)
                if slot is None and req.lead is not None:
                    slot = <_FinderSlot> req.lead
                    req.lead = None
                if slot is not None:
                    self._release_slot(slot)
            raise
        if req.error is not None:
            raise req.error
        return req.out

    def find_proteins_batch(self, object sequences, object tokens, *, object out=None, object stream=None, bint translate=False,
                            object training_infos=None, object regions=None, object circular=None, object sets=None,
                            object trim_terminal_repeats=None):
        """`find_genes_batch`, and the proteins of every gene left in device memory as token ids: returns `(genes, proteins)`, the
        list of `Genes` that `find_genes_batch` returns for the same arguments and a `DeviceProteins`.

        `tokens`: a `ProteinTokens` -- vocabulary, special tokens, element type, padded or ragged layout.  The tensor is written on
        the device while the batch is resident, under the translation table of the model that called each gene; row (or slice) g is
        gene g of the request, contig after contig (`proteins.gene_begin`).  `out`: the device tensor to write (anything with
        `__cuda_array_interface__`), `None`: a torch tensor allocated under torch's current stream; `stream`: the stream that last
        used `out`.  Every option of `find_genes_batch` applies and `sequences` may be a `DeviceSequences`.  The request is a device
        call of its own: one tensor per request, so a request that `training_infos` would split into several device calls is a
        `ValueError`."""
        if not isinstance(tokens, _cabi.ProteinTokens):
            raise TypeError("`tokens` must be a ProteinTokens, not %r" % type(tokens).__name__)
        return self._find_tensor_batch("find_proteins_batch", sequences, tokens, out, stream, translate, training_infos, regions, circular, sets,
                                       trim_terminal_repeats)

    def find_labels_batch(self, object sequences, object labels, *, object out=None, object stream=None, bint translate=False,
                          object training_infos=None, object regions=None, object circular=None, object sets=None,
                          object trim_terminal_repeats=None):
        """`find_genes_batch`, and the annotation of every base left in device memory as a tensor in the shape of the input: returns
        `(genes, device_labels)`, the list of `Genes` that `find_genes_batch` returns for the same arguments and a `DeviceLabels`.

        `labels`: a `BaseLabels` -- the class of every raw byte (codon position per strand, start and stop codons), element type,
        padded or ragged layout.  The tensor is written on the device while the batch is resident, on the batch the finder called:
        row (or slice) i is sequence i of the request, and with `trim_terminal_repeats` a trimmed record's row ends at its trimmed
        length (`device_labels.lengths[i]`), the rest of the row being `pad`.  `out`: the device tensor to write (anything with
        `__cuda_array_interface__`), `None`: a torch tensor allocated under torch's current stream; `stream`: the stream that last
        used `out`.  Every option of `find_genes_batch` applies and `sequences` may be a `DeviceSequences`.  The request is a device
        call of its own: one tensor per request, so a request that `training_infos` would split into several device calls is a
        `ValueError`."""
        if not isinstance(labels, _cabi.BaseLabels):
            raise TypeError("`labels` must be a BaseLabels, not %r" % type(labels).__name__)
        return self._find_tensor_batch("find_labels_batch", sequences, labels, out, stream, translate, training_infos, regions, circular, sets,
                                       trim_terminal_repeats)

    def find_windows_batch(self, object sequences, object windows, *, object out=None, object stream=None, bint translate=False,
                           object training_infos=None, object regions=None, object circular=None, object sets=None,
                           object trim_terminal_repeats=None):
        """`find_genes_batch`, and the nucleotides of every gene or of a region around it left in device memory as token ids, one
        row per gene in the gene's own reading direction: returns `(genes, device_windows)`, the list of `Genes` that
        `find_genes_batch` returns for the same arguments and a `DeviceWindows`.

        `windows`: a `GeneWindows` -- where a window begins and ends against the gene's start and end, bases or codons, vocabulary,
        special tokens, element type, padded or ragged layout.  The tensor is written on the device while the batch is resident, on
        the batch the finder called: row (or slice) g is gene g of the request, contig after contig (`device_windows.gene_begin`);
        a window wraps at the origin of a circular contig, reads `outside` beyond the ends of a linear one, and with
        `trim_terminal_repeats` a trimmed record is read in its trimmed coordinates.  `out`: the device tensor to write (anything
        with `__cuda_array_interface__`), `None`: a torch tensor allocated under torch's current stream; `stream`: the stream that
        last used `out`.  Every option of `find_genes_batch` applies and `sequences` may be a `DeviceSequences`.  The request is a
        device call of its own: one tensor per request, so a request that `training_infos` would split into several device calls
        is a `ValueError`."""
        if not isinstance(windows, _cabi.GeneWindows):
            raise TypeError("`windows` must be a GeneWindows, not %r" % type(windows).__name__)
        return self._find_tensor_batch("find_windows_batch", sequences, windows, out, stream, translate, training_infos, regions, circular, sets,
                                       trim_terminal_repeats)

    def find_counts_batch(self, object sequences, object counts, *, object out=None, object stream=None, bint translate=False,
                          object training_infos=None, object regions=None, object circular=None, object sets=None,
                          object trim_terminal_repeats=None):
        """`find_genes_batch`, and the k-mers of every contig or of every gene counted into an `int32` tensor left in device memory:
        returns `(genes, device_counts)`, the list of `Genes` that `find_genes_batch` returns for the same arguments and a
        `DeviceCounts`.

        `counts`: a `KmerCounts` -- k, rows per contig, per gene or per contig over its genes, step, folded or binned by a table.
        The tensor is written on the device while the batch is resident, on the batch the finder called: a gene row is gene g of the
        request, contig after contig (`device_counts.gene_begin`), read in the gene's own direction and across the origin of a
        circular contig; a contig row is sequence i of the request, and with `trim_terminal_repeats` a trimmed record is counted in
        its trimmed coordinates, as a circle.  `out`: the `[R, S >= n_bins]` device tensor to write (anything with
        `__cuda_array_interface__`), `None`: a torch tensor allocated under torch's current stream; `stream`: the stream that last
        used `out`.  Every option of `find_genes_batch` applies and `sequences` may be a `DeviceSequences`.  The request is a device
        call of its own: one tensor per request, so a request that `training_infos` would split into several device calls is a
        `ValueError`."""
        if not isinstance(counts, _cabi.KmerCounts):
            raise TypeError("`counts` must be a KmerCounts, not %r" % type(counts).__name__)
        return self._find_tensor_batch("find_counts_batch", sequences, counts, out, stream, translate, training_infos, regions, circular, sets,
                                       trim_terminal_repeats)

    def find_groups_batch(self, object sequences, object groups, *, object out=None, object stream=None, bint translate=False,
                          object training_infos=None, object regions=None, object circular=None, object sets=None,
                          object trim_terminal_repeats=None):
        """`find_genes_batch`, and the genes with the same predicted protein (or the same bases) grouped on the device, exactly:
        returns `(genes, device_groups)`, the list of `Genes` that `find_genes_batch` returns for the same arguments and a
        `DeviceGroups`.

        `groups`: a `ProteinGroups` -- proteins or bases, and the translation's options.  Gene g of the request, contig after contig
        (`device_groups.gene_begin`), gets `group[g]`; the groups are numbered in order of first appearance, `representatives[u]` is
        the first gene of group u and `sizes[u]` its members; `digests[g]` is the portable digest of the gene's string
        (`ProteinGroups.digest_of`), with which the results of several requests can be merged.  Two genes share a group exactly when
        their strings are equal byte for byte.  The tensors are written while the batch is resident, on the batch the finder
        called, each contig under the table of the model that won it.  `out`: a `(group, representatives, sizes, digests)` tuple of
        int64 device tensors to write (anything with `__cuda_array_interface__`; `None` for any of the last three), omitted: torch
        tensors allocated under torch's current stream; `stream`: the stream that last used them.  Every option of
        `find_genes_batch` applies and `sequences` may be a `DeviceSequences`.  The request is a device call of its own: one set of
        tensors per request, so a request that `training_infos` would split into several device calls is a `ValueError`."""
        if not isinstance(groups, _cabi.ProteinGroups):
            raise TypeError("`groups` must be a ProteinGroups, not %r" % type(groups).__name__)
        return self._find_tensor_batch("find_groups_batch", sequences, groups, out, stream, translate, training_infos, regions, circular, sets,
                                       trim_terminal_repeats)

    def find_sketches_batch(self, object sequences, object sketches, *, object out=None, object stream=None, bint translate=False,
                            object training_infos=None, object regions=None, object circular=None, object sets=None,
                            object trim_terminal_repeats=None):
        """`find_genes_batch`, and a bottom-s MinHash sketch of every gene's predicted protein (or of its bases) on the device:
        returns `(genes, device_sketches)`, the list of `Genes` that `find_genes_batch` returns for the same arguments and a
        `DeviceSketches`.

        `sketches`: a `ProteinSketches` -- window length, sketch size, unit, seed, letter classes and the translation's options.
        Gene g of the request, contig after contig (`device_sketches.gene_begin`), gets row `sketches[g]`: its at most `size`
        smallest distinct window hashes in ascending order, `INT64_MAX` behind the `counts[g]` real ones; `windows[g]` is the number
        of its valid windows.  A sketch is a property of the gene's string alone (`ProteinSketches.sketch_of`), so the rows of
        several requests can be compared; `device_sketches.compare(pairs)` estimates the resemblance of pairs of rows on the device.
        The tensors are written while the batch is resident, on the batch the finder called, each contig under the table of the model
        that won it.  `out`: a `(sketches, counts, windows)` tuple of int64 device tensors to write (anything with
        `__cuda_array_interface__`; `None` for the last), omitted: torch tensors allocated under torch's current stream; `stream`:
        the stream that last used them.  Every option of `find_genes_batch` applies and `sequences` may be a `DeviceSequences`.  The
        request is a device call of its own: one set of tensors per request, so a request that `training_infos` would split into
        several device calls is a `ValueError`."""
        if not isinstance(sketches, _cabi.ProteinSketches):
            raise TypeError("`sketches` must be a ProteinSketches, not %r" % type(sketches).__name__)
        return self._find_tensor_batch("find_sketches_batch", sequences, sketches, out, stream, translate, training_infos, regions, circular, sets,
                                       trim_terminal_repeats)

    def find_clusters_batch(self, object sequences, object clusters, *, object out=None, object stream=None, bint translate=False,
                            object training_infos=None, object regions=None, object circular=None, object sets=None,
                            object trim_terminal_repeats=None):
        """`find_genes_batch`, and the genes whose predicted proteins (or bases) are near-copies of each other clustered on the
        device: returns `(genes, device_clusters)`, the list of `Genes` that `find_genes_batch` returns for the same arguments and a
        `DeviceClusters`.

        `clusters`: a `ProteinClusters` -- the `ProteinSketches` to sketch under, the probes, the least resemblance and the least
        union.  Exactly `find_sketches_batch` with `clusters.sketches` followed by `device_sketches.cluster(clusters)`: gene g of
        the request, contig after contig, gets `cluster[g]`; the clusters are numbered in order of their smallest members,
        `representatives[u]` is the member with the most valid windows and `sizes[u]` its members; `edges`, `edge_shared` and
        `edge_union` are the accepted pairs, for a linkage of the caller's own; `device_clusters.sketches` is the `DeviceSketches`.
        `out`: a `(cluster, representatives, sizes, edges, edge_shared, edge_union)` tuple of int64 device tensors to write
        (anything with `__cuda_array_interface__`; `None` for the second and third, and for the last three together), omitted:
        torch tensors allocated under torch's current stream; `stream`: the stream that last used them.  Every option of
        `find_genes_batch` applies and `sequences` may be a `DeviceSequences`.  The request is a device call of its own: one set of
        tensors per request, so a request that `training_infos` would split into several device calls is a `ValueError`."""
        if not isinstance(clusters, _cabi.ProteinClusters):
            raise TypeError("`clusters` must be a ProteinClusters, not %r" % type(clusters).__name__)
        return self._find_tensor_batch("find_clusters_batch", sequences, clusters, out, stream, translate, training_infos, regions, circular, sets,
                                       trim_terminal_repeats)

    def find_verified_clusters_batch(self, object sequences, object verified, *, object out=None, object stream=None,
                                     bint translate=False, object training_infos=None, object regions=None, object circular=None,
                                     object sets=None, object trim_terminal_repeats=None):
        """`find_genes_batch`, and the genes whose predicted proteins are near-copies of each other clustered on the device with
        every edge checked against the proteins themselves: returns `(genes, device_verified_clusters)`, the list of `Genes` that
        `find_genes_batch` returns for the same arguments and a `DeviceVerifiedClusters`.

        `verified`: a `VerifiedClusters` -- the `ProteinClusters` that proposes pairs from the sketches, the `ProteinAlignments`
        that decides them and the `ProteinTokens` the proteins are compared as.  Exactly `find_proteins_batch` with
        `verified.tokens`, `find_clusters_batch` with `verified.clusters`, `device_proteins.align(device_clusters.edges,
        verified.alignments)` and `device_clusters.relink(keep=passed)`, all in one device call on the resident batch: `cluster[g]`,
        `representatives[u]` and `sizes[u]` are the components under the edges that passed, numbered as `find_clusters_batch`
        numbers them; `edge_distance` and `edge_passed` say what became of every edge of `candidates.edges`; `candidates` is the
        `DeviceClusters` of the sketch stage and `proteins` the `DeviceProteins`.  `out`: a `(cluster, representatives, sizes)`
        triple of int64 device tensors to write (anything with `__cuda_array_interface__`; `None` for the last two), omitted:
        torch tensors allocated under torch's current stream; the tokens, sketches and edge tensors are always new torch tensors.
        `stream`: the stream that last used `out`.  Every option of `find_genes_batch` applies and `sequences` may be a
        `DeviceSequences`.  The request is a device call of its own: one set of tensors per request, so a request that
        `training_infos` would split into several device calls is a `ValueError`."""
        if not isinstance(verified, _cabi.VerifiedClusters):
            raise TypeError("`verified` must be a VerifiedClusters, not %r" % type(verified).__name__)
        return self._find_tensor_batch("find_verified_clusters_batch", sequences, verified, out, stream, translate, training_infos, regions,
                                       circular, sets, trim_terminal_repeats)

    def find_starts_batch(self, object sequences, object starts, *, object out=None, object stream=None, bint translate=False,
                          object training_infos=None, object regions=None, object circular=None, object sets=None,
                          object trim_terminal_repeats=None):
        """`find_genes_batch`, and every candidate start site of every gene left in device memory: returns `(genes, device_starts)`,
        the list of `Genes` that `find_genes_batch` returns for the same arguments and a `DeviceStarts`.

        `starts`: a `StartCandidates` -- the score columns, element types, ragged or padded layout.  For gene g of the request, contig
        after contig (`device_starts.gene_begin`), the tensors hold all start nodes of its ORF in reading direction, outermost first,
        with their position, start codon type and scores under the winning model; `device_starts.chosen[g]` is the start the finder
        chose.  They are written while the request still holds its context, from the node arrays the finder left on the device: the
        call keeps them there (`PGA_NODES_DEVICE`) also when the finder was created with `keep_nodes=False`.  `out`: a `(positions,
        types, scores)` triple of device tensors to write (anything with `__cuda_array_interface__`), `None`: torch tensors
        allocated under torch's current stream; `stream`: the stream that last used `out`.  Every option of `find_genes_batch`
        applies but `circular` and `trim_terminal_repeats` (the nodes of a circle live in the coordinates of the rotated sequence, as
        for `write_scores`), and `sequences` may be a `DeviceSequences`.  The request is a device call of its own: one set of
        tensors per request, so a request that `training_infos` would split into several device calls is a `ValueError`."""
        if not isinstance(starts, _cabi.StartCandidates):
            raise TypeError("`starts` must be a StartCandidates, not %r" % type(starts).__name__)
        if circular is not None and circular is not False and circular is not True:
            circular = [bool(x) for x in circular]        # (a list that flags nothing asks for nothing: as in find_genes_batch)
        if (circular is True or (circular and any(circular))) or (trim_terminal_repeats is not None and trim_terminal_repeats is not False):
            raise ValueError("find_starts_batch: " + _cabi._NO_START_CANDIDATES)
        return self._find_tensor_batch("find_starts_batch", sequences, starts, out, stream, translate, training_infos, regions, circular, sets,
                                       None)

    cdef tuple _find_tensor_batch(self, str method, object sequences, object spec, object out, object stream, bint translate,
                                  object training_infos, object regions, object circular, object sets, object trim_terminal_repeats):
        """What the nine `find_*_batch` methods with a device-tensor output share (proteins, labels, windows, counts, groups,
        sketches, clusters, verified clusters, starts): (the `Genes` of `find_genes_batch`, what the rule `spec` wrote on the device)."""
        cdef dict tok = {"spec": spec, "out": out, "stream": stream, "result": None, "method": method}
        cdef list circ, tr_search
        cdef object dev, set_ids, tr_params
        dev, sequences, circ, set_ids, tr_search, tr_params = self._batch_options(sequences, training_infos, circular, sets, trim_terminal_repeats)
        sequences = list(sequences)
        if not sequences:
            raise ValueError("%s needs at least one sequence" % method)
        if dev is not None:
            genes = self._find_genes_device(dev, translate, training_infos, regions, circ, set_ids, tr_search, tr_params, tok)
        elif training_infos is not None:
            genes = self._find_genes_models(sequences, translate, training_infos, regions, circ, tr_search, tr_params, tok)
        else:
            if not self.meta and self.training_info is None:
                raise RuntimeError("cannot find genes without having trained in single mode")
            genes = self._find_genes_sets(self._wrap_sequences(sequences, regions), translate, set_ids, circ, tr_search, tr_params, tok)
        return genes, tok["result"]

    cdef tuple _batch_options(self, object sequences, object training_infos, object circular, object sets, object trim_terminal_repeats):
        """The options of `find_genes_batch` and of the nine `find_*_batch` methods with a device-tensor output, checked against each
        other and against the number of sequences: (the DeviceSequences or None, the sequences, circular flags, set ids,
        terminal-repeat search and its parameters)."""
        cdef list circ = None
        cdef object dev = None
        if isinstance(sequences, _DeviceSequences):
            dev = sequences
            sequences = [None] * len(dev)         # (the options below only count them)
        cdef object set_ids = None
        cdef list tr_search = None
        cdef object tr_params = None
        if trim_terminal_repeats is not None and trim_terminal_repeats is not False:
            sequences = list(sequences)
            if sets is not None:
                raise ValueError("`sets` cannot be combined with `trim_terminal_repeats`: the second pass of a circular call holds only "
                                 "the circular members of a set")
            tr_search, tr_params = _terminal_repeat_option(trim_terminal_repeats, len(sequences))
        if sets is not None:
            sequences = list(sequences)
            if not self.meta:
                raise ValueError("`sets` is a meta-mode option: this finder is in single mode")
            if training_infos is not None:
                raise ValueError("`sets` cannot be combined with `training_infos` (a single-mode option)")
            if circular is not None and circular is not False:
                raise ValueError("`sets` cannot be combined with `circular`: the second pass of a circular call holds only the "
                                 "circular members of a set")
            labels = list(sets)
            if len(labels) != len(sequences):
                raise ValueError("`sets` has %d entries for %d sequences" % (len(labels), len(sequences)))
            set_ids = np.full(max(len(labels), 1), -1, np.int32)
            seen = {}
            for k, lab in enumerate(labels):
                if lab is not None:
                    set_ids[k] = seen.setdefault(lab, len(seen))
        if circular is not None and circular is not False:
            sequences = list(sequences)
            if circular is True:
                circ = [True] * len(sequences)
            else:
                circ = [bool(x) for x in circular]
                if len(circ) != len(sequences):
                    raise ValueError("`circular` has %d entries for %d sequences" % (len(circ), len(sequences)))
            if not any(circ):
                circ = None
        return dev, sequences, circ, set_ids, tr_search, tr_params

    cdef list _wrap_sequences(self, object sequences, object regions=None):
        """The finder's masking rule on every sequence (the reference always re-wraps, lib.pyx:5433-5438): a Sequence that already
        follows it is used as it is.  The regions a Sequence carries stay with it; `regions` (one entry per sequence or None) are
        the call's own and join them."""
        cdef list seqs = []
        cdef list given = list(sequences)
        cdef list extra = None
        cdef Py_ssize_t i
        cdef Sequence q
        if regions is not None:
            extra = list(regions)
            if len(extra) != len(given):
                raise ValueError("`regions` has %d entries for %d sequences" % (len(extra), len(given)))
        for i in range(len(given)):
            s = given[i]
            r = extra[i] if extra is not None else None
            which = "sequence %d: " % i if len(given) > 1 else ""
            if isinstance(s, Sequence):
                q = <Sequence> s
                if r is not None:
                    r = _check_regions(r, len(q.data), which)
                    if r is not None and q._regions is not None:
                        r = np.concatenate([q._regions, r])
                rules = self.mask or self.mask_lowercase
                if (q.mask != self.mask or q.mask_lowercase != self.mask_lowercase or (rules and <int> q.mask_size != self.min_mask)
                        or r is not None):
                    s = Sequence(q.data, mask=self.mask, mask_size=self.min_mask, mask_lowercase=self.mask_lowercase)
                    (<Sequence> s)._regions = r if r is not None else q._regions
            else:
                s = Sequence(s, mask=self.mask, mask_size=self.min_mask, mask_lowercase=self.mask_lowercase)
                if r is not None:
                    (<Sequence> s)._regions = _check_regions(r, len((<Sequence> s).data), which)
            seqs.append(s)
        return seqs

    cdef list _model_calls(self, list lengths, list tinfs):
        """The device calls of a request with a model per sequence: consecutive runs of sequence indices under the base budget
        (`coalesce_bases`) and at most four distinct translation tables, what one context's model set holds."""
        cdef list calls = [], cur = []
        cdef set tables = set()
        cdef int64_t bases = 0, nb
        cdef Py_ssize_t i
        for i in range(len(lengths)):
            nb = lengths[i]
            tt = (<TrainingInfo> tinfs[i]).translation_table
            if cur and (bases + nb > self.coalesce_bases or (tt not in tables and len(tables) == 4)):
                calls.append(cur); cur = []; tables = set(); bases = 0
            cur.append(i); tables.add(tt); bases += nb
        calls.append(cur)
        return calls

    cdef _FinderSlot _own_slot(self):
        """A context for one request alone (never coalesced with other callers', like the training takes one): waits until one is
        free and marks it busy."""
        cdef _FinderSlot slot
        with self._cv:
            while True:
                slot = self._free_slot()
                if slot is not None:
                    break
                self._cv.wait()
            slot.busy = True
        return slot

    cdef int _single_mode_only(self) except -1:
        if self.meta:
            raise ValueError("`training_infos` is a single-mode option: this finder is in meta mode")
        return 0

    cdef list _checked_training_infos(self, list tinfs, Py_ssize_t n):
        """`training_infos=` of a call over n sequences, as a list: one `TrainingInfo` per sequence."""
        if len(tinfs) != n:
            raise ValueError("`training_infos` has %d entries for %d sequences" % (len(tinfs), n))
        for i, t in enumerate(tinfs):
            if not isinstance(t, TrainingInfo):
                raise TypeError("training_infos[%d] is not a TrainingInfo (%r)" % (i, type(t).__name__))
        return tinfs

    cdef list _own_calls(self, list calls, list seqs, list circ, object set_ids, list tr_search, object tr_params, object tokens,
                         list tinfs=None, object dev=None, list regs=None):
        """The device calls of a request that takes a context for itself: `calls` holds the sequence indices of every call (runs in
        input order), the options come per sequence of the request.  Returns (request, tinf_of, dev, dev_regions) per device call,
        as `_run_alone` takes them; a call over part of a `DeviceSequences` takes its (offset, length) pairs: no data moves."""
        cdef _FindRequest req
        cdef list out = []
        for idx in calls:
            req = _FindRequest.__new__(_FindRequest)
            req.seqs = [seqs[i] for i in idx]
            req.circ = None if circ is None else [circ[i] for i in idx]
            req.sets = set_ids
            req.tr_search = None if tr_search is None else [tr_search[i] for i in idx]
            req.tr_params = tr_params if tr_search is not None else None
            req.tokens = tokens
            out.append((req, None if tinfs is None else [tinfs[i] for i in idx],
                        None if dev is None else (dev if len(idx) == len(seqs) else dev.take(idx)),
                        None if regs is None else [regs[i] for i in idx]))
        return out

    cdef list _run_alone(self, list calls, bint translate):
        """Run the device calls of one request (`_own_calls`) in order on a context taken for it alone, never coalesced with other
        callers' sequences: numbers the sequences, counts the calls, returns the `Genes` in input order."""
        cdef _FindRequest req
        cdef _FinderSlot slot
        cdef list out = []
        with self._lock:
            for call in calls:
                req = call[0]
                req.first_id = self._num_seq
                self._num_seq += len(req.seqs)
        slot = self._own_slot()
        try:
            for req, tinf_of, dev, regs in calls:
                out.extend(self._device_call(slot, req.seqs, translate, [req], tinf_of, dev, regs))
                with self._lock:
                    self.stats["device_calls"] += 1
                    self.stats["sequences"] += len(req.seqs)
        finally:
            with self._lock:
                self._release_slot(slot)
        return out

    def _find_genes_models(self, object sequences, bint translate, object training_infos, object regions=None, list circ=None,
                           list tr_search=None, object tr_params=None, object tokens=None):
        """`find_genes_batch(..., training_infos=...)`: single mode with a model per sequence (`pga_find_genes_models`).  The
        sequences go in device calls of at most `coalesce_bases` bases and four translation tables (what one context's model set
        holds); identical `TrainingInfo` objects are loaded once per call."""
        self._single_mode_only()
        cdef list tinfs = list(training_infos)
        cdef list seqs = self._wrap_sequences(sequences, regions)
        self._checked_training_infos(tinfs, len(seqs))
        if not seqs:
            return []
        cdef list calls = self._model_calls([len((<Sequence> q).data) for q in seqs], tinfs)
        _one_call_for_tokens(tokens, calls)
        return self._run_alone(self._own_calls(calls, seqs, circ, None, tr_search, tr_params, tokens, tinfs), translate)

    def _find_genes_device(self, object dev, bint translate, object training_infos, object regions, list circ, object set_ids,
                           list tr_search, object tr_params, object tokens=None):
        """`find_genes_batch(DeviceSequences)`: a request of its own, never coalesced with other callers' sequences (as with `sets`).
        With `training_infos` it splits into device calls as `_find_genes_models` does, each over a subset of the (offset, length)
        pairs of `dev`: no data moves."""
        cdef Py_ssize_t n = len(dev), i
        cdef list tinfs = None, regs = None, calls
        if training_infos is not None:
            self._single_mode_only()
            tinfs = self._checked_training_infos(list(training_infos), n)
        elif not self.meta and self.training_info is None:
            raise RuntimeError("cannot find genes without having trained in single mode")
        if regions is not None:
            regs = list(regions)
            if len(regs) != n:
                raise ValueError("`regions` has %d entries for %d sequences" % (len(regs), n))
            for i in range(n):
                regs[i] = _check_regions(regs[i], int(dev.lengths[i]), "sequence %d: " % i if n > 1 else "")
        if n == 0:
            return []
        calls = [list(range(n))] if tinfs is None else self._model_calls(dev.lengths.tolist(), tinfs)
        _one_call_for_tokens(tokens, calls)
        # (the Sequence objects are made from the packed letters, in the device call)
        return self._run_alone(self._own_calls(calls, [None] * n, circ, set_ids, tr_search, tr_params, tokens, tinfs, dev, regs), translate)

    def _find_genes_sets(self, list seqs, bint translate, object set_ids, list circ=None, list tr_search=None, object tr_params=None,
                         object tokens=None):
        """`find_genes_batch(..., sets=...)`: every set must sit in one device call, so the request takes a context for itself and is
        never coalesced with other callers' sequences.  `find_proteins_batch` on host sequences rides the same way, with the options
        a set cannot have."""
        return self._run_alone(self._own_calls([list(range(len(seqs)))], seqs, circ, set_ids, tr_search, tr_params, tokens), translate)

    cdef int _release_slot(self, _FinderSlot slot) except -1:
        """(lock held) The context goes to the oldest waiting request that has no context yet, or back to the pool."""
        cdef _FindRequest r
        for r in self._pending:
            if r.lead is None:
                r.lead = slot
                _signal(r)
                return 0
        slot.busy = False
        self._cv.notify_all()
        return 0

    cdef int _run(self, _FinderSlot slot, list take) except -1:
        """One device call over the sequences of every request in `take`; each request gets its `Genes` (or the error)."""
        cdef _FindRequest r
        cdef list seqs = []
        for r in take:
            seqs.extend(r.seqs)
        cdef bint translate = (<_FindRequest> take[0]).translate
        st = self.stats
        try:
            out = self._device_call(slot, seqs, translate, take)
        except Exception as e:
            if len(take) == 1:
                (<_FindRequest> take[0]).error = e
                return 0
            # A device call that carries the sequences of several callers failed.  The reference's calls have private state: one
            # caller's bad input never fails another's.  So every request rides a device call of its own now, and gets its own
            # result or its own error.
            st["device_calls_retried_per_request"] = st.get("device_calls_retried_per_request", 0) + 1
            for r in take:
                try:
                    r.out = self._device_call(slot, r.seqs, translate, [r])
                    st["device_calls"] += 1
                    st["sequences"] += len(r.seqs)
                except Exception as e1:
                    r.error = e1
            return 0
        # (anything else -- KeyboardInterrupt, SystemExit -- is this thread being stopped: it goes up, and the caller's clean-up tells
        #  the passengers that their device call was interrupted)
        cdef ssize_t k = 0
        for r in take:
            r.out = out[k:k + len(r.seqs)]
            k += len(r.seqs)
        st["device_calls"] += 1
        st["sequences"] += len(seqs)
        if len(take) > st["max_calls_per_device_call"]:
            st["max_calls_per_device_call"] = len(take)
        return 0

    cdef list _device_call(self, _FinderSlot slot, list seqs, bint translate, list take, list tinf_of=None, object dev=None,
                           list dev_regions=None):
        # tinf_of: one TrainingInfo per sequence (single mode, a model per sequence: pga_find_genes_models), or None
        # dev: the sequences lie in device memory (a DeviceSequences; dev_regions: their checked regions or None) -- the batch is packed
        #      there, `seqs` holds placeholders and is filled from the packed letters, fetched once
        cdef int n = len(seqs), i, rc
        cdef const char** ptrs = NULL
        cdef int64_t* lens = NULL
        cdef pga_params p
        cdef pga_result* res = NULL
        cdef _CallState o = _call_options(take, n)
        cdef object moc = None
        cdef bint masked = self.mask_lowercase       # a mask source beyond params.mask: the call goes through a resident batch
        p.closed = self.closed; p.min_gene = self.min_gene; p.min_edge_gene = self.min_edge_gene
        p.max_overlap = self.max_overlap; p.meta = self.meta; p.want_nodes = self.keep_nodes
        p.mask = self.mask; p.min_mask = self.min_mask
        if o.tok is not None and getattr(o.tok["spec"], "needs_nodes", False) and not self.keep_nodes:
            p.want_nodes = 2                         # PGA_NODES_DEVICE: the rule reads the node arrays, and only on the device
        try:
            if dev is None:
                ptrs = <const char**> malloc(sizeof(char*) * max(n, 1))
                lens = <int64_t*> malloc(sizeof(int64_t) * max(n, 1))
                if ptrs == NULL or lens == NULL:
                    raise MemoryError()
                for i in range(n):
                    ptrs[i] = PyBytes_AS_STRING((<Sequence> seqs[i]).data)
                    lens[i] = len((<Sequence> seqs[i]).data)
                    if (<Sequence> seqs[i])._regions is not None:
                        masked = True
            elif dev_regions is not None:
                for r in dev_regions:
                    if r is not None:
                        masked = True
            if tinf_of is None:
                self._ensure_models(slot)
            else:
                moc = self._load_models_of(slot, tinf_of)[1]
            if (dev is None and moc is None and not translate and not masked and o.flags is None and o.set_ids is None
                    and o.tr_params is None and o.tok is None):
                with nogil:
                    rc = pga_find_genes_batch(slot.ctx, n, ptrs, lens, &p, &res)
                if rc != PGA_OK:
                    _raise_for(slot.ctx, rc, "pga_find_genes_batch")
            else:
                seqs = self._resident_call(slot.ctx, &p, o, seqs, masked, translate, moc, tinf_of, ptrs, lens, dev, dev_regions, &res)
            return self._genes_of_call(o, seqs, res, tinf_of)
        finally:
            free(ptrs); free(lens)
            if res != NULL:
                pga_result_free(res)

    cdef list _sequences_of_batch(self, pga_ctx* ctx, pga_batch* batch, object dev, list dev_regions):
        """The host copy of the letters of a batch packed from `dev`: one device-to-host copy of the packed batch, cut into the usual
        Sequence objects."""
        cdef int n = len(dev), i, rc
        cdef int64_t at = 0
        cdef Sequence tseq
        cdef list seqs = []
        letters = np.empty(max(int(dev.total), 1), np.uint8)
        cdef size_t p_letters = letters.ctypes.data
        with nogil:
            rc = pga_batch_read(ctx, batch, -1, <char*> p_letters)
        if rc != PGA_OK:
            _raise_for(ctx, rc, "pga_batch_read")
        for i in range(n):
            tseq = Sequence(letters[at:at + int(dev.lengths[i])].tobytes(), mask=self.mask, mask_size=self.min_mask,
                            mask_lowercase=self.mask_lowercase)
            at += int(dev.lengths[i])
            if dev_regions is not None and dev_regions[i] is not None:
                tseq._regions = dev_regions[i]
            seqs.append(tseq)
        return seqs

    cdef list _resident_call(self, pga_ctx* ctx, pga_params* p, _CallState o, list seqs, bint masked, bint translate, object moc,
                             list tinf_of, const char** ptrs, const int64_t* lens, object dev, list dev_regions, pga_result** res):
        """A device call through a resident batch: made from the host pointers or packed from `dev`, given the options of the call,
        handed to the finder (`moc`: the loaded model of every sequence, or None), read for what the options report and for
        translations and tokens, and released.  Fills `res` and the arrays of `o`; returns the Sequence objects of the call -- `seqs`,
        or with `dev` the ones made from the packed letters."""
        cdef int n = len(seqs), rc
        cdef pga_batch* batch = NULL
        cdef pga_batch* whole = NULL                 # the batch as uploaded, while `batch` is its trimmed copy
        cdef pga_batch* trimmed = NULL
        cdef size_t p_moc = 0, p_flags = 0, p_cuts = 0, p_sets = 0, p_smodel = 0, p_sscore = 0, p_mscores = 0
        try:
            if dev is not None:
                batch = _device_batch(ctx, dev)
                seqs = self._sequences_of_batch(ctx, batch, dev, dev_regions)
            else:
                rc = pga_batch_create(ctx, n, ptrs, lens, &batch)
                if rc != PGA_OK:
                    _raise_for(ctx, rc, "pga_batch_create")
            if masked:
                _attach_masks(ctx, batch, seqs, self.mask_lowercase)
            if o.flags is not None:
                p_flags = o.flags.ctypes.data; p_cuts = o.cuts.ctypes.data
                pga_batch_set_circular(batch, <const uint8_t*> p_flags)
            if o.set_ids is not None:
                p_sets = o.set_ids.ctypes.data
                rc = pga_batch_set_sets(batch, <const int32_t*> p_sets)
                if rc != PGA_OK:
                    _raise_for(ctx, rc, "pga_batch_set_sets")
            if o.tr_params is not None:
                trimmed = _trimmed_batch(ctx, batch, o.tr_flags.ctypes.data, o.tr_params, o.tr_match.ctypes.data, o.tr_trim.ctypes.data)
                if trimmed != NULL:
                    whole = batch; batch = trimmed
            if moc is not None:
                p_moc = moc.ctypes.data
                with nogil:
                    rc = pga_find_genes_models(ctx, batch, p, <const int32_t*> p_moc, res)
                if rc != PGA_OK:
                    _raise_for(ctx, rc, "pga_find_genes_models")
            else:
                with nogil:
                    rc = pga_find_genes(ctx, batch, p, res)
                if rc != PGA_OK:
                    _raise_for(ctx, rc, "pga_find_genes")
            if o.set_ids is not None:
                o.n_models = len(self.metagenomic_bins)
                o.set_model = np.full(max(n, 1), -1, np.int32); o.set_score = np.full(max(n, 1), np.nan, np.float64)
                o.model_scores = np.full(max(n * o.n_models, 1), np.nan, np.float64)
                p_smodel = o.set_model.ctypes.data; p_sscore = o.set_score.ctypes.data; p_mscores = o.model_scores.ctypes.data
                pga_set_choice(ctx, n, <int32_t*> p_smodel, <double*> p_sscore)
                pga_model_scores(ctx, n, o.n_models, <double*> p_mscores)
            if o.flags is not None:
                pga_circular_cuts(ctx, n, <int32_t*> p_cuts)
            if translate:
                o.prot, o.prot_off, o.tables = self._translate(ctx, batch, res[0], n, tinf_of)
            if o.tok is not None:
                if o.tok["spec"].per_contig == "lengths":
                    # (the batch the finder called: without the bases `_trimmed_batch` took off)
                    per_contig = np.array([len((<Sequence> q).data) for q in seqs], np.int64)
                    if trimmed != NULL:
                        per_contig -= o.tr_trim[:n]
                else:
                    per_contig = self._tables_of(res[0], n, tinf_of)[:n]
                self._device_tensor(ctx, batch, res[0], per_contig, o.tok)
        finally:
            if batch != NULL:
                pga_batch_free(batch)
            if whole != NULL:
                pga_batch_free(whole)
        return seqs

    cdef list _genes_of_call(self, _CallState o, list seqs, pga_result* res, list tinf_of):
        """One `Genes` per sequence of a device call, from its result and from what the call's options reported."""
        cdef int n = len(seqs), i, j
        cdef pga_contig_result* cr
        cdef Genes genes
        cdef Sequence seq, tseq
        cdef list out = []
        if o.tr_trim is not None:
            seqs = list(seqs)                      # (the caller's list keeps the records as they came)
            for i in range(n):
                if o.tr_trim[i] > 0:
                    # the record without the second copy of its first bases: what the device called, and what the host writers read
                    o.flags[i] = 1
                    tseq = <Sequence> seqs[i]
                    r_clip = None
                    if tseq._regions is not None:
                        r_clip = np.minimum(tseq._regions, len(tseq.data) - int(o.tr_trim[i])).astype(np.int32)
                        r_clip = r_clip[r_clip[:, 0] < r_clip[:, 1]]
                        if len(r_clip) == 0:
                            r_clip = None
                    seq = Sequence(tseq.data[:len(tseq.data) - int(o.tr_trim[i])], mask=tseq.mask, mask_size=tseq.mask_size,
                                   mask_lowercase=tseq.mask_lowercase)
                    seq._regions = r_clip
                    seqs[i] = seq
        for i in range(n):
            cr = &res.contigs[i]
            seq = <Sequence> seqs[i]
            genes = Genes.__new__(Genes)
            genes.sequence = seq
            seq._gc = cr.gc
            seq._unknown = cr.n_unknown
            if seq._masks is None:
                seq._masks = []
                if res.mask_off != NULL:
                    for j in range(res.mask_off[i], res.mask_off[i + 1]):
                        seq._masks.append(Mask(res.masks[2 * j], res.masks[2 * j + 1]))
            genes.meta = self.meta
            genes._num_seq = o.ids[i]
            genes.score = cr.score
            genes.circular = o.flags is not None and o.flags[i] != 0
            genes.cut = int(o.cuts[i]) if genes.circular else None
            genes.terminal_repeat = genes.terminal_repeat_match = None
            if o.tr_flags is not None and o.tr_flags[i]:
                genes.terminal_repeat = int(o.tr_trim[i]); genes.terminal_repeat_match = int(o.tr_match[i])
            if o.set_model is not None:
                genes.set_score = float(o.set_score[i]) if o.set_model[i] >= 0 else None
                ms = o.model_scores[i * o.n_models:(i + 1) * o.n_models]
                genes.model_scores = {j: float(ms[j]) for j in range(o.n_models) if ms[j] == ms[j]}
            if self.meta:
                if cr.model >= 0:
                    genes.metagenomic_bin = self.metagenomic_bins[cr.model]
                    genes.training_info = genes.metagenomic_bin.training_info
                else:
                    genes.metagenomic_bin = genes.training_info = None
            else:
                genes.metagenomic_bin = None
                genes.training_info = self.training_info if tinf_of is None else tinf_of[i]
            genes._nodes = None
            genes._node_blob = None
            genes._node_n = 0
            if self.keep_nodes and res.nodes != NULL:
                genes._node_blob = _pack_nodes(&res.nodes[i])
                genes._node_n = res.nodes[i].n
            genes._genes = None
            genes._n = cr.n_genes
            genes._recs = PyBytes_FromStringAndSize(<const char*> &res.genes[cr.gene_begin], cr.n_genes * sizeof(pga_gene)) if cr.n_genes > 0 else b""
            genes._prot = None; genes._prot_off = None; genes._prot_tt = 0
            if o.prot is not None:
                genes._prot = o.prot[o.prot_off[cr.gene_begin]:o.prot_off[cr.gene_begin + cr.n_genes]].tobytes()
                genes._prot_off = (o.prot_off[cr.gene_begin:cr.gene_begin + cr.n_genes + 1] - o.prot_off[cr.gene_begin]).copy()
                genes._prot_tt = int(o.tables[i])
            out.append(genes)
        return out

    cdef int _device_tensor(self, pga_ctx* ctx, pga_batch* batch, pga_result* res, object per_contig, dict tok) except -1:
        """What the request's rule makes of the genes of `res` -- any of the nine rules of `_cabi` (protein tokens, base labels, gene
        windows, k-mer counts, protein groups, protein sketches, protein clusters, verified clusters, start candidates) -- into the request's device tensors while the batch
        the finder called is resident (through the rule's `write`, the raw layer's marshalling); `per_contig`: what the rule needs of
        every contig, tables or lengths (`spec.per_contig`).  Leaves the rule's `Device*` result in `tok`."""
        genes = np.zeros(0, _cabi.GENE_DTYPE)
        if res.n_genes > 0:
            genes = np.frombuffer(PyBytes_FromStringAndSize(<const char*> res.genes, res.n_genes * sizeof(pga_gene)), dtype=_cabi.GENE_DTYPE)
        tok["result"] = tok["spec"].write(_cabi.load(), ctypes.c_void_p(<size_t> ctx), ctypes.c_void_p(<size_t> batch), self.device, genes,
                                          per_contig, tok["out"], tok["stream"])
        return 0

    cdef object _tables_of(self, pga_result* res, int n, list tinf_of):
        """The translation table every contig of `res` was called under (int32; 11 where no model won)."""
        cdef int i
        cdef pga_contig_result* cr
        tables = np.full(max(n, 1), 11, np.int32)
        for i in range(n):
            cr = &res.contigs[i]
            if self.meta:
                if cr.model >= 0:
                    tables[i] = (<MetagenomicBin> self.metagenomic_bins[cr.model]).training_info.translation_table
            elif tinf_of is not None:
                tables[i] = (<TrainingInfo> tinf_of[i]).translation_table
            else:
                tables[i] = (<TrainingInfo> self.training_info).translation_table
        return tables

    cdef tuple _translate(self, pga_ctx* ctx, pga_batch* batch, pga_result* res, int n, list tinf_of):
        """Proteins of every gene of `res` on the device: (letters, offsets, table of every contig)."""
        cdef int rc
        cdef int64_t j, ng
        cdef size_t p_tab, p_off, p_out
        prot_off = np.zeros(res.n_genes + 1, np.int64)
        tables = self._tables_of(res, n, tinf_of)
        for j in range(res.n_genes):
            prot_off[j + 1] = prot_off[j] + (res.genes[j].end - res.genes[j].begin + 1) // 3
        prot = np.zeros(max(int(prot_off[res.n_genes]), 1), np.uint8)
        p_tab = tables.ctypes.data; p_off = prot_off.ctypes.data; p_out = prot.ctypes.data
        ng = res.n_genes
        with nogil:
            rc = pga_translate_genes(ctx, batch, ng, res.genes, <const int32_t*> p_tab, 88, 1, 1,
                                     <const int64_t*> p_off, <char*> p_out)
        if rc != PGA_OK:
            _raise_for(ctx, rc, "pga_translate_genes")
        return prot, prot_off, tables

    cdef tuple _load_models_of(self, _FinderSlot slot, list tinf_of):
        """Load the distinct `TrainingInfo` objects of `tinf_of` (by identity, first-seen order) into the slot's context; returns
        them and the model index of every sequence.  The slot no longer holds the finder's own model set afterwards."""
        cdef int rc, i, n
        cdef const pga_training** ptrs
        cdef dict index = {}
        cdef list models = []
        moc = np.zeros(max(len(tinf_of), 1), np.int32)
        for i, t in enumerate(tinf_of):
            k = index.get(id(t))
            if k is None:
                k = index[id(t)] = len(models)
                models.append(t)
            moc[i] = k
        if slot.ctx == NULL:
            rc = pga_create(self.device, &slot.ctx)
            if rc != PGA_OK:
                slot.ctx = NULL
                _raise_for(NULL, rc, "pga_create")
        n = len(models)
        blobs = [(<TrainingInfo> t)._raw for t in models]
        ptrs = <const pga_training**> malloc(sizeof(void*) * max(n, 1))
        if ptrs == NULL:
            raise MemoryError()
        slot.models_loaded = False        # whatever happens now, the next ordinary call loads the finder's models again
        try:
            for i in range(n):
                ptrs[i] = <const pga_training*> <size_t> blobs[i].ctypes.data
            rc = pga_set_models(slot.ctx, ptrs, n)
        finally:
            free(ptrs)
        if rc != PGA_OK:
            _raise_for(slot.ctx, rc, "pga_set_models")
        return models, moc

    cdef Sequence _training_sequence(self, object sequence, tuple sequences, str which, object regions=None):
        """One genome as `train(sequence, *sequences)` takes it: several contigs joined with `TTAATTAATTAA` linkers like in
        Prodigal (ref: lib.pyx:5510-5532), then the length rules (`which` names the genome in the messages).  `regions`: the
        intervals of the one sequence, or with several contigs one entry (None or intervals) per contig -- they travel with
        their contig through the join."""
        import warnings
        cdef Sequence seq
        cdef list joined = None, per
        cdef Py_ssize_t at = 0, k
        if regions is not None and sequences:
            per = list(regions)
            if len(per) != 1 + len(sequences):
                raise ValueError("%s`regions` has %d entries for %d contigs" % (which, len(per), 1 + len(sequences)))
            joined = []
            for k, x in enumerate((sequence,) + sequences):
                r = _check_regions(per[k], len(x), "%scontig %d: " % (which, k))
                if r is not None:
                    joined.extend([(int(b) + at, int(e) + at) for b, e in r.tolist()])
                at += len(x) + 12
            regions = joined
        if isinstance(sequence, Sequence):
            if sequences:
                raise NotImplementedError("cannot use more than one `Sequence` object in `GeneFinder.train`")
            seq = Sequence(sequence, mask=self.mask, mask_size=self.min_mask, mask_lowercase=self.mask_lowercase)
            if regions is not None:
                r = _check_regions(regions, len(seq.data), which)
                if r is not None:
                    seq._regions = r if seq._regions is None else np.concatenate([seq._regions, r])
        elif isinstance(sequence, str):
            if sequences:
                sequence = "TTAATTAATTAA".join(list((sequence,) + sequences) + [""])
            seq = Sequence(sequence, mask=self.mask, mask_size=self.min_mask, mask_lowercase=self.mask_lowercase)
            seq._regions = _check_regions(regions, len(seq.data), which)
        else:
            if sequences:
                sequence = b"TTAATTAATTAA".join([bytes(memoryview(x)) for x in (sequence,) + sequences] + [b""])
            seq = Sequence(sequence, mask=self.mask, mask_size=self.min_mask, mask_lowercase=self.mask_lowercase)
            seq._regions = _check_regions(regions, len(seq.data), which)
        if len(seq) < MIN_SINGLE_GENOME:
            raise ValueError("%ssequence must be at least %d characters (%d found)" % (which, MIN_SINGLE_GENOME, len(seq)))
        elif len(seq) < IDEAL_SINGLE_GENOME:
            warnings.warn("%ssequence should be at least %d characters (%d found)" % (which, IDEAL_SINGLE_GENOME, len(seq)))
        return seq

    def select_translation_table(self, object genomes, *, object candidates=(11, 4), double min_gain=0.05, double min_density=0.7,
                                 bint force_nonsd=False, double start_weight=4.35, object regions=None):
        """The translation table of every genome, chosen by coding density (`pyrodigal_amd.tables`), on the device.

        `regions`: one entry per genome, as `train` takes them (the intervals of a one-sequence genome, or one entry per contig);
        every candidate is trained and called under the same masks.

        A genome is one sequence or a list / tuple of contigs, as `train_batch` takes it.  For every candidate table it is trained
        (the contigs joined with linkers, this finder's options, `force_nonsd`, `start_weight`) and its contigs called with that
        model, one by one; the coding bases -- positions inside at least one gene -- are counted on the device where the gene
        records are (`pga_find_coding_bases`).  A candidate other than the first (the default) wins when it covers more than
        `min_gain` more of the genome and more than `min_density` of it; the best such candidate, else the default.

        Returns one read-only `TableSelection` per genome: `translation_table`, its `training_info`, `coding_density` and
        `coding_bases` of every candidate, `length`.  The genomes are uploaded once per device call and copied on the device for
        every candidate; only a few numbers per genome come back.  The finder's own `training_info` is left alone."""
        _refuse_device_input(genomes, "select_translation_table")
        if self.meta:
            raise RuntimeError("cannot use training sequence in metagenomic mode")
        cands = _tables.check_candidates(candidates)
        min_gain, min_density = _tables.check_thresholds(min_gain, min_density)
        cdef list gl = list(genomes)
        cdef list rl = None
        if regions is not None:
            rl = list(regions)
            if len(rl) != len(gl):
                raise ValueError("`regions` has %d entries for %d genomes" % (len(rl), len(gl)))
        return self._select_tables(gl, cands, min_gain, min_density, [bool(force_nonsd)] * len(gl), [float(start_weight)] * len(gl),
                                   "genome %d: ", list(range(len(gl))), rl)

    def _select_tables(self, list gl, tuple cands, double min_gain, double min_density, list fns, list sws, str which, list names,
                       list regions=None):
        """`select_translation_table` with one `force_nonsd` / `start_weight` per genome (`names[g]`: the genome's number in messages)."""
        cdef Py_ssize_t G = len(gl), K = len(cands), g, k
        if G == 0:
            return []
        # per genome: the joined training sequence (train's length rules) and the contigs as find_genes wraps them
        cdef list train_seqs = [], contigs = [], lengths = []
        for g in range(G):
            x = gl[g]
            parts = list(x) if isinstance(x, (list, tuple)) else [x]
            if not parts:
                raise ValueError((which % names[g]) + "no sequence")
            rg = regions[g] if regions is not None else None
            train_seqs.append(self._training_sequence(parts[0], tuple(parts[1:]), which % names[g], rg))
            cs = self._wrap_sequences(parts, None if rg is None else (list(rg) if len(parts) > 1 else [rg]))
            contigs.append(cs)
            lengths.append(sum([len((<Sequence> c).data) for c in cs]))
        # the device calls: consecutive genomes, every candidate of a genome in the same call; K copies of a genome count against
        # `coalesce_bases`, and at most _SELECT_MAX_MODELS models are loaded at once
        cdef list calls = [], cur = []
        cdef int64_t bases = 0, nb
        for g in range(G):
            nb = K * len((<Sequence> train_seqs[g]).data)
            if cur and (bases + nb > self.coalesce_bases or (len(cur) + 1) * K > _SELECT_MAX_MODELS):
                calls.append(cur); cur = []; bases = 0
            cur.append(g); bases += nb
        calls.append(cur)
        cdef list out = [None] * G
        cdef _FinderSlot slot
        with self._cv:
            while True:
                slot = self._free_slot()
                if slot is not None:
                    break
                self._cv.wait()
            slot.busy = True
        try:
            if slot.ctx == NULL:
                rc = pga_create(self.device, &slot.ctx)
                if rc != PGA_OK:
                    slot.ctx = NULL
                    _raise_for(NULL, rc, "pga_create")
            slot.models_loaded = False            # the training and the K models of every genome replace the loaded set
            for idx in calls:
                raws, cov = self._select_call(slot, idx, train_seqs, contigs, cands, fns, sws, names)
                for j, g in enumerate(idx):
                    coding = {cands[k]: int(cov[k, j]) for k in range(K)}
                    dens = {t: _tables.coding_density(n, lengths[g]) for t, n in coding.items()}
                    t = _tables.choose_table(dens, cands, min_gain, min_density)
                    k = cands.index(t)
                    out[g] = TableSelection(t, TrainingInfo(raw=raws[k][j]), coding, lengths[g])
        finally:
            with self._lock:
                self._release_slot(slot)
        return out

    cdef tuple _select_call(self, _FinderSlot slot, list idx, list train_seqs, list contigs, tuple cands, list fns, list sws,
                            list names):
        """One device call of `_select_tables` over the genomes `idx`: train every genome under every candidate, then call its
        contigs under each of those models and count the coding bases.  Returns (raws[k][j], coding[k, j]) for cands[k], idx[j]."""
        cdef Py_ssize_t n = len(idx), K = len(cands), nc, j, k, i, e
        cdef pga_ctx* ctx = slot.ctx
        cdef pga_params p
        cdef pga_batch* up = NULL
        cdef pga_batch* rep = NULL
        cdef const char** ptrs = NULL
        cdef int64_t* lens = NULL
        cdef const pga_training** mptrs = NULL
        cdef int rc
        cdef size_t p_coe, p_tt, p_sw, p_fn, p_out, p_st, p_moc, p_cov, p_ng, p_sc
        p.closed = self.closed; p.min_gene = self.min_gene; p.min_edge_gene = self.min_edge_gene
        p.max_overlap = self.max_overlap; p.meta = 0; p.want_nodes = 0
        p.mask = self.mask; p.min_mask = self.min_mask
        # 1. the joined genomes, uploaded once and copied K times on the device (entry k * n + j: genome idx[j] under cands[k])
        coe = np.tile(np.arange(n, dtype=np.int32), K)
        a_tt = np.repeat(np.array(cands, np.int32), n)
        a_sw = np.tile(np.array([sws[g] for g in idx], np.float64), K)
        a_fn = np.tile(np.array([int(fns[g]) for g in idx], np.int32), K)
        raw = np.zeros(n * K * TRAINING_INFO_SIZE, np.uint8)
        status = np.zeros(n * K, np.int32)
        p_coe = coe.ctypes.data; p_tt = a_tt.ctypes.data; p_sw = a_sw.ctypes.data; p_fn = a_fn.ctypes.data
        p_out = raw.ctypes.data; p_st = status.ctypes.data
        ptrs = <const char**> malloc(sizeof(char*) * max(n, 1))
        lens = <int64_t*> malloc(sizeof(int64_t) * max(n, 1))
        if ptrs == NULL or lens == NULL:
            free(ptrs); free(lens)
            raise MemoryError()
        try:
            for j in range(n):
                ptrs[j] = PyBytes_AS_STRING((<Sequence> train_seqs[idx[j]]).data)
                lens[j] = len((<Sequence> train_seqs[idx[j]]).data)
            rc = pga_batch_create(ctx, <int32_t> n, ptrs, lens, &up)
        finally:
            free(ptrs); free(lens)
        if rc != PGA_OK:
            _raise_for(ctx, rc, "pga_batch_create")
        try:
            _attach_masks(ctx, up, [train_seqs[g] for g in idx], self.mask_lowercase)      # the copies inherit them
            rc = pga_batch_replicate(ctx, up, <int32_t> (n * K), <const int32_t*> p_coe, &rep)
            if rc != PGA_OK:
                _raise_for(ctx, rc, "pga_batch_replicate")
            with nogil:
                rc = pga_train_batch(ctx, rep, &p, <const int32_t*> p_tt, <const double*> p_sw, <const int32_t*> p_fn, 0,
                                     <pga_training*> p_out, <int32_t*> p_st)
            if rc != PGA_OK:
                _raise_for(ctx, rc, "pga_train_batch")
        finally:
            pga_batch_free(rep); rep = NULL
            pga_batch_free(up); up = NULL
        for e in range(n * K):
            if status[e] != PGA_OK:
                raise ValueError("genome %d could not be trained with translation table %d: no start / stop node in the sequence"
                                 % (names[idx[e % n]], cands[e // n]))
        # 2. the contigs, uploaded once and copied K times; contig i of genome j under model k * n + j
        cdef list cseqs = []
        cdef list genome_of = []
        for j in range(n):
            for c in contigs[idx[j]]:
                cseqs.append(c); genome_of.append(j)
        nc = len(cseqs)
        coe = np.tile(np.arange(nc, dtype=np.int32), K)
        gof = np.array(genome_of, np.int32)
        moc = (np.repeat(np.arange(K, dtype=np.int32) * n, nc) + np.tile(gof, K)).astype(np.int32)
        cov = np.zeros(max(nc * K, 1), np.int64)
        ng = np.zeros(max(nc * K, 1), np.int32)
        sc = np.zeros(max(nc * K, 1), np.float64)
        p_coe = coe.ctypes.data; p_moc = moc.ctypes.data; p_cov = cov.ctypes.data; p_ng = ng.ctypes.data; p_sc = sc.ctypes.data
        ptrs = <const char**> malloc(sizeof(char*) * max(nc, 1))
        lens = <int64_t*> malloc(sizeof(int64_t) * max(nc, 1))
        mptrs = <const pga_training**> malloc(sizeof(void*) * max(n * K, 1))
        if ptrs == NULL or lens == NULL or mptrs == NULL:
            free(ptrs); free(lens); free(mptrs)
            raise MemoryError()
        try:
            for i in range(nc):
                ptrs[i] = PyBytes_AS_STRING((<Sequence> cseqs[i]).data)
                lens[i] = len((<Sequence> cseqs[i]).data)
            for e in range(n * K):
                mptrs[e] = <const pga_training*> <size_t> (p_out + <size_t> e * TRAINING_INFO_SIZE)
            rc = pga_set_models(ctx, mptrs, <int> (n * K))
            if rc != PGA_OK:
                _raise_for(ctx, rc, "pga_set_models")
            rc = pga_batch_create(ctx, <int32_t> nc, ptrs, lens, &up)
            if rc != PGA_OK:
                _raise_for(ctx, rc, "pga_batch_create")
        finally:
            free(ptrs); free(lens); free(mptrs)
        try:
            _attach_masks(ctx, up, cseqs, self.mask_lowercase)
            rc = pga_batch_replicate(ctx, up, <int32_t> (nc * K), <const int32_t*> p_coe, &rep)
            if rc != PGA_OK:
                _raise_for(ctx, rc, "pga_batch_replicate")
            with nogil:
                rc = pga_find_coding_bases(ctx, rep, &p, <const int32_t*> p_moc, <int64_t*> p_cov, <int32_t*> p_ng, <double*> p_sc)
            if rc != PGA_OK:
                _raise_for(ctx, rc, "pga_find_coding_bases")
        finally:
            pga_batch_free(rep)
            pga_batch_free(up)
        # 3. per genome and candidate: the sum over its contigs
        coding = np.zeros((K, n), np.int64)
        for k in range(K):
            np.add.at(coding[k], gof, cov[k * nc:(k + 1) * nc])
        raws = [[raw[(k * n + j) * TRAINING_INFO_SIZE:(k * n + j + 1) * TRAINING_INFO_SIZE].copy() for j in range(n)] for k in range(K)]
        return raws, coding

    def train_batch(self, object genomes, *, object force_nonsd=False, object start_weight=4.35, object translation_table=11,
                    object regions=None):
        """`train` on many genomes at once, on the device (`pga_train_batch`): every stage and training round runs once for the
        whole batch.  A genome is one sequence or a list / tuple of contigs (joined as `train(*contigs)` joins them); the
        keywords take a scalar or one value per genome.  Returns one `TrainingInfo` per genome, identical to
        `GeneFinder(<same options>).train(genome, ...)`; the finder's own `training_info` is left alone.  Device calls hold at most
        `coalesce_bases` bases and four translation tables; the results do not depend on that split."""
        _refuse_device_input(genomes, "train_batch")
        if self.meta:
            raise RuntimeError("cannot use training sequence in metagenomic mode")
        cdef list gl = list(genomes)
        cdef Py_ssize_t G = len(gl), g
        if G == 0:
            return []
        cdef list rl = None         # `regions`: one entry per genome, as `train` takes them
        if regions is not None:
            rl = list(regions)
            if len(rl) != G:
                raise ValueError("`regions` has %d entries for %d genomes" % (len(rl), G))
        def per_genome(v, name):
            if isinstance(v, (list, tuple, np.ndarray)):
                if len(v) != G:
                    raise ValueError("`%s` has %d values for %d genomes" % (name, len(v), G))
                return list(v)
            return [v] * G
        cdef list fns = [bool(x) for x in per_genome(force_nonsd, "force_nonsd")]
        cdef list sws = [float(x) for x in per_genome(start_weight, "start_weight")]
        cdef list tts = per_genome(translation_table, "translation_table")
        cdef list auto = []
        for g in range(G):
            if isinstance(tts[g], str) and tts[g] == "auto":
                auto.append(g)
            elif isinstance(tts[g], (str, bytes)) or tts[g] not in TRANSLATION_TABLES:
                raise ValueError("genome %d: %r is not a valid translation table index" % (g, tts[g]))
        if auto:
            # "auto": the table of `select_translation_table` with its defaults; the other genomes train as they are
            rest = [g for g in range(G) if g not in set(auto)]
            picked = self._select_tables([gl[g] for g in auto], _tables.DEFAULT_CANDIDATES, _tables.DEFAULT_MIN_GAIN,
                                         _tables.DEFAULT_MIN_DENSITY, [fns[g] for g in auto], [sws[g] for g in auto], "genome %d: ", auto,
                                         None if rl is None else [rl[g] for g in auto])
            trained = self.train_batch([gl[g] for g in rest], force_nonsd=[fns[g] for g in rest], start_weight=[sws[g] for g in rest],
                                       translation_table=[tts[g] for g in rest],
                                       regions=None if rl is None else [rl[g] for g in rest]) if rest else []
            merged = [None] * G
            for ga, sel in zip(auto, picked):
                merged[ga] = sel.training_info
            for ga, tinf in zip(rest, trained):
                merged[ga] = tinf
            return merged
        cdef list seqs = []
        for g in range(G):
            x = gl[g]
            rg = rl[g] if rl is not None else None
            seqs.append(self._training_sequence(x[0], tuple(x[1:]), "genome %d: " % g, rg) if isinstance(x, (list, tuple))
                        else self._training_sequence(x, (), "genome %d: " % g, rg))
        # the device calls: consecutive genomes under the base budget and at most four distinct tables
        cdef list calls = [], cur = []
        cdef set tables = set()
        cdef int64_t bases = 0, nb
        for g in range(G):
            nb = len((<Sequence> seqs[g]).data)
            if cur and (bases + nb > self.coalesce_bases or (tts[g] not in tables and len(tables) == 4)):
                calls.append(cur); cur = []; tables = set(); bases = 0
            cur.append(g); tables.add(tts[g]); bases += nb
        if cur:
            calls.append(cur)
        cdef list out = []
        cdef pga_params p
        cdef pga_batch* batch = NULL
        cdef const char** ptrs
        cdef int64_t* lens
        cdef int rc, n, k
        cdef size_t p_tt, p_sw, p_fn, p_out, p_st
        cdef _FinderSlot slot
        cdef pga_ctx* ctx
        p.closed = self.closed; p.min_gene = self.min_gene; p.min_edge_gene = self.min_edge_gene
        p.max_overlap = self.max_overlap; p.meta = 0; p.want_nodes = 0
        p.mask = self.mask; p.min_mask = self.min_mask
        with self._cv:
            while True:
                slot = self._free_slot()
                if slot is not None:
                    break
                self._cv.wait()
            slot.busy = True
        try:
            if slot.ctx == NULL:
                rc = pga_create(self.device, &slot.ctx)
                if rc != PGA_OK:
                    slot.ctx = NULL
                    _raise_for(NULL, rc, "pga_create")
            ctx = slot.ctx
            slot.models_loaded = False            # the training loads its own partial models into the context
            for idx in calls:
                n = len(idx)
                a_tt = np.array([tts[g] for g in idx], np.int32)
                a_sw = np.array([sws[g] for g in idx], np.float64)
                a_fn = np.array([fns[g] for g in idx], np.int32)
                raw = np.zeros(n * TRAINING_INFO_SIZE, np.uint8)
                status = np.zeros(n, np.int32)
                p_tt = a_tt.ctypes.data; p_sw = a_sw.ctypes.data; p_fn = a_fn.ctypes.data; p_out = raw.ctypes.data; p_st = status.ctypes.data
                ptrs = <const char**> malloc(sizeof(char*) * n)
                lens = <int64_t*> malloc(sizeof(int64_t) * n)
                if ptrs == NULL or lens == NULL:
                    free(ptrs); free(lens)
                    raise MemoryError()
                try:
                    for k in range(n):
                        ptrs[k] = PyBytes_AS_STRING((<Sequence> seqs[idx[k]]).data)
                        lens[k] = len((<Sequence> seqs[idx[k]]).data)
                    rc = pga_batch_create(ctx, n, ptrs, lens, &batch)
                finally:
                    free(ptrs); free(lens)
                if rc != PGA_OK:
                    _raise_for(ctx, rc, "pga_batch_create")
                try:
                    _attach_masks(ctx, batch, [seqs[g] for g in idx], self.mask_lowercase)
                    with nogil:
                        rc = pga_train_batch(ctx, batch, &p, <const int32_t*> p_tt, <const double*> p_sw, <const int32_t*> p_fn, 0,
                                             <pga_training*> p_out, <int32_t*> p_st)
                finally:
                    pga_batch_free(batch)
                    batch = NULL
                if rc != PGA_OK:
                    _raise_for(ctx, rc, "pga_train_batch")
                for k in range(n):
                    if status[k] != PGA_OK:
                        raise ValueError("genome %d could not be trained: no start / stop node in the sequence" % idx[k])
                out.extend([TrainingInfo(raw=raw[k * TRAINING_INFO_SIZE:(k + 1) * TRAINING_INFO_SIZE].copy()) for k in range(n)])
        finally:
            with self._lock:
                self._release_slot(slot)
        return out

    def train(self, object sequence, *sequences, bint force_nonsd=False, double start_weight=4.35, object translation_table=11,
              object regions=None):
        """Train on the given genome, on the device, and use the result for the next `find_genes` (ref: lib.pyx:5471-5575).

        Several sequences (the contigs of one genome) are joined with `TTAATTAATTAA` linkers like in Prodigal.
        `translation_table="auto"` trains with the table `select_translation_table` chooses with its defaults (11, or 4 when it
        covers clearly more of the genome); the contigs are then also called one by one, as `find_genes` calls them.

        `regions`: masked intervals as `find_genes` takes them -- of the one sequence, or with several contigs one entry (None or
        intervals) per contig; they travel with their contig through the join."""
        import warnings
        cdef Sequence seq
        cdef pga_params p
        _refuse_device_input(sequence, "train")
        cdef pga_batch* batch = NULL
        cdef const char* ptr
        cdef int64_t length
        cdef int rc
        cdef object raw
        cdef _FinderSlot slot
        cdef pga_ctx* ctx
        if self.meta:
            raise RuntimeError("cannot use training sequence in metagenomic mode")
        if isinstance(translation_table, str):
            if translation_table != "auto":
                raise ValueError("%r is not a valid translation table index (an int, or \"auto\")" % (translation_table,))
            picked = self.select_translation_table([(sequence,) + sequences], force_nonsd=force_nonsd, start_weight=start_weight,
                                                   regions=None if regions is None else [regions])[0]
            self.training_info = picked.training_info
            return picked.training_info
        cdef int tt = translation_table       # an int as before ("auto" above)
        if tt not in TRANSLATION_TABLES:
            raise ValueError("%d is not a valid translation table index" % tt)
        seq = self._training_sequence(sequence, sequences, "", regions)
        p.closed = self.closed; p.min_gene = self.min_gene; p.min_edge_gene = self.min_edge_gene
        p.max_overlap = self.max_overlap; p.meta = 0; p.want_nodes = 0
        p.mask = self.mask; p.min_mask = self.min_mask
        raw = np.zeros(TRAINING_INFO_SIZE, np.uint8)
        cdef size_t out_ptr = raw.ctypes.data
        ptr = PyBytes_AS_STRING(seq.data)
        length = len(seq.data)
        # the training takes a context for itself, like a device call of find_genes
        with self._cv:
            while True:
                slot = self._free_slot()
                if slot is not None:
                    break
                self._cv.wait()
            slot.busy = True
        try:
            if slot.ctx == NULL:
                rc = pga_create(self.device, &slot.ctx)
                if rc != PGA_OK:
                    slot.ctx = NULL
                    _raise_for(NULL, rc, "pga_create")
            ctx = slot.ctx
            slot.models_loaded = False            # the training loads its own partial models into the context
            rc = pga_batch_create(ctx, 1, &ptr, &length, &batch)
            if rc != PGA_OK:
                _raise_for(ctx, rc, "pga_batch_create")
            try:
                _attach_masks(ctx, batch, [seq], self.mask_lowercase)
                with nogil:
                    rc = pga_train(ctx, batch, &p, tt, start_weight, force_nonsd, 0, <pga_training*> out_ptr)
                if rc != PGA_OK:
                    _raise_for(ctx, rc, "pga_train")
            finally:
                pga_batch_free(batch)
            tinf = TrainingInfo(raw=raw)
            self.training_info = tinf
        finally:
            with self._lock:
                self._release_slot(slot)
        return tinf


def _gene_finder_from_state(training_info, dict kw):
    return GeneFinder(training_info, **kw)


cdef object _arr(const void* ptr, ssize_t nbytes, object dtype):
    if ptr == NULL or nbytes == 0:
        return np.zeros(0, dtype=dtype)
    return np.frombuffer(PyBytes_FromStringAndSize(<const char*> ptr, nbytes), dtype=dtype)


cdef Nodes _copy_nodes(const pga_nodes* nd):
    cdef Nodes out = Nodes()
    cdef ssize_t n = nd.n
    f = out._f
    f["ndx"] = _arr(nd.ndx, 4 * n, np.int32); f["stop_val"] = _arr(nd.stop_val, 4 * n, np.int32)
    f["traceb"] = _arr(nd.traceb, 4 * n, np.int32); f["tracef"] = _arr(nd.tracef, 4 * n, np.int32)
    f["star_ptr"] = _arr(nd.star_ptr, 12 * n, np.int32).reshape(-1, 3)
    f["type"] = _arr(nd.type, n, np.uint8); f["edge"] = _arr(nd.edge, n, np.uint8); f["elim"] = _arr(nd.elim, n, np.uint8)
    f["rbs"] = _arr(nd.rbs, 2 * n, np.uint8).reshape(-1, 2)
    f["strand"] = _arr(nd.strand, n, np.int8); f["ov_mark"] = _arr(nd.ov_mark, n, np.int8)
    f["gc_cont"] = _arr(nd.gc_cont, 4 * n, np.float32)
    f["cscore"] = _arr(nd.cscore, 8 * n, np.float64); f["sscore"] = _arr(nd.sscore, 8 * n, np.float64)
    f["rscore"] = _arr(nd.rscore, 8 * n, np.float64); f["uscore"] = _arr(nd.uscore, 8 * n, np.float64)
    f["tscore"] = _arr(nd.tscore, 8 * n, np.float64); f["score"] = _arr(nd.score, 8 * n, np.float64)
    f["mot_score"] = _arr(nd.mot_score, 8 * n, np.float64); f["mot_ndx"] = _arr(nd.mot_ndx, 4 * n, np.int32)
    f["mot_len"] = _arr(nd.mot_len, n, np.uint8); f["mot_spacer"] = _arr(nd.mot_spacer, n, np.uint8)
    f["mot_spacendx"] = _arr(nd.mot_spacendx, n, np.uint8)
    return out


# The node arrays of one contig, field after field in one bytes object: what a Genes keeps until `.nodes` is asked for.
_NODE_BLOB_FIELDS = [
    ("ndx", np.int32, 1), ("stop_val", np.int32, 1), ("traceb", np.int32, 1), ("tracef", np.int32, 1), ("star_ptr", np.int32, 3),
    ("gc_cont", np.float32, 1), ("mot_ndx", np.int32, 1),
    ("cscore", np.float64, 1), ("sscore", np.float64, 1), ("rscore", np.float64, 1), ("uscore", np.float64, 1),
    ("tscore", np.float64, 1), ("score", np.float64, 1), ("mot_score", np.float64, 1),
    ("type", np.uint8, 1), ("edge", np.uint8, 1), ("elim", np.uint8, 1), ("rbs", np.uint8, 2), ("strand", np.int8, 1),
    ("ov_mark", np.int8, 1), ("mot_len", np.uint8, 1), ("mot_spacer", np.uint8, 1), ("mot_spacendx", np.uint8, 1),
]


cdef bytes _pack_nodes(const pga_nodes* nd):
    cdef ssize_t n = nd.n
    cdef const void* src[23]
    cdef ssize_t width[23]
    cdef ssize_t k, total = 0, at = 0
    src[0] = nd.ndx; src[1] = nd.stop_val; src[2] = nd.traceb; src[3] = nd.tracef; src[4] = nd.star_ptr
    src[5] = nd.gc_cont; src[6] = nd.mot_ndx
    src[7] = nd.cscore; src[8] = nd.sscore; src[9] = nd.rscore; src[10] = nd.uscore; src[11] = nd.tscore; src[12] = nd.score
    src[13] = nd.mot_score
    src[14] = nd.type; src[15] = nd.edge; src[16] = nd.elim; src[17] = nd.rbs; src[18] = nd.strand; src[19] = nd.ov_mark
    src[20] = nd.mot_len; src[21] = nd.mot_spacer; src[22] = nd.mot_spacendx
    width[0] = 4; width[1] = 4; width[2] = 4; width[3] = 4; width[4] = 12; width[5] = 4; width[6] = 4
    for k in range(7, 14):
        width[k] = 8
    for k in range(14, 23):
        width[k] = 1
    width[17] = 2
    for k in range(23):
        total += width[k] * n
    cdef bytes blob = PyBytes_FromStringAndSize(NULL, total)
    cdef char* dst = PyBytes_AS_STRING(blob)
    for k in range(23):
        if n > 0 and src[k] != NULL:
            memcpy(dst + at, src[k], width[k] * n)
        elif n > 0:
            memset(dst + at, 0, width[k] * n)
        at += width[k] * n
    return blob


cdef Nodes _nodes_from_blob(bytes blob, ssize_t n):
    cdef Nodes out = Nodes()
    cdef ssize_t at = 0
    f = out._f
    for name, dt, mult in _NODE_BLOB_FIELDS:
        a = np.frombuffer(blob, dtype=dt, count=n * mult, offset=at)
        f[name] = a.reshape(-1, mult) if mult > 1 else a
        at += a.nbytes
    return out


def _seq_pointers(list seqs):
    """The C-ABI's argument arrays for a list of ``bytes`` contigs: (addresses as uint64, lengths as int64, total bases).  What
    `_cabi.Batch` hands to ``pga_batch_create`` -- one C loop instead of 6 000 ctypes conversions under the GIL per device call
    (4 - 7 ms of a 6 250-contig call's host time).  The caller keeps ``seqs`` alive while the addresses are in use."""
    cdef ssize_t n = len(seqs), i
    cdef int64_t total = 0
    ptrs = np.empty(max(n, 1), dtype=np.uint64)
    lens = np.empty(max(n, 1), dtype=np.int64)
    cdef unsigned long long[::1] p = ptrs
    cdef int64_t[::1] l = lens
    cdef object o
    for i in range(n):
        o = seqs[i]
        if not isinstance(o, bytes):
            raise TypeError("contigs must be bytes")
        p[i] = <unsigned long long> <size_t> PyBytes_AS_STRING(o)
        l[i] = len(<bytes> o)
        total += l[i]
    return ptrs, lens, total


def _render_gene_line(str fmt, bytes rec, TrainingInfo training_info not None, str sequence_id, ssize_t num_seq, ssize_t index,
                      bint full_id=False, bint include_translation_table=False, str version_separator="_v"):
    """One line as the host writers print it, for the device renderer's flagged lines (`_cabi.Context.render_genes`): the
    gene line of `write_gff` (fmt "gff") or the record header of `write_translations` / `write_genes` (fmt "faa" / "fna"), for
    gene `index` of its sequence whose packed record is `rec`."""
    if len(rec) != sizeof(pga_gene):
        raise ValueError("a gene record is %d bytes" % sizeof(pga_gene))
    cdef Genes owner = Genes.__new__(Genes)
    owner.training_info = training_info
    cdef Gene gene = Gene.__new__(Gene)
    gene.owner = owner
    gene.g = (<const pga_gene*> PyBytes_AS_STRING(rec))[0]
    ident = gene._gene_data(sequence_id if full_id else num_seq, index)
    if fmt != "gff":
        return ">%s_%d # %d # %d # %d # %s\n" % (sequence_id, index + 1, gene.g.begin, gene.g.end, gene.g.strand, ident)
    line = "%s\tpyrodigal_amd%s%s\tCDS\t%d\t%d\t%.1f\t%s\t0\t%s;" % (
        sequence_id, version_separator, _VERSION, gene.g.begin, gene.g.end, gene.g.sscore + gene.g.cscore,
        "+" if gene.g.strand > 0 else "-", ident)
    if include_translation_table:
        line += "transl_table=%d;" % training_info.translation_table
    return line + gene._score_data() + "\n"


def _genes_from_records(object sequence, bytes recs, TrainingInfo training_info, ssize_t num_seq, bint meta=False,
                        object metagenomic_bin=None, bint circular=False, object cut=None):
    """A `Genes` over packed gene records of one sequence (a slice of a `pga_result`'s records, as bytes), for the host writers:
    what a `GeneFinder` call returns for the sequence, without node arrays."""
    if len(recs) % sizeof(pga_gene):
        raise ValueError("a gene record is %d bytes" % sizeof(pga_gene))
    cdef Genes genes = Genes.__new__(Genes)
    genes.sequence = sequence if isinstance(sequence, Sequence) else Sequence(sequence)
    genes.training_info = training_info
    genes.metagenomic_bin = metagenomic_bin
    genes.meta = meta
    genes.score = 0.0
    genes._num_seq = num_seq
    genes.circular = circular
    genes.cut = cut
    genes._genes = None
    genes._recs = recs
    genes._n = len(recs) // sizeof(pga_gene)
    genes._node_blob = None; genes._node_n = 0; genes._nodes = None
    genes._prot = None; genes._prot_off = None; genes._prot_tt = 0
    return genes


def circular_cut(ssize_t length, object begins, object ends):
    """Where a circular sequence of `length` bases whose linear call found genes `begins[k] .. ends[k]` (1-based, inclusive) is cut
    open for its second pass (`pga_circular_cut`): the middle of the widest stretch no gene covers, in the middle half of the
    record when there is one there."""
    b = np.ascontiguousarray(begins, np.int32).reshape(-1)
    e = np.ascontiguousarray(ends, np.int32).reshape(-1)
    if b.size != e.size:
        raise ValueError("%d begins for %d ends" % (b.size, e.size))
    if length < 0 or length > 0x7fffffff:
        raise ValueError("`length` must be a 32-bit length")
    cdef size_t pb = b.ctypes.data, pe = e.ctypes.data
    cdef int rc = pga_circular_cut(<int32_t> length, <int32_t> b.size, <const int32_t*> pb, <const int32_t*> pe)
    if rc < 0:
        raise ValueError("pga_circular_cut: bad arguments")
    return rc
