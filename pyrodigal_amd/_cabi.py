"""ctypes binding of ``libpyrodigal_amd.so`` (the C-ABI declared in ``include/pyrodigal_amd.h``).

There is no CPU implementation behind this module: if the shared library is missing, or no
gfx950 device is visible, calls raise instead of silently computing elsewhere.
"""
import ctypes
import fractions
import functools
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpyrodigal_amd.so")

PGA_OK, PGA_EINVAL, PGA_ENOMEM, PGA_EDEVICE, PGA_ENODEVICE = 0, -1, -2, -3, -4
TRAINING_SIZE = 558392

EXPORTS = [
    "pga_create", "pga_destroy", "pga_last_error", "pga_device_info", "pga_set_models",
    "pga_score_connections", "pga_score_connections_training", "pga_find_genes_batch", "pga_result_free",
    "pga_batch_create", "pga_batch_free", "pga_find_genes", "pga_nodes_stage",
    "pga_fasta_open", "pga_fasta_next", "pga_fasta_error", "pga_fasta_close", "pga_train", "pga_dp_stats", "pga_dp_timings", "pga_extract_stats", "pga_dp_plan_summary", "pga_dp_start_order", "pga_cs_task_summary",
    "pga_fasta_next_packed", "pga_batch_create_packed", "pga_translate_genes", "pga_fasta_open_callback", "pga_fasta_release_spare", "pga_dp_xcd_order", "pga_release_cached",
    "pga_find_genes_models", "pga_train_batch", "pga_render_genes", "pga_render_free",
    "pga_batch_replicate", "pga_find_coding_bases",
    "pga_batch_set_regions", "pga_batch_set_mask_case",
    "pga_batch_set_circular", "pga_circular_cuts", "pga_circular_cut",
    "pga_batch_set_sets", "pga_set_choice", "pga_model_scores", "pga_render_seqnums",
    "pga_batch_terminal_repeats", "pga_batch_trim_terminal_repeats", "pga_terminal_repeat_chunk",
    "pga_debug_poison",
    "pga_batch_create_device", "pga_batch_read",
    "pga_translate_genes_tokens", "pga_label_bases", "pga_gene_windows",
    "pga_start_plan_create", "pga_start_plan_write", "pga_start_plan_nodes", "pga_start_plan_free", "pga_device_read",
    "pga_count_kmers", "pga_kmer_counts_chunk",
    "pga_group_proteins", "pga_protein_groups_stats",
    "pga_sketch_proteins", "pga_sketch_pairs", "pga_sketch_passes",
    "pga_cluster_sketches", "pga_cluster_stats",
    "pga_align_pairs", "pga_align_stats", "pga_cluster_edges",
]
STAGE_EXTRACT, STAGE_SCORE, STAGE_OVERLAP, STAGE_SEQUENCE = 1, 2, 3, 4


class Params(ctypes.Structure):
    _fields_ = [("closed", ctypes.c_int32), ("min_gene", ctypes.c_int32), ("min_edge_gene", ctypes.c_int32),
                ("max_overlap", ctypes.c_int32), ("meta", ctypes.c_int32), ("want_nodes", ctypes.c_int32),
                ("mask", ctypes.c_int32), ("min_mask", ctypes.c_int32)]


class Gene(ctypes.Structure):
    _fields_ = [("contig", ctypes.c_int32), ("begin", ctypes.c_int32), ("end", ctypes.c_int32),
                ("start_ndx", ctypes.c_int32), ("stop_ndx", ctypes.c_int32), ("strand", ctypes.c_int8),
                ("partial_begin", ctypes.c_uint8), ("partial_end", ctypes.c_uint8), ("start_type", ctypes.c_uint8),
                ("rbs", ctypes.c_uint8 * 2), ("mot_len", ctypes.c_uint8), ("mot_spacer", ctypes.c_uint8),
                ("mot_ndx", ctypes.c_int32), ("gc_cont", ctypes.c_float),
                ("cscore", ctypes.c_double), ("sscore", ctypes.c_double), ("rscore", ctypes.c_double),
                ("uscore", ctypes.c_double), ("tscore", ctypes.c_double), ("mot_score", ctypes.c_double)]


_P = ctypes.POINTER


class Nodes(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32),
                ("ndx", _P(ctypes.c_int32)), ("stop_val", _P(ctypes.c_int32)), ("traceb", _P(ctypes.c_int32)),
                ("tracef", _P(ctypes.c_int32)), ("star_ptr", _P(ctypes.c_int32)),
                ("type", _P(ctypes.c_uint8)), ("edge", _P(ctypes.c_uint8)), ("elim", _P(ctypes.c_uint8)),
                ("rbs", _P(ctypes.c_uint8)), ("strand", _P(ctypes.c_int8)), ("ov_mark", _P(ctypes.c_int8)),
                ("gc_cont", _P(ctypes.c_float)),
                ("cscore", _P(ctypes.c_double)), ("sscore", _P(ctypes.c_double)), ("rscore", _P(ctypes.c_double)),
                ("uscore", _P(ctypes.c_double)), ("tscore", _P(ctypes.c_double)), ("score", _P(ctypes.c_double)),
                ("mot_score", _P(ctypes.c_double)), ("mot_ndx", _P(ctypes.c_int32)),
                ("mot_len", _P(ctypes.c_uint8)), ("mot_spacer", _P(ctypes.c_uint8)), ("mot_spacendx", _P(ctypes.c_uint8))]


class ContigResult(ctypes.Structure):
    _fields_ = [("model", ctypes.c_int32), ("n_nodes", ctypes.c_int32), ("gene_begin", ctypes.c_int64),
                ("n_genes", ctypes.c_int32), ("n_unknown", ctypes.c_int32), ("gc", ctypes.c_double),
                ("score", ctypes.c_double)]


class Result(ctypes.Structure):
    _fields_ = [("n_contigs", ctypes.c_int32), ("n_genes", ctypes.c_int64), ("contigs", _P(ContigResult)),
                ("genes", _P(Gene)), ("nodes", _P(Nodes)), ("t_total_ms", ctypes.c_double),
                ("t_dp_ms", ctypes.c_double), ("node_passes", ctypes.c_int64), ("n_chains", ctypes.c_int32),
                ("_pad", ctypes.c_int32), ("mask_off", _P(ctypes.c_int32)), ("masks", _P(ctypes.c_int32))]


class RenderOpts(ctypes.Structure):
    _fields_ = [("formats", ctypes.c_int32), ("meta", ctypes.c_int32), ("first_seqnum", ctypes.c_int64),
                ("source", ctypes.c_char_p), ("version", ctypes.c_char_p), ("model_desc", _P(ctypes.c_char_p)),
                ("gff_header", ctypes.c_int32), ("gff_include_translation_table", ctypes.c_int32), ("gff_full_id", ctypes.c_int32),
                ("faa_width", ctypes.c_int32), ("faa_translation_table", ctypes.c_int32), ("faa_include_stop", ctypes.c_int32),
                ("faa_strict", ctypes.c_int32), ("faa_full_id", ctypes.c_int32), ("fna_width", ctypes.c_int32),
                ("fna_full_id", ctypes.c_int32), ("fallback_margin", ctypes.c_double),
                ("gbk_division", ctypes.c_char_p), ("gbk_date", ctypes.c_char_p), ("gbk_version", ctypes.c_char_p),
                ("gbk_translation_table", ctypes.c_int32), ("gbk_strict", ctypes.c_int32), ("sco_header", ctypes.c_int32),
                ("_pad1", ctypes.c_int32)]


class Text(ctypes.Structure):
    _fields_ = [("data", ctypes.c_void_p), ("size", ctypes.c_int64), ("contig_off", _P(ctypes.c_int64)),
                ("n_fallback", ctypes.c_int64), ("fallback", _P(ctypes.c_int64))]


class RenderResult(ctypes.Structure):
    _fields_ = [("n_contigs", ctypes.c_int32), ("_pad", ctypes.c_int32), ("text", Text * 5), ("t_kernels_ms", ctypes.c_double * 5)]


class TokenOpts(ctypes.Structure):
    _fields_ = [("elem_bytes", ctypes.c_int32), ("layout", ctypes.c_int32), ("row_width", ctypes.c_int64), ("row_stride", ctypes.c_int64),
                ("include_stop", ctypes.c_int32), ("strict", ctypes.c_int32), ("unknown_residue", ctypes.c_int32), ("_pad", ctypes.c_int32),
                ("max_length", ctypes.c_int64), ("vocab", ctypes.c_int64 * 128), ("bos", ctypes.c_int64), ("eos", ctypes.c_int64),
                ("pad", ctypes.c_int64)]


class LabelOpts(ctypes.Structure):
    _fields_ = [("elem_bytes", ctypes.c_int32), ("layout", ctypes.c_int32), ("row_width", ctypes.c_int64), ("row_stride", ctypes.c_int64),
                ("class_map", ctypes.c_int64 * 256), ("pad", ctypes.c_int64)]


class WindowOpts(ctypes.Structure):
    _fields_ = [("elem_bytes", ctypes.c_int32), ("layout", ctypes.c_int32), ("row_width", ctypes.c_int64), ("row_stride", ctypes.c_int64),
                ("unit", ctypes.c_int32), ("from_anchor", ctypes.c_int32), ("to_anchor", ctypes.c_int32), ("_pad", ctypes.c_int32),
                ("from_delta", ctypes.c_int64), ("to_delta", ctypes.c_int64), ("max_length", ctypes.c_int64),
                ("ids", ctypes.c_int64 * 66), ("bos", ctypes.c_int64), ("eos", ctypes.c_int64), ("pad", ctypes.c_int64)]


class CountOpts(ctypes.Structure):
    _fields_ = [("rows", ctypes.c_int32), ("k", ctypes.c_int32), ("step", ctypes.c_int32), ("n_bins", ctypes.c_int32),
                ("row_stride", ctypes.c_int64), ("bin_of_code", ctypes.c_void_p)]


class GroupOpts(ctypes.Structure):
    _fields_ = [("unit", ctypes.c_int32), ("include_stop", ctypes.c_int32), ("strict", ctypes.c_int32), ("unknown_residue", ctypes.c_int32)]


class SketchOpts(ctypes.Structure):
    _fields_ = [("unit", ctypes.c_int32), ("k", ctypes.c_int32), ("size", ctypes.c_int32), ("seed", ctypes.c_uint32),
                ("include_stop", ctypes.c_int32), ("strict", ctypes.c_int32), ("unknown_residue", ctypes.c_int32), ("_pad", ctypes.c_int32),
                ("classes", ctypes.c_uint8 * 128)]


class ClusterOpts(ctypes.Structure):
    _fields_ = [("size", ctypes.c_int32), ("probes", ctypes.c_int32), ("num", ctypes.c_int32), ("den", ctypes.c_int32),
                ("min_union", ctypes.c_int32), ("_pad", ctypes.c_int32)]


class AlignOpts(ctypes.Structure):
    _fields_ = [("elem_bytes", ctypes.c_int32), ("max_distance", ctypes.c_int32), ("num", ctypes.c_int32), ("den", ctypes.c_int32)]


class StartOpts(ctypes.Structure):
    _fields_ = [("index_bytes", ctypes.c_int32), ("score_bytes", ctypes.c_int32), ("layout", ctypes.c_int32), ("n_fields", ctypes.c_int32),
                ("row_width", ctypes.c_int64), ("row_stride", ctypes.c_int64), ("fields", ctypes.c_int32 * 7), ("_pad", ctypes.c_int32),
                ("index_pad", ctypes.c_int64), ("score_pad", ctypes.c_double)]


TOKENS_RAGGED, TOKENS_PADDED = 0, 1                         # pga_token_opts.layout
WINDOW_BASES, WINDOW_CODONS = 0, 1                          # pga_window_opts.unit
WINDOW_START, WINDOW_END = 0, 1                             # pga_window_opts.from_anchor / to_anchor
COUNT_CONTIG, COUNT_GENE, COUNT_CONTIG_GENES = 0, 1, 2      # pga_count_opts.rows
GROUP_PROTEIN, GROUP_GENE = 0, 1                            # pga_group_opts.unit
SKETCH_PROTEIN, SKETCH_GENE = 0, 1                          # pga_sketch_opts.unit
TOKEN_NONE = -(1 << 63)                                     # pga_token_opts.bos / eos: no such token
RENDER_FORMATS = ("gff", "faa", "fna", "gbk", "scores")     # PGA_RENDER_* bit order
NODES_DEVICE = 2                                            # pga_params.want_nodes: keep the node arrays on the device
GENE_DTYPE = np.dtype(Gene)
CONTIG_DTYPE = np.dtype(ContigResult)

_lib = None
FASTA_READ_FN = ctypes.CFUNCTYPE(ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64)


def load():
    """Load the C-ABI library; raises ``RuntimeError`` when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950); pyrodigal_amd has no CPU fallback")
    L = ctypes.CDLL(LIB_PATH)
    vp, i32, i64, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    L.pga_create.restype = ctypes.c_int; L.pga_create.argtypes = [ctypes.c_int, _P(vp)]
    L.pga_destroy.restype = None; L.pga_destroy.argtypes = [vp]
    L.pga_last_error.restype = ctypes.c_char_p; L.pga_last_error.argtypes = [vp]
    L.pga_dp_stats.restype = ctypes.c_int; L.pga_dp_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_int32)]
    L.pga_dp_timings.restype = ctypes.c_int; L.pga_dp_timings.argtypes = [vp, ctypes.POINTER(ctypes.c_double)]
    L.pga_extract_stats.restype = ctypes.c_int; L.pga_extract_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_int32)]
    L.pga_dp_plan_summary.restype = ctypes.c_int
    L.pga_dp_plan_summary.argtypes = [ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)]
    L.pga_device_info.restype = ctypes.c_int
    L.pga_device_info.argtypes = [vp, ctypes.c_char_p, ctypes.c_int, _P(ctypes.c_int), _P(i64)]
    L.pga_set_models.restype = ctypes.c_int; L.pga_set_models.argtypes = [vp, _P(vp), ctypes.c_int]
    L.pga_score_connections.restype = ctypes.c_int
    L.pga_score_connections.argtypes = [vp, i32] + [vp] * 9 + [f64, ctypes.c_int, vp, vp, vp, _P(i32), _P(f64)]
    L.pga_score_connections_training.restype = ctypes.c_int
    L.pga_score_connections_training.argtypes = [vp, i32] + [vp] * 7 + [f64, vp, vp, vp, _P(i32), _P(f64)]
    L.pga_find_genes_batch.restype = ctypes.c_int
    L.pga_find_genes_batch.argtypes = [vp, i32, _P(ctypes.c_char_p), _P(i64), _P(Params), _P(_P(Result))]
    L.pga_result_free.restype = None; L.pga_result_free.argtypes = [_P(Result)]
    L.pga_batch_create.restype = ctypes.c_int
    L.pga_batch_create.argtypes = [vp, i32, _P(ctypes.c_char_p), _P(i64), _P(vp)]
    L.pga_batch_free.restype = None; L.pga_batch_free.argtypes = [vp]
    L.pga_find_genes.restype = ctypes.c_int; L.pga_find_genes.argtypes = [vp, vp, _P(Params), _P(_P(Result))]
    L.pga_find_genes_models.restype = ctypes.c_int; L.pga_find_genes_models.argtypes = [vp, vp, _P(Params), vp, _P(_P(Result))]
    L.pga_batch_replicate.restype = ctypes.c_int; L.pga_batch_replicate.argtypes = [vp, vp, i32, vp, _P(vp)]
    L.pga_batch_set_regions.restype = ctypes.c_int; L.pga_batch_set_regions.argtypes = [vp, vp, vp]
    L.pga_batch_set_mask_case.restype = ctypes.c_int; L.pga_batch_set_mask_case.argtypes = [vp, ctypes.c_int]
    L.pga_batch_set_circular.restype = ctypes.c_int; L.pga_batch_set_circular.argtypes = [vp, vp]
    L.pga_circular_cuts.restype = ctypes.c_int; L.pga_circular_cuts.argtypes = [vp, i32, vp]
    L.pga_circular_cut.restype = ctypes.c_int; L.pga_circular_cut.argtypes = [i32, i32, vp, vp]
    L.pga_batch_set_sets.restype = ctypes.c_int; L.pga_batch_set_sets.argtypes = [vp, vp]
    L.pga_batch_terminal_repeats.restype = ctypes.c_int; L.pga_batch_terminal_repeats.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp]
    L.pga_batch_trim_terminal_repeats.restype = ctypes.c_int; L.pga_batch_trim_terminal_repeats.argtypes = [vp, vp, vp, _P(vp)]
    L.pga_terminal_repeat_chunk.restype = ctypes.c_int; L.pga_terminal_repeat_chunk.argtypes = []
    L.pga_set_choice.restype = ctypes.c_int; L.pga_set_choice.argtypes = [vp, i32, vp, vp]
    L.pga_model_scores.restype = ctypes.c_int; L.pga_model_scores.argtypes = [vp, i32, i32, vp]
    L.pga_render_seqnums.restype = ctypes.c_int; L.pga_render_seqnums.argtypes = [vp, i32, vp]
    L.pga_find_coding_bases.restype = ctypes.c_int; L.pga_find_coding_bases.argtypes = [vp, vp, _P(Params), vp, vp, vp, vp]
    L.pga_nodes_stage.restype = ctypes.c_int
    L.pga_nodes_stage.argtypes = [vp, vp, _P(Params), ctypes.c_int, ctypes.c_int, _P(_P(Result))]
    L.pga_train.restype = ctypes.c_int
    L.pga_train.argtypes = [vp, vp, _P(Params), ctypes.c_int, f64, ctypes.c_int, ctypes.c_int, vp]
    L.pga_train_batch.restype = ctypes.c_int
    L.pga_train_batch.argtypes = [vp, vp, _P(Params), vp, vp, vp, ctypes.c_int, vp, vp]
    L.pga_fasta_open.restype = ctypes.c_int; L.pga_fasta_open.argtypes = [ctypes.c_char_p, _P(vp)]
    L.pga_fasta_open_callback.restype = ctypes.c_int; L.pga_fasta_open_callback.argtypes = [FASTA_READ_FN, vp, _P(vp)]
    L.pga_fasta_next.restype = ctypes.c_int
    L.pga_fasta_next.argtypes = [vp, i64, i32, _P(i32), _P(_P(ctypes.c_char_p)), _P(_P(vp)), _P(_P(i64))]
    L.pga_fasta_next_packed.restype = ctypes.c_int
    L.pga_fasta_next_packed.argtypes = [vp, i64, i32, i32, _P(i32), _P(_P(ctypes.c_char_p)), _P(vp), _P(_P(i64)), _P(_P(i64))]
    L.pga_batch_create_packed.restype = ctypes.c_int
    L.pga_batch_create_packed.argtypes = [vp, i32, vp, _P(i64), _P(i64), _P(vp)]
    L.pga_batch_create_device.restype = ctypes.c_int
    L.pga_batch_create_device.argtypes = [vp, i32, vp, i64, i32, vp, vp, vp, i32, vp, _P(vp)]
    L.pga_batch_read.restype = ctypes.c_int; L.pga_batch_read.argtypes = [vp, vp, i32, vp]
    L.pga_translate_genes.restype = ctypes.c_int
    L.pga_translate_genes.argtypes = [vp, vp, i64, vp, vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp]
    L.pga_translate_genes_tokens.restype = ctypes.c_int
    L.pga_translate_genes_tokens.argtypes = [vp, vp, i64, vp, vp, _P(TokenOpts), vp, i64, vp, vp]
    L.pga_label_bases.restype = ctypes.c_int
    L.pga_label_bases.argtypes = [vp, vp, i64, vp, _P(LabelOpts), vp, i64, vp, vp]
    L.pga_gene_windows.restype = ctypes.c_int
    L.pga_gene_windows.argtypes = [vp, vp, i64, vp, _P(WindowOpts), vp, i64, vp, vp]
    L.pga_count_kmers.restype = ctypes.c_int
    L.pga_count_kmers.argtypes = [vp, vp, i64, vp, _P(CountOpts), vp, i64, vp, vp]
    L.pga_kmer_counts_chunk.restype = ctypes.c_int; L.pga_kmer_counts_chunk.argtypes = []
    L.pga_group_proteins.restype = ctypes.c_int
    L.pga_group_proteins.argtypes = [vp, vp, i64, vp, vp, _P(GroupOpts), vp, vp, vp, vp, i64, vp, _P(i64)]
    L.pga_protein_groups_stats.restype = ctypes.c_int; L.pga_protein_groups_stats.argtypes = [vp, _P(i64)]
    L.pga_sketch_proteins.restype = ctypes.c_int
    L.pga_sketch_proteins.argtypes = [vp, vp, i64, vp, vp, _P(SketchOpts), vp, vp, vp, vp]
    L.pga_sketch_pairs.restype = ctypes.c_int
    L.pga_sketch_pairs.argtypes = [vp, vp, vp, i64, ctypes.c_int32, vp, i64, vp, vp, vp]
    L.pga_sketch_passes.restype = ctypes.c_int; L.pga_sketch_passes.argtypes = [vp, _P(i64)]
    L.pga_cluster_sketches.restype = ctypes.c_int
    L.pga_cluster_sketches.argtypes = [vp, vp, vp, vp, i64, _P(ClusterOpts), vp, vp, vp, i64, vp, vp, vp, i64, vp, _P(i64), _P(i64)]
    L.pga_cluster_stats.restype = ctypes.c_int; L.pga_cluster_stats.argtypes = [vp, _P(i64)]
    L.pga_align_pairs.restype = ctypes.c_int
    L.pga_align_pairs.argtypes = [vp, vp, i64, vp, vp, i64, vp, i64, _P(AlignOpts), vp, vp, vp]
    L.pga_align_stats.restype = ctypes.c_int; L.pga_align_stats.argtypes = [vp, _P(i64)]
    L.pga_cluster_edges.restype = ctypes.c_int
    L.pga_cluster_edges.argtypes = [vp, vp, vp, i64, i64, vp, vp, vp, vp, i64, vp, _P(i64), _P(i64)]
    L.pga_start_plan_create.restype = ctypes.c_int
    L.pga_start_plan_create.argtypes = [vp, vp, i64, vp, _P(vp), vp, vp]
    L.pga_start_plan_write.restype = ctypes.c_int
    L.pga_start_plan_write.argtypes = [vp, vp, _P(StartOpts), vp, vp, vp, i64, i64, i64, vp]
    L.pga_start_plan_nodes.restype = ctypes.c_int
    L.pga_start_plan_nodes.argtypes = [vp, vp, vp, i64]
    L.pga_start_plan_free.restype = None; L.pga_start_plan_free.argtypes = [vp, vp]
    L.pga_device_read.restype = ctypes.c_int
    L.pga_device_read.argtypes = [vp, vp, i64, vp, vp]
    L.pga_render_genes.restype = ctypes.c_int
    L.pga_render_genes.argtypes = [vp, vp, vp, i64, vp, vp, vp, vp, _P(RenderOpts), _P(_P(RenderResult))]
    L.pga_render_free.restype = None; L.pga_render_free.argtypes = [_P(RenderResult)]
    L.pga_fasta_error.restype = ctypes.c_char_p; L.pga_fasta_error.argtypes = [vp]
    L.pga_fasta_close.restype = None; L.pga_fasta_close.argtypes = [vp]
    L.pga_fasta_release_spare.restype = None; L.pga_fasta_release_spare.argtypes = []
    L.pga_release_cached.restype = None; L.pga_release_cached.argtypes = []
    L.pga_debug_poison.restype = ctypes.c_int; L.pga_debug_poison.argtypes = [vp, ctypes.c_int, _P(i64)]
    _lib = L
    return L


def dp_start_order(nodes_per_chain):
    """The order in which the wave-batch connection scorer starts the chains of a launch (host arithmetic, no device needed)."""
    L = load()
    n = len(nodes_per_chain)
    arr = (ctypes.c_int32 * max(n, 1))(*[int(x) for x in nodes_per_chain])
    out = (ctypes.c_int32 * max(n, 1))()
    L.pga_dp_start_order.restype = ctypes.c_int
    rc = L.pga_dp_start_order(ctypes.c_int32(n), arr, out)
    if rc != PGA_OK:
        raise ValueError("pga_dp_start_order failed (code %d)" % rc)
    return list(out[:n])


def dp_xcd_order(nodes_per_chain, key_of_chain, order=None):
    """The start order dealt to the eight XCDs (host arithmetic, no device needed): entry 8 k + x is the k-th chain of XCD x, -1 a filler."""
    L = load()
    n = len(nodes_per_chain)
    order = dp_start_order(nodes_per_chain) if order is None else list(order)
    nk = (max(key_of_chain) + 1) if n else 0
    i32 = ctypes.c_int32
    out = (i32 * max(8 * n, 1))()
    L.pga_dp_xcd_order.restype = ctypes.c_int64
    L.pga_dp_xcd_order.argtypes = [i32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, i32, ctypes.c_void_p, ctypes.c_int64]
    got = L.pga_dp_xcd_order(n, (i32 * max(n, 1))(*order), (i32 * max(n, 1))(*[int(x) for x in nodes_per_chain]),
                             (i32 * max(n, 1))(*[int(x) for x in key_of_chain]), nk, out, 8 * n)
    if got < 0:
        raise ValueError("pga_dp_xcd_order failed (code %d)" % -got)
    return list(out[:got])


def cs_task_summary(nodes_per_contig, first_column, models_per_contig, task_nodes=4096):
    """How the coding-score walks of one translation-table group are cut into tasks (host arithmetic, no device needed)."""
    L = load()
    n = len(nodes_per_contig)
    mk = lambda xs: (ctypes.c_int32 * max(n, 1))(*[int(x) for x in xs])
    out = (ctypes.c_int64 * 5)()
    L.pga_cs_task_summary.restype = ctypes.c_int
    rc = L.pga_cs_task_summary(ctypes.c_int32(n), mk(nodes_per_contig), mk(first_column), mk(models_per_contig), ctypes.c_int32(task_nodes), out)
    if rc != PGA_OK:
        raise ValueError("pga_cs_task_summary: the LDS form does not apply (code %d)" % rc)
    return {"tasks": out[0], "entries": out[1], "largest_task": out[2], "nodes": out[3], "high_columns_first": bool(out[4])}


def dp_plan_summary(nodes_per_chain):
    """How a connection-scoring launch over chains of these node counts would be cut (host arithmetic, no device needed)."""
    L = load()
    n = len(nodes_per_chain)
    arr = (ctypes.c_int32 * max(n, 1))(*[int(x) for x in nodes_per_chain])
    out = (ctypes.c_int64 * 4)()
    rc = L.pga_dp_plan_summary(n, arr, out)
    if rc != PGA_OK:
        raise ValueError("pga_dp_plan_summary failed (code %d)" % rc)
    return {"chains": out[0], "segments": out[1], "max_sub_chain": out[2], "scratch": out[3]}


class PgaError(RuntimeError):
    pass


def _raise(L, ctx, code, what):
    msg = L.pga_last_error(ctx).decode("utf-8", "replace") if ctx else ""
    if code == PGA_EINVAL:
        raise ValueError(f"{what}: {msg}")
    if code == PGA_ENOMEM:
        raise MemoryError(f"{what}: {msg}")
    if code == PGA_ENODEVICE:
        raise PgaError(f"{what}: no gfx950 (MI355X) device visible; pyrodigal_amd has no CPU fallback")
    raise PgaError(f"{what}: {msg} (code {code})")


class Context:
    """Owns a ``pga_ctx`` bound to one GPU."""

    def __init__(self, device=0):
        self.L = load()
        h = ctypes.c_void_p()
        rc = self.L.pga_create(int(device), ctypes.byref(h))
        if rc != PGA_OK:
            _raise(self.L, None, rc, "pga_create")
        self.h = h
        self.device = int(device)
        self._models = []

    def close(self):
        if getattr(self, "h", None):
            self.L.pga_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def device_info(self):
        name = ctypes.create_string_buffer(256)
        cus, mem = ctypes.c_int(), ctypes.c_int64()
        rc = self.L.pga_device_info(self.h, name, 256, ctypes.byref(cus), ctypes.byref(mem))
        if rc != PGA_OK:
            _raise(self.L, self.h, rc, "pga_device_info")
        return {"name": name.value.decode(), "cus": cus.value, "hbm_bytes": mem.value}

    def dp_stats(self):
        """How the last connection scoring ran: segmented chains, segments, nodes rejected by each verification round,
        chains walked serially in the end."""
        out = (ctypes.c_int32 * 8)()
        rc = self.L.pga_dp_stats(self.h, out)
        if rc != PGA_OK:
            _raise(self.L, self.h, rc, "pga_dp_stats")
        return {"chains": out[0], "segments": out[1], "rejected": [out[2], out[3], out[4]], "serial": out[5],
                "sched": out[6], "sched_missed": out[7]}

    def dp_timings(self):
        """Device milliseconds of the last find_genes call's connection scoring by part: the scoring launch(es), the topology kernels,
        the step-schedule kernels (HIP events on the context's stream)."""
        out = (ctypes.c_double * 4)()
        rc = self.L.pga_dp_timings(self.h, out)
        if rc != PGA_OK:
            _raise(self.L, self.h, rc, "pga_dp_timings")
        return {"dp_ms": out[0], "topo_ms": out[1], "sched_ms": out[2]}

    def extract_stats(self):
        """How the last node extraction ran: passes (2: a tile overflowed the half-density staging, or the pool of stop values of its
        workgroup, and the batch was extracted again)."""
        out = (ctypes.c_int32 * 2)()
        rc = self.L.pga_extract_stats(self.h, out)
        if rc != PGA_OK:
            _raise(self.L, self.h, rc, "pga_extract_stats")
        return {"passes": out[0]}

    def debug_poison(self, byte):
        """Test support (``pga_debug_poison``): fill every floating-point workspace buffer of the context, and every block such a
        buffer acquires from now on, with ``byte`` (0 .. 255; -1 or None: off).  Returns ``(buffers, bytes)`` filled by this call."""
        out = (ctypes.c_int64 * 2)()
        rc = self.L.pga_debug_poison(self.h, -1 if byte is None else int(byte), out)
        if rc != PGA_OK:
            _raise(self.L, self.h, rc, "pga_debug_poison")
        return int(out[0]), int(out[1])

    @staticmethod
    def dp_kernel_name():
        """The connection-scoring kernel a launch with many (>= 2048) chains runs (dp.hip, pga_launch_dp)."""
        return {"tree1": "k_dp_tree", "scan": "k_dp_chain"}.get(os.environ.get("PGA_DP_KERNEL", ""), "k_dp_wave")

    def set_models(self, blobs):
        """``blobs``: iterable of 558 392-byte ``struct _training`` buffers (bytes / uint8 arrays)."""
        arrs = []
        for b in blobs:
            a = np.frombuffer(bytes(b), dtype=np.uint8).copy() if not isinstance(b, np.ndarray) else np.ascontiguousarray(b, np.uint8)
            if a.size != TRAINING_SIZE:
                raise ValueError(f"training info must be {TRAINING_SIZE} bytes, got {a.size}")
            arrs.append(a)
        ptrs = (ctypes.c_void_p * max(1, len(arrs)))(*[a.ctypes.data for a in arrs])
        rc = self.L.pga_set_models(self.h, ptrs, len(arrs))
        if rc != PGA_OK:
            _raise(self.L, self.h, rc, "pga_set_models")
        self._models = arrs

    def score_connections(self, ndx, stop_val, type_, strand, cscore, sscore, rscore, uscore, star_ptr, st_wt, final=True):
        """Whole-array ``ConnectionScorer.index`` + ``score_connections``. Returns (score, traceb, ov_mark, max_index, kernel_ms)."""
        n = len(ndx)
        c = lambda a, t: np.ascontiguousarray(a, dtype=t)
        ndx, stop_val = c(ndx, np.int32), c(stop_val, np.int32)
        type_, strand = c(type_, np.uint8), c(strand, np.int8)
        cscore, sscore, rscore, uscore = (c(x, np.float64) for x in (cscore, sscore, rscore, uscore))
        star_ptr = c(star_ptr, np.int32).reshape(-1)
        score = np.zeros(n, np.float64); traceb = np.zeros(n, np.int32); ov = np.zeros(n, np.int8)
        mi, ms = ctypes.c_int32(-1), ctypes.c_double(0)
        p = lambda a: a.ctypes.data
        rc = self.L.pga_score_connections(self.h, n, p(ndx), p(stop_val), p(type_), p(strand), p(cscore), p(sscore),
                                          p(rscore), p(uscore), p(star_ptr), float(st_wt), int(final),
                                          p(score), p(traceb), p(ov), ctypes.byref(mi), ctypes.byref(ms))
        if rc != PGA_OK:
            _raise(self.L, self.h, rc, "pga_score_connections")
        return score, traceb, ov, mi.value, ms.value

    def score_connections_training(self, ndx, stop_val, type_, strand, gc_score, bias, star_ptr, st_wt):
        """The training pass (``final=False``) of the same scorer, from the nodes' frame-bias scores."""
        n = len(ndx)
        c = lambda a, t: np.ascontiguousarray(a, dtype=t)
        ndx, stop_val = c(ndx, np.int32), c(stop_val, np.int32)
        type_, strand = c(type_, np.uint8), c(strand, np.int8)
        gc_score, bias = c(gc_score, np.float64).reshape(-1), c(bias, np.float64)
        star_ptr = c(star_ptr, np.int32).reshape(-1)
        score = np.zeros(n, np.float64); traceb = np.zeros(n, np.int32); ov = np.zeros(n, np.int8)
        mi, ms = ctypes.c_int32(-1), ctypes.c_double(0)
        p = lambda a: a.ctypes.data
        rc = self.L.pga_score_connections_training(self.h, n, p(ndx), p(stop_val), p(type_), p(strand), p(gc_score), p(bias),
                                                   p(star_ptr), float(st_wt), p(score), p(traceb), p(ov), ctypes.byref(mi), ctypes.byref(ms))
        if rc != PGA_OK:
            _raise(self.L, self.h, rc, "pga_score_connections_training")
        return score, traceb, ov, mi.value, ms.value


_NODE_FIELDS = [
    ("ndx", np.int32, 1), ("stop_val", np.int32, 1), ("traceb", np.int32, 1), ("tracef", np.int32, 1),
    ("star_ptr", np.int32, 3), ("type", np.uint8, 1), ("edge", np.uint8, 1), ("elim", np.uint8, 1),
    ("rbs", np.uint8, 2), ("strand", np.int8, 1), ("ov_mark", np.int8, 1), ("gc_cont", np.float32, 1),
    ("cscore", np.float64, 1), ("sscore", np.float64, 1), ("rscore", np.float64, 1), ("uscore", np.float64, 1),
    ("tscore", np.float64, 1), ("score", np.float64, 1), ("mot_score", np.float64, 1), ("mot_ndx", np.int32, 1),
    ("mot_len", np.uint8, 1), ("mot_spacer", np.uint8, 1), ("mot_spacendx", np.uint8, 1),
]


class BatchResult:
    """Host copy of a ``pga_result``: ``contigs`` / ``genes`` structured arrays (+ per-contig node dicts)."""

    def __init__(self, contigs, genes, nodes, t_total_ms, t_dp_ms, node_passes, n_chains=0, masks=None, cuts=None):
        self.contigs, self.genes, self.nodes = contigs, genes, nodes
        self.cuts = cuts            # int32 per contig: where a circular contig was cut open (-1: linear), or None when the batch has no flag
        self.masks = masks          # per contig an (k, 2) array of [begin, end) intervals, or None when masking is off
        self.t_total_ms, self.t_dp_ms, self.node_passes, self.n_chains = t_total_ms, t_dp_ms, node_passes, n_chains
        # contig sets (Batch.set_sets), None when the batch carried no labels: per contig the model chosen for its set (-1: none) and
        # that model's summed score (NaN: none); [contig][model] the path score a contig contributed (NaN: none)
        self.set_models = self.set_scores = self.model_scores = None
        # direct terminal repeats (find_genes_batch(..., trim_terminal_repeats=...)): int32 per contig, the letters taken off its end
        # before it was called as a circle (0: none, or not searched); None when the call did not ask
        self.terminal_repeats = None

    def genes_of(self, i):
        c = self.contigs[i]
        return self.genes[c["gene_begin"]:c["gene_begin"] + c["n_genes"]]


_SEQ_POINTERS = [False]


def _seq_pointers_fn():
    """``pyrodigal_amd.lib._seq_pointers`` (the Cython host layer's C loop over a list of bytes), or None when that module is not
    built: argument marshalling only -- the ctypes conversions below do the same, slower."""
    if _SEQ_POINTERS[0] is False:
        try:
            from . import lib as _lib
            _SEQ_POINTERS[0] = _lib._seq_pointers
        except Exception:
            _SEQ_POINTERS[0] = None
    return _SEQ_POINTERS[0]


def pack_regions(regions, n):
    """The caller's masked regions as ``pga_batch_set_regions`` takes them: ``regions`` holds one entry per sequence, ``None`` or
    an iterable of ``(begin, end)`` pairs (or objects with ``begin`` / ``end``), 0-based and half-open.  Returns ``(off, iv)``
    int32 arrays, or ``None`` when no sequence carries one."""
    if regions is None:
        return None
    regions = list(regions)
    if len(regions) != n:
        raise ValueError(f"regions has {len(regions)} entries for {n} sequences")
    off = np.zeros(n + 1, np.int32)
    flat = []
    for i, r in enumerate(regions):
        if r is not None:
            if isinstance(r, np.ndarray):
                a = np.asarray(r, dtype=np.int64).reshape(-1, 2)
            else:
                a = np.asarray([(m.begin, m.end) if hasattr(m, "begin") else tuple(m) for m in r], dtype=np.int64).reshape(-1, 2)
            if a.size and (a.min() < -(1 << 31) or a.max() >= (1 << 31)):
                raise ValueError(f"sequence {i}: an interval lies outside the 32-bit range")
            flat.append(a.astype(np.int32))
            off[i + 1] = len(a)
    np.cumsum(off, out=off)
    if off[-1] == 0:
        return None
    return off, np.ascontiguousarray(np.concatenate(flat), dtype=np.int32)


def dense_set_ids(labels, n):
    """Set labels (one per sequence: any hashable, ``None`` or -1 for a sequence on its own) as the int32 array
    ``pga_batch_set_sets`` takes: dense ids in order of first appearance, -1 for the unlabelled."""
    labels = list(labels)
    if len(labels) != n:
        raise ValueError(f"sets has {len(labels)} entries for {n} sequences")
    ids, seen = np.full(max(n, 1), -1, np.int32), {}
    for i, lab in enumerate(labels):
        if lab is None or (isinstance(lab, (int, np.integer)) and not isinstance(lab, bool) and lab == -1):
            continue
        ids[i] = seen.setdefault(lab, len(seen))
    return ids[:n] if n else ids[:0]


class Batch:
    """Contigs packed and resident in HBM (``pga_batch``)."""

    def set_masks(self, regions=None, mask_lowercase=False):
        """Attach mask sources to the batch (``pga_batch_set_regions`` / ``pga_batch_set_mask_case``): ``regions`` as
        :func:`pack_regions` takes them (``None`` detaches), ``mask_lowercase`` masks runs of lower-case letters.  Every later call
        on the batch honours them; ``ValueError`` names the sequence and the interval that does not lie inside it."""
        packed = pack_regions(regions, self.n)
        L = self.ctx.L
        if packed is None:
            rc = L.pga_batch_set_regions(self.h, None, None)
        else:
            rc = L.pga_batch_set_regions(self.h, ctypes.c_void_p(packed[0].ctypes.data), ctypes.c_void_p(packed[1].ctypes.data))
        if rc == PGA_OK:
            rc = L.pga_batch_set_mask_case(self.h, int(bool(mask_lowercase)))
        if rc != PGA_OK:
            _raise(L, self.ctx.h, rc, "pga_batch_set_regions")
        return self

    circular = None     # the flags of set_circular (uint8 per contig), or None: every contig is linear

    def set_circular(self, circular=None):
        """Mark contigs circular (``pga_batch_set_circular``): ``None`` / ``False`` (all linear), ``True`` (all circular) or one flag
        per contig.  ``find_genes`` then calls the flagged contigs across the origin and reports ``cuts``."""
        if circular is None or circular is False:
            flags = None
        elif circular is True:
            flags = np.ones(max(self.n, 1), np.uint8)
        else:
            flags = np.ascontiguousarray([1 if x else 0 for x in circular], dtype=np.uint8)
            if flags.shape != (self.n,):
                raise ValueError(f"circular has {flags.size} entries for {self.n} contigs")
            if not flags.any():
                flags = None
        rc = self.ctx.L.pga_batch_set_circular(self.h, None if flags is None else ctypes.c_void_p(flags.ctypes.data))
        if rc != PGA_OK:
            _raise(self.ctx.L, self.ctx.h, rc, "pga_batch_set_circular")
        self.circular = flags
        return self

    sets = None         # the dense ids of set_sets (int32 per contig, -1: on its own), or None: no labels

    def set_sets(self, labels=None):
        """Label contigs as members of sets that are known to be one organism (``pga_batch_set_sets``): one label per contig, any
        hashable, ``None`` (or -1) for a contig on its own; ``labels=None`` clears them.  Labels become dense ids in order of first
        appearance.  A meta-mode ``find_genes`` then chooses one model per set and reports ``set_models`` / ``set_scores`` /
        ``model_scores``."""
        ids = None if labels is None else dense_set_ids(labels, self.n)
        rc = self.ctx.L.pga_batch_set_sets(self.h, None if ids is None else ctypes.c_void_p(ids.ctypes.data))
        if rc != PGA_OK:
            _raise(self.ctx.L, self.ctx.h, rc, "pga_batch_set_sets")
        self.sets = ids
        return self

    def terminal_repeats(self, search=None, min_length=20, max_length=65536, max_base_percent=75):
        """Direct terminal repeats of the resident contigs, found on the device (``pga_batch_terminal_repeats``): ``(match, trim)``,
        int32 per contig.  ``match`` is the longest r in ``min_length .. min(max_length, L // 2)`` for which the first r bases of
        the contig are also its last r (0: none); ``trim`` is ``match``, or 0 where one base makes up more than
        ``max_base_percent`` percent of the repeat.  ``search``: one flag per contig (``None``: all); the others report 0.  The
        batch is left as it is."""
        flags = None
        if search is not None:
            flags = np.ascontiguousarray([1 if x else 0 for x in search], dtype=np.uint8)
            if flags.shape != (self.n,):
                raise ValueError(f"search has {flags.size} entries for {self.n} contigs")
        match, trim = np.zeros(max(self.n, 1), np.int32), np.zeros(max(self.n, 1), np.int32)
        rc = self.ctx.L.pga_batch_terminal_repeats(self.ctx.h, self.h, None if flags is None or not self.n else ctypes.c_void_p(flags.ctypes.data),
                                                   int(min_length), int(max_length), int(max_base_percent),
                                                   ctypes.c_void_p(match.ctypes.data), ctypes.c_void_p(trim.ctypes.data))
        if rc != PGA_OK:
            _raise(self.ctx.L, self.ctx.h, rc, "pga_batch_terminal_repeats")
        return match[:self.n], trim[:self.n]

    def trim_terminal_repeats(self, trim):
        """A new resident :class:`Batch` whose contig i has lost its last ``trim[i]`` letters and is flagged circular where
        ``trim[i] > 0`` (``pga_batch_trim_terminal_repeats``); mask sources, set labels and circular flags travel with the contigs.
        Returns ``self``, and copies nothing, when every entry is 0."""
        t = np.ascontiguousarray(trim, dtype=np.int32).reshape(-1)
        if t.shape != (self.n,):
            raise ValueError(f"trim has {t.size} entries for {self.n} contigs")
        h = ctypes.c_void_p()
        rc = self.ctx.L.pga_batch_trim_terminal_repeats(self.ctx.h, self.h, ctypes.c_void_p(t.ctypes.data) if self.n else None, ctypes.byref(h))
        if rc != PGA_OK:
            _raise(self.ctx.L, self.ctx.h, rc, "pga_batch_trim_terminal_repeats")
        if not h:
            return self
        b = Batch.__new__(Batch)
        b.ctx, b.n, b.h = self.ctx, self.n, h
        b.total = None if self.total is None else int(self.total) - int(t.sum())
        b.lengths = np.asarray(self.lengths, np.int64) - t
        flags = (t > 0).astype(np.uint8)
        if self.circular is not None:
            flags |= (self.circular[:self.n] != 0).astype(np.uint8)
        b.circular = np.ascontiguousarray(flags)
        if self.sets is not None:
            b.sets = self.sets
        return b

    def __init__(self, ctx, seqs):
        self.ctx = ctx
        self.n = len(seqs)
        fast = _seq_pointers_fn() if type(seqs) is list else None
        arrays = None
        if fast is not None:
            try:
                arrays = fast(seqs)             # every contig a bytes object: the argument arrays by one C loop
            except TypeError:
                arrays = None
        if arrays is not None:
            p_arr, l_arr, self.total = arrays
            self.lengths = np.array(l_arr[:self.n], np.int64)
            ptrs = p_arr.ctypes.data_as(ctypes.POINTER(ctypes.c_char_p))
            lens = l_arr.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
        else:
            seqs = [s.encode("ascii") if isinstance(s, str) else bytes(s) for s in seqs]
            self.total = sum(len(s) for s in seqs)
            self.lengths = np.array([len(s) for s in seqs], np.int64)
            ptrs = (ctypes.c_char_p * max(1, self.n))(*seqs)
            lens = (ctypes.c_int64 * max(1, self.n))(*[len(s) for s in seqs])
        h = ctypes.c_void_p()
        rc = ctx.L.pga_batch_create(ctx.h, self.n, ptrs, lens, ctypes.byref(h))
        del arrays
        if rc != PGA_OK:
            _raise(ctx.L, ctx.h, rc, "pga_batch_create")
        self.h = h

    def read(self, contig=None):
        """The packed letters of the resident batch as ``bytes`` (``pga_batch_read``): those of contig ``contig``, or with ``None``
        those of the whole batch, contig after contig.  One device-to-host copy.  Every way to make a batch records ``lengths``."""
        if contig is None:
            size, which = int(np.sum(self.lengths, dtype=np.int64)) if self.n else 0, -1
        else:
            which = int(contig)
            if not 0 <= which < self.n:
                raise IndexError(f"contig {which} of a batch of {self.n}")
            size = int(self.lengths[which])
        buf = ctypes.create_string_buffer(max(size, 1))
        rc = self.ctx.L.pga_batch_read(self.ctx.h, self.h, which, buf)
        if rc != PGA_OK:
            _raise(self.ctx.L, self.ctx.h, rc, "pga_batch_read")
        return buf.raw[:size]

    def close(self):
        if getattr(self, "h", None):
            self.ctx.L.pga_batch_free(self.h)
            self.h = None

    def __del__(self):
        self.close()


_DEVICE_DTYPES = {"|u1": 1, "|i1": 1, "<i4": 4, "<i8": 8}


def _host_ints(values, name):
    """Host integers of ``lengths`` / ``offsets`` as an int64 array: an object with ``tolist()`` (a tensor, an array) goes through it."""
    if hasattr(values, "tolist"):
        values = values.tolist()
    values = list(values)
    for v in values:
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"{name} must hold integers, not {type(v).__name__}")
    return np.array(values, dtype=np.int64).reshape(-1)


def normalise_alphabet(alphabet):
    """``alphabet=`` of :class:`DeviceSequences` as the table ``pga_batch_create_device`` takes: ``None``, or ``bytes`` of at most 256
    ASCII letters indexed by token id.  A ``str`` / ``bytes`` is that table; a ``{id: letter}`` dict is filled up with ``N``."""
    if alphabet is None:
        return None
    if isinstance(alphabet, dict):
        if not alphabet:
            table = b""
        else:
            for k in alphabet:
                if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
                    raise TypeError(f"alphabet ids must be integers, not {type(k).__name__}")
                if not 0 <= int(k) < 256:
                    raise ValueError(f"alphabet id {k} is outside 0 .. 255: the table has at most 256 entries")
            t = bytearray(b"N" * (max(int(k) for k in alphabet) + 1))
            for k, v in alphabet.items():
                v = v.encode("ascii", "replace") if isinstance(v, str) else (bytes([v]) if isinstance(v, (int, np.integer)) else bytes(v))
                if len(v) != 1:
                    raise ValueError(f"alphabet id {k}: {v!r} is not one letter")
                t[int(k)] = v[0]
            table = bytes(t)
    elif isinstance(alphabet, str):
        table = alphabet.encode("ascii", "replace")
    else:
        table = bytes(alphabet)
    if len(table) > 256:
        raise ValueError(f"an alphabet has at most 256 entries, not {len(table)}")
    for k, a in enumerate(table):
        if not (65 <= a <= 90 or 97 <= a <= 122):
            raise ValueError(f"alphabet entry {k} ({bytes([a])!r}) is not an ASCII letter")
    return table


class DeviceSequences:
    """Sequences that already lie in device memory, as ``pga_batch_create_device`` takes them (the rule is in ``pyrodigal_amd.h``).

    ``data``: any object with ``__cuda_array_interface__`` (a torch tensor on a ROCm device has it; a three-line wrapper around a raw
    pointer also serves), 1-D or 2-D, dtype ``uint8`` / ``int8`` (letters, or token ids with an ``alphabet``), ``int32`` or ``int64``
    (token ids), last dimension contiguous.  2-D: row i is sequence i, ``lengths[i] <= shape[1]`` of it (the padding is never read).
    1-D: the sequences lie back to back, or start at ``offsets[i]``.  ``lengths`` / ``offsets``: host integers (an object with
    ``tolist()`` goes through it).  ``alphabet``: ``None`` (bytes are letters), a ``bytes`` / ``str`` indexed by token id, or a
    ``{id: letter}`` dict; any id outside it becomes ``N``.  ``stream``: the stream that produces ``data`` -- an int handle, an
    object with ``.cuda_stream``, or ``None``: torch's current stream of the tensor's device when ``data`` is a torch tensor (and
    torch is loaded), else the null stream.  The upload waits for the work that stream holds when it is called.

    The object keeps ``data`` alive.  ``ds[k:l]`` and ``ds.take(indices)`` are ``DeviceSequences`` over the same memory with a subset
    of the (offset, length) pairs: no data moves.  Every shape, dtype and length check raises before any device call."""

    def __init__(self, data, lengths, *, offsets=None, alphabet=None, stream=None):
        cai = getattr(data, "__cuda_array_interface__", None)
        if not isinstance(cai, dict):
            raise TypeError("data must have a __cuda_array_interface__ (a device tensor or array), not %r" % type(data).__name__)
        typestr = str(cai.get("typestr"))
        if typestr not in _DEVICE_DTYPES:
            raise TypeError(f"data has dtype {typestr}: uint8, int8, int32 or int64 (|u1, |i1, <i4, <i8) is needed")
        eb = _DEVICE_DTYPES[typestr]
        shape = tuple(int(x) for x in cai["shape"])
        if len(shape) not in (1, 2):
            raise ValueError(f"data must be 1-D or 2-D, not {len(shape)}-D")
        strides = cai.get("strides")
        strides = None if strides is None else tuple(int(x) for x in strides)
        if strides is not None and shape[-1] > 1 and strides[-1] != eb:
            raise ValueError("the last dimension of data is not contiguous: call .contiguous() on it first")
        lens = _host_ints(lengths, "lengths")
        n = int(lens.size)
        if n and lens.min() < 0:
            raise ValueError(f"sequence {int(np.argmin(lens))} has the negative length {int(lens.min())}")
        if len(shape) == 2:
            if offsets is not None:
                raise ValueError("offsets belong to 1-D data: row i of 2-D data is sequence i")
            if n != shape[0]:
                raise ValueError(f"lengths has {n} entries for {shape[0]} rows")
            if n and lens.max() > shape[1]:
                i = int(np.argmax(lens))
                raise ValueError(f"sequence {i}: length {int(lens[i])} is more than the {shape[1]} columns of its row")
            row = shape[1] if strides is None else strides[0] // eb
            if strides is not None and shape[0] > 1 and (strides[0] % eb or strides[0] < 0):
                raise ValueError("the rows of data do not lie a whole, positive number of elements apart: call .contiguous() on it first")
            offs = np.arange(n, dtype=np.int64) * int(row)
            n_elems = (shape[0] - 1) * int(row) + shape[1] if shape[0] and shape[1] else 0
        else:
            n_elems = shape[0]
            if offsets is None:
                offs = np.zeros(n, np.int64)
                if n > 1:
                    np.cumsum(lens[:-1], out=offs[1:])
            else:
                offs = _host_ints(offsets, "offsets")
                if offs.size != n:
                    raise ValueError(f"offsets has {offs.size} entries for {n} lengths")
            if n:
                bad = np.nonzero((offs < 0) | (offs + lens > n_elems))[0]
                if bad.size:
                    i = int(bad[0])
                    raise ValueError(f"sequence {i}: elements [{int(offs[i])}, {int(offs[i])} + {int(lens[i])}) do not lie in the {n_elems} elements of data")
        table = normalise_alphabet(alphabet)
        if table is None and eb != 1:
            raise ValueError(f"data of dtype {typestr} holds token ids: an alphabet is needed")
        if n and lens.max() > 0x7fff0000:
            raise ValueError(f"sequence {int(np.argmax(lens))} is longer than 0x7fff0000 bases")
        ptr = cai["data"][0]
        self.data = data
        self.ptr = int(ptr) if ptr else 0
        self.n_elems, self.elem_bytes = int(n_elems), eb
        self.offsets, self.lengths = np.ascontiguousarray(offs, np.int64), np.ascontiguousarray(lens, np.int64)
        self.alphabet = table
        self.total = int(lens.sum()) if n else 0
        self.stream = self._stream_of(data, stream)

    @staticmethod
    def _stream_of(data, stream):
        if stream is None:
            import sys
            torch = sys.modules.get("torch")
            if torch is not None and isinstance(data, torch.Tensor):
                return int(torch.cuda.current_stream(data.device).cuda_stream)
            return 0
        if hasattr(stream, "cuda_stream"):
            return int(stream.cuda_stream)
        if isinstance(stream, bool) or not isinstance(stream, (int, np.integer)):
            raise TypeError("stream must be an int handle, an object with .cuda_stream, or None, not %r" % type(stream).__name__)
        return int(stream)

    def __len__(self):
        return int(self.lengths.size)

    def take(self, indices):
        """The sequences ``indices`` (any order, repeats allowed) as a ``DeviceSequences`` over the same memory."""
        idx = np.asarray(_host_ints(indices, "indices"), dtype=np.int64)
        n = len(self)
        if idx.size and (idx.min() < -n or idx.max() >= n):
            raise IndexError(f"an index is outside the {n} sequences")
        sub = DeviceSequences.__new__(DeviceSequences)
        sub.data, sub.ptr, sub.n_elems, sub.elem_bytes = self.data, self.ptr, self.n_elems, self.elem_bytes
        sub.alphabet, sub.stream = self.alphabet, self.stream
        sub.offsets, sub.lengths = np.ascontiguousarray(self.offsets[idx]), np.ascontiguousarray(self.lengths[idx])
        sub.total = int(sub.lengths.sum()) if idx.size else 0
        return sub

    def __getitem__(self, index):
        if isinstance(index, slice):
            return self.take(range(*index.indices(len(self))))
        return self.take([index])


def _upload_device(self, ds):
    """A resident :class:`Batch` from sequences that already lie in device memory (``pga_batch_create_device``): one packing kernel,
    nothing goes through the host.  With ``find_genes`` on that batch only the gene records come home."""
    if not isinstance(ds, DeviceSequences):
        raise TypeError("upload_device takes a DeviceSequences, not %r" % type(ds).__name__)
    b = Batch.__new__(Batch)
    b.ctx, b.n, b.total, b.lengths = self, len(ds), ds.total, ds.lengths.copy()
    ab = ds.alphabet
    h = ctypes.c_void_p()
    rc = self.L.pga_batch_create_device(self.h, b.n, ctypes.c_void_p(ds.ptr), ds.n_elems, ds.elem_bytes,
                                        ctypes.c_void_p(ds.offsets.ctypes.data) if b.n else None,
                                        ctypes.c_void_p(ds.lengths.ctypes.data) if b.n else None,
                                        ab, 0 if ab is None else len(ab), ctypes.c_void_p(ds.stream), ctypes.byref(h))
    if rc != PGA_OK:
        _raise(self.L, self.h, rc, "pga_batch_create_device")
    b.h = h
    return b


class _ResultOwner:
    """Keeps a ``pga_result`` alive for as long as an array built over its memory is."""

    def __init__(self, L, res):
        self.L, self.res = L, res

    def __del__(self):
        if self.res is not None:
            self.L.pga_result_free(self.res)
            self.res = None


def _view(owner, ptr, count, ctype, dtype):
    """A numpy array over ``count`` C structs at ``ptr`` (no copy); the array keeps the owning result alive."""
    if not count or not ptr:
        return np.zeros(0, dtype)
    buf = (ctype * count).from_address(ctypes.addressof(ptr.contents))
    buf._owner = owner                       # numpy array -> base: this ctypes array -> the result
    return np.frombuffer(buf, dtype=dtype)


def _unpack_result(L, res, want_nodes):
    owner = _ResultOwner(L, res)
    r = res.contents
    # contigs and genes stay where the C library put them: two views, no copies (32 MB of gene records per 250 Mbp batch)
    contigs = _view(owner, r.contigs, r.n_contigs, ContigResult, CONTIG_DTYPE)
    genes = _view(owner, r.genes, r.n_genes, Gene, GENE_DTYPE)
    nodes = None
    if want_nodes and r.nodes:
        nodes = []
        for i in range(r.n_contigs):
            nd = r.nodes[i]
            d = {"n": nd.n}
            for name, dt, mult in _NODE_FIELDS:
                ptr = getattr(nd, name)
                if nd.n == 0 or not ptr:
                    a = np.zeros((0, mult) if mult > 1 else 0, dt)
                else:
                    a = np.ctypeslib.as_array(ptr, (nd.n * mult,)).copy()
                    if mult > 1:
                        a = a.reshape(nd.n, mult)
                d[name] = a
            nodes.append(d)
    masks = None
    if r.mask_off:
        off = np.ctypeslib.as_array(r.mask_off, (r.n_contigs + 1,)).copy()
        iv = np.ctypeslib.as_array(r.masks, (2 * int(off[-1]),)).copy().reshape(-1, 2) if off[-1] else np.zeros((0, 2), np.int32)
        masks = [iv[off[i]:off[i + 1]] for i in range(r.n_contigs)]
    return BatchResult(contigs, genes, nodes, r.t_total_ms, r.t_dp_ms, r.node_passes, r.n_chains, masks)


def _upload(self, seqs):
    return Batch(self, seqs)


class PackedRecords:
    """One batch of a :class:`FastaReader` in packed form: the letters of all records back to back in a pinned staging arena of
    the reader (``ptr``), record i at ``offs[i]``, ``lens[i]`` long.  ``ids`` / ``descriptions`` are Python strings.  The arena
    is handed back to the reader by ``release()`` (called by ``Context.upload_packed`` once the letters are on the device)."""

    def __init__(self, reader, n, ids, descriptions, ptr, offs, lens, arena):
        self.reader, self.n, self.ids, self.descriptions = reader, n, ids, descriptions
        self.ptr, self.offs, self.lens, self.arena = ptr, offs, lens, arena
        self.total = int(offs[n]) if n else 0

    def sequence(self, i):
        """A copy of record i's letters (only while the arena has not been released)."""
        return ctypes.string_at(self.ptr + int(self.offs[i]), int(self.lens[i]))

    def release(self):
        if self.arena is not None:
            self.reader._free[self.arena].set()
            self.arena = None


def _upload_packed(self, pb):
    """A resident :class:`Batch` straight from a reader's pinned staging arena: no host-side packing, one DMA."""
    b = Batch.__new__(Batch)
    b.ctx, b.n, b.total = self, pb.n, pb.total
    b.lengths = np.array([int(x) for x in pb.lens[:pb.n]], np.int64)
    offs = (ctypes.c_int64 * max(1, pb.n + 1))(*[int(x) for x in pb.offs[:pb.n + 1]])
    lens = (ctypes.c_int64 * max(1, pb.n))(*[int(x) for x in pb.lens[:pb.n]])
    h = ctypes.c_void_p()
    rc = self.L.pga_batch_create_packed(self.h, pb.n, ctypes.c_void_p(pb.ptr), offs, lens, ctypes.byref(h))
    pb.release()
    if rc != PGA_OK:
        _raise(self.L, self.h, rc, "pga_batch_create_packed")
    b.h = h
    return b


def _want_nodes(want_nodes):
    if isinstance(want_nodes, str):
        if want_nodes != "device":
            raise ValueError("want_nodes must be a bool or \"device\", not %r" % (want_nodes,))
        return NODES_DEVICE
    return int(bool(want_nodes))


def _find_genes(self, batch, meta=True, closed=False, min_gene=90, min_edge_gene=60, max_overlap=60, want_nodes=False,
                mask=False, min_mask=50, model_of_contig=None):
    """``GeneFinder.find_genes`` over every contig of a resident :class:`Batch`.

    ``model_of_contig`` (single mode): contig i is called with loaded model ``model_of_contig[i]`` (``pga_find_genes_models``).
    ``want_nodes``: True also returns the winning model's node arrays (``nodes``); ``"device"`` keeps them on the device only, for
    ``render_genes(..., "scores")`` on this result before the next call on the context (``nodes`` stays None)."""
    wn = _want_nodes(want_nodes)
    p = Params(int(closed), min_gene, min_edge_gene, max_overlap, int(meta), wn, int(mask), min_mask)
    res = _P(Result)()
    if model_of_contig is None:
        rc = self.L.pga_find_genes(self.h, batch.h, ctypes.byref(p), ctypes.byref(res))
        what = "pga_find_genes"
    else:
        moc = np.ascontiguousarray(model_of_contig, dtype=np.int32)
        if moc.shape != (batch.n,):
            raise ValueError(f"model_of_contig has {moc.size} entries for {batch.n} contigs")
        rc = self.L.pga_find_genes_models(self.h, batch.h, ctypes.byref(p), ctypes.c_void_p(moc.ctypes.data), ctypes.byref(res))
        what = "pga_find_genes_models"
    if rc != PGA_OK:
        _raise(self.L, self.h, rc, what)
    out = _unpack_result(self.L, res, wn == 1)
    if batch.circular is not None:
        cuts = np.full(max(batch.n, 1), -1, np.int32)
        rc = self.L.pga_circular_cuts(self.h, batch.n, ctypes.c_void_p(cuts.ctypes.data))
        if rc != PGA_OK:
            _raise(self.L, self.h, rc, "pga_circular_cuts")
        out.cuts = cuts[:batch.n]
    if batch.sets is not None and model_of_contig is None:
        n, nm = batch.n, len(self._models)
        sm, ss = np.full(max(n, 1), -1, np.int32), np.full(max(n, 1), np.nan, np.float64)
        ms = np.full(max(n * nm, 1), np.nan, np.float64)
        rc = self.L.pga_set_choice(self.h, n, ctypes.c_void_p(sm.ctypes.data), ctypes.c_void_p(ss.ctypes.data))
        if rc == PGA_OK:
            rc = self.L.pga_model_scores(self.h, n, nm, ctypes.c_void_p(ms.ctypes.data))
        if rc != PGA_OK:
            _raise(self.L, self.h, rc, "pga_set_choice")
        out.set_models, out.set_scores, out.model_scores = sm[:n], ss[:n], ms[:n * nm].reshape(n, nm)
    return out


def _replicate(self, batch, contig_of_entry):
    """A new resident :class:`Batch` whose entry i is a device-side copy of contig ``contig_of_entry[i]`` of ``batch``."""
    coe = np.ascontiguousarray(contig_of_entry, dtype=np.int32).reshape(-1)
    h = ctypes.c_void_p()
    rc = self.L.pga_batch_replicate(self.h, batch.h, int(coe.size), ctypes.c_void_p(coe.ctypes.data), ctypes.byref(h))
    if rc != PGA_OK:
        _raise(self.L, self.h, rc, "pga_batch_replicate")
    b = Batch.__new__(Batch)
    b.ctx, b.n, b.h = self, int(coe.size), h
    b.total = None
    b.lengths = np.asarray(batch.lengths, np.int64)[coe]
    if batch.circular is not None and batch.circular[coe].any():        # the flags travel with the contigs
        b.circular = np.ascontiguousarray(batch.circular[coe])
    if batch.sets is not None:                                           # and so do the set labels
        b.sets = np.ascontiguousarray(batch.sets[coe])
    return b


def _find_coding_bases(self, batch, model_of_contig, closed=False, min_gene=90, min_edge_gene=60, max_overlap=60, mask=False,
                       min_mask=50):
    """Single mode with loaded model ``model_of_contig[i]`` on contig i, reduced on the device (``pga_find_coding_bases``).
    Returns ``(coding_bases int64, n_genes int32, score float64)``, one entry per contig."""
    p = Params(int(closed), min_gene, min_edge_gene, max_overlap, 0, 0, int(mask), min_mask)
    moc = np.ascontiguousarray(model_of_contig, dtype=np.int32)
    if moc.shape != (batch.n,):
        raise ValueError(f"model_of_contig has {moc.size} entries for {batch.n} contigs")
    n = max(batch.n, 1)
    cov, ng, sc = np.zeros(n, np.int64), np.zeros(n, np.int32), np.zeros(n, np.float64)
    rc = self.L.pga_find_coding_bases(self.h, batch.h, ctypes.byref(p), ctypes.c_void_p(moc.ctypes.data), cov.ctypes.data,
                                      ng.ctypes.data, sc.ctypes.data)
    if rc != PGA_OK:
        _raise(self.L, self.h, rc, "pga_find_coding_bases")
    return cov[:batch.n], ng[:batch.n], sc[:batch.n]


def terminal_repeat_options(n, option):
    """``trim_terminal_repeats=`` as the finder calls take it -> ``(search, (min_length, max_length, max_base_percent))``, or ``None``
    when nothing is to be searched.  ``option``: ``None`` / ``False``, ``True`` (the defaults, every sequence), an object with
    ``min_length`` / ``max_length`` / ``max_base_percent`` (every sequence), or one such entry per sequence -- a call has one set of
    parameters, so two different parameter objects in one list are a ``ValueError``."""
    default = (20, 65536, 75)

    def params(o):
        return (int(o.min_length), int(o.max_length), int(o.max_base_percent))

    if option is None or option is False:
        return None
    if option is True:
        return np.ones(max(n, 1), np.uint8)[:n], default
    if hasattr(option, "min_length"):
        return np.ones(max(n, 1), np.uint8)[:n], params(option)
    entries = list(option)
    if len(entries) != n:
        raise ValueError("`trim_terminal_repeats` has %d entries for %d sequences" % (len(entries), n))
    search, shared = np.zeros(max(n, 1), np.uint8)[:n], None
    for i, e in enumerate(entries):
        if e is None or e is False:
            continue
        search[i] = 1
        if e is True:
            continue
        if not hasattr(e, "min_length"):
            raise TypeError("trim_terminal_repeats[%d] is neither a bool nor a TerminalRepeats (%r)" % (i, type(e).__name__))
        if shared is not None and e is not shared and e != shared:
            raise ValueError("`trim_terminal_repeats` names two different TerminalRepeats in one call (sequence %d): "
                             "a call has one set of parameters" % i)
        shared = shared if shared is not None else e
    if not search.any():
        return None
    return search, (default if shared is None else params(shared))


def _find_genes_batch(self, seqs, regions=None, mask_lowercase=False, circular=None, sets=None, trim_terminal_repeats=None, **kw):
    """Upload + find + free: ``seqs`` is a list of ASCII ``bytes``/``str`` contigs.  ``regions`` (one entry per contig: ``None`` or
    ``(begin, end)`` pairs) and ``mask_lowercase`` are more mask sources (:meth:`Batch.set_masks`); ``masks`` of the result is their
    union with the runs of unknown bases of ``mask=True``.  ``circular``: as :meth:`Batch.set_circular` takes it; ``sets``: as
    :meth:`Batch.set_sets` takes it (meta mode).  ``trim_terminal_repeats``: as :func:`terminal_repeat_options` takes it -- the
    searched contigs that end in a copy of their first bases lose it on the device and are called as circles
    (``terminal_repeats`` of the result: the letters each contig lost)."""
    b = _upload_device(self, seqs) if isinstance(seqs, DeviceSequences) else Batch(self, seqs)
    t = b
    try:
        if sets is not None:
            b.set_sets(sets)
        if regions is not None or mask_lowercase:
            b.set_masks(regions, mask_lowercase)
        if circular is not None and circular is not False:
            b.set_circular(circular)      # (through a resident batch: the one-step pga_find_genes_batch has none to flag)
        tr = terminal_repeat_options(b.n, trim_terminal_repeats)
        trim = None
        if tr is not None:
            _, trim = b.terminal_repeats(tr[0], *tr[1])
            t = b.trim_terminal_repeats(trim)
        out = _find_genes(self, t, **kw)
        if trim_terminal_repeats is not None and trim_terminal_repeats is not False:
            out.terminal_repeats = trim if trim is not None else np.zeros(b.n, np.int32)
        return out
    finally:
        if t is not b:
            t.close()
        b.close()


def _nodes_stage(self, seqs, stage, translation_table=11, closed=False, min_gene=90, min_edge_gene=60, max_overlap=60,
                 is_meta=False, mask=False, min_mask=50, regions=None, mask_lowercase=False):
    """Node arrays after ``Nodes.extract`` (stage 1), ``Nodes.score`` (2) or overlapping starts (3), one dict per contig.

    Stages 2 and 3 score with model 0 of the context (``set_models`` first)."""
    b = seqs if isinstance(seqs, Batch) else Batch(self, seqs)
    try:
        if b is not seqs and (regions is not None or mask_lowercase):
            b.set_masks(regions, mask_lowercase)
        p = Params(int(closed), min_gene, min_edge_gene, max_overlap, int(is_meta), 1, int(mask), min_mask)
        res = _P(Result)()
        rc = self.L.pga_nodes_stage(self.h, b.h, ctypes.byref(p), int(stage), int(translation_table), ctypes.byref(res))
        if rc != PGA_OK:
            _raise(self.L, self.h, rc, "pga_nodes_stage")
        out = _unpack_result(self.L, res, True)
        return out if stage == STAGE_SEQUENCE else out.nodes
    finally:
        if b is not seqs:
            b.close()


def _train(self, seq, translation_table=11, start_weight=4.35, force_nonsd=False, closed=False, min_gene=90, min_edge_gene=60,
           max_overlap=60, mask=False, min_mask=50, upto=0, regions=None, mask_lowercase=False):
    """``GeneFinder.train`` on one sequence: returns the 558 392-byte ``struct _training`` as ``bytes``.  ``regions``: the masked
    intervals of that sequence."""
    b = Batch(self, [seq])
    try:
        if regions is not None or mask_lowercase:
            b.set_masks(None if regions is None else [regions], mask_lowercase)
        p = Params(int(closed), min_gene, min_edge_gene, max_overlap, 0, 0, int(mask), min_mask)
        out = ctypes.create_string_buffer(TRAINING_SIZE)
        rc = self.L.pga_train(self.h, b.h, ctypes.byref(p), int(translation_table), float(start_weight), int(force_nonsd), int(upto), out)
        if rc != PGA_OK:
            _raise(self.L, self.h, rc, "pga_train")
        return out.raw
    finally:
        b.close()


def _per_genome(value, n, dtype, name):
    a = np.asarray(value, dtype=dtype)
    a = np.full(n, a, dtype) if a.ndim == 0 else np.ascontiguousarray(a)
    if a.shape != (n,):
        raise ValueError(f"{name}: {a.size} values for {n} genomes")
    return a


def _train_batch(self, seqs, translation_table=11, start_weight=4.35, force_nonsd=False, closed=False, min_gene=90, min_edge_gene=60,
                 max_overlap=60, mask=False, min_mask=50, upto=0, regions=None, mask_lowercase=False):
    """``GeneFinder.train`` on many genomes in one call (``pga_train_batch``): ``seqs[g]`` is genome g (contigs already joined),
    the three training options a scalar or one value per genome.  Returns one 558 392-byte ``struct _training`` per genome; raises
    naming the first genome that could not be trained."""
    n = len(seqs)
    if n == 0:
        return []
    tts = _per_genome(translation_table, n, np.int32, "translation_table")
    sws = _per_genome(start_weight, n, np.float64, "start_weight")
    fns = _per_genome(np.asarray(force_nonsd, dtype=bool).astype(np.int32), n, np.int32, "force_nonsd")
    b = Batch(self, list(seqs))
    try:
        if regions is not None or mask_lowercase:
            b.set_masks(regions, mask_lowercase)
        p = Params(int(closed), min_gene, min_edge_gene, max_overlap, 0, 0, int(mask), min_mask)
        out = np.zeros(n * TRAINING_SIZE, np.uint8)
        status = np.zeros(n, np.int32)
        rc = self.L.pga_train_batch(self.h, b.h, ctypes.byref(p), tts.ctypes.data, sws.ctypes.data, fns.ctypes.data, int(upto),
                                    out.ctypes.data, status.ctypes.data)
        if rc != PGA_OK:
            _raise(self.L, self.h, rc, "pga_train_batch")
        bad = np.flatnonzero(status != PGA_OK)
        if bad.size:
            g = int(bad[0])
            raise (ValueError if status[g] == PGA_EINVAL else PgaError)(
                f"pga_train_batch: genome {g} could not be trained (no start / stop node; code {int(status[g])})")
        return [out[g * TRAINING_SIZE:(g + 1) * TRAINING_SIZE].tobytes() for g in range(n)]
    finally:
        b.close()


def _translate_genes(self, batch, result, tables=None, unknown_residue="X", include_stop=True, strict=True):
    """Proteins of ``result.genes`` (a result of ``find_genes`` on the resident ``batch``), translated on the device.

    ``tables``: translation table per contig (default: the table of the model that won the contig).  Returns
    ``(letters, offsets)``: gene g is ``letters[offsets[g]:offsets[g + 1]]`` (a uint8 array of ASCII codes)."""
    genes = np.ascontiguousarray(result.genes)
    n = len(genes)
    tables = np.ascontiguousarray(_default_tables(self, result.contigs) if tables is None else tables, np.int32)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(_residue_counts(genes, include_stop), out=off[1:])
    out = np.zeros(max(int(off[-1]), 1), np.uint8)
    unk = unknown_residue.encode("ascii") if isinstance(unknown_residue, str) else bytes(unknown_residue)
    if len(unk) != 1:
        raise ValueError("`unknown_residue` must be a single character")
    rc = self.L.pga_translate_genes(self.h, batch.h, n, genes.ctypes.data, tables.ctypes.data, unk[0], int(include_stop), int(strict),
                                    off.ctypes.data, out.ctypes.data)
    if rc != PGA_OK:
        _raise(self.L, self.h, rc, "pga_translate_genes")
    return out[:int(off[-1])], off


def _default_tables(self, contigs):
    """The translation table of every contig of a result: that of the model that won it, 11 where none did."""
    tts = [int(np.frombuffer(m[8:12].tobytes(), np.int32)[0]) for m in self._models]
    return [tts[c["model"]] if c["model"] >= 0 else 11 for c in contigs]


def _tables_or_default(self, result_or_genes, tables):
    """``tables`` where the caller gave them, else those of the models that won the result's contigs."""
    if tables is not None:
        return tables
    contigs = getattr(result_or_genes, "contigs", None)
    if contigs is None:
        raise ValueError("bare gene records carry no models: pass tables=, the translation table of every contig")
    return _default_tables(self, contigs)


def _tables_arg(tables, n_contigs, unit=None):
    """The translation table of every contig as the library takes it: (the int32 array, its pointer).  ``unit``: that of a rule which
    reads ``tables`` only for its protein unit; without them the pointer is NULL for any other."""
    if tables is None and unit is not None:
        if unit == "protein":
            raise ValueError("the protein unit needs tables=, the translation table of every contig")
        return None, ctypes.c_void_p(0)
    tables = np.ascontiguousarray(tables, np.int32)
    if tables.shape != (n_contigs,):
        raise ValueError(f"tables has {tables.size} entries for {n_contigs} contigs")
    return tables, ctypes.c_void_p(tables.ctypes.data)


def _gene_begin(genes, n_contigs):
    """The genes of contig i are records ``gene_begin[i] .. gene_begin[i + 1]``: int64, or ``None`` when the records are not in contig
    order."""
    if len(genes) and np.any(np.diff(genes["contig"]) < 0):
        return None
    return np.searchsorted(genes["contig"], np.arange(n_contigs + 1)).astype(np.int64)


def _residue_counts(genes, include_stop):
    """Residues of every gene record (int64): host arithmetic on the coordinates, as the library does it."""
    stop_edge = np.where(genes["strand"] == 1, genes["partial_end"], genes["partial_begin"]).astype(bool)
    r = (genes["end"].astype(np.int64) - genes["begin"] + 1) // 3
    return np.maximum(r if include_stop else r - (~stop_edge), 0)


AMINO_ACIDS = "ACDEFGHIKLMNPQRSTVWY"
_TOKEN_DTYPES = {"uint8": (1, "|u1", 0, 255), "int32": (4, "<i4", -(1 << 31), (1 << 31) - 1), "int64": (8, "<i8", -(1 << 63), (1 << 63) - 1)}


def _token_id(value, name):
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)):
        raise TypeError(f"{name} must be an integer id, not {type(value).__name__}")
    return int(value)


class _TensorRule:
    """What the rules of the device-tensor outputs share.  Every rule gets value semantics over ``_key()`` -- the attributes
    ``_fields`` names -- and pickles through it (``_derive`` restores what the constructor computes from them); it says what one row
    is (``row`` and its ``unit``) and what it needs of every contig of the batch (``per_contig``: ``"tables"`` or ``"lengths"``),
    and has ``write``, the call on raw handles with just that.  Only the rules that write rows of one element type in either
    layout -- ProteinTokens, BaseLabels, GeneWindows -- take the rest: the format (``_set_format``, ``elem_bytes``, ``typestr``),
    ``_check_fit`` and the head of the options struct (``_opts``)."""

    _fields = ()

    def _set_format(self, dtype, layout):
        name = dtype if isinstance(dtype, str) else np.dtype(dtype).name
        if name not in _TOKEN_DTYPES:
            raise ValueError(f"dtype must be uint8, int32 or int64, not {name!r}")
        if layout not in ("padded", "ragged"):
            raise ValueError(f"layout must be \"padded\" or \"ragged\", not {layout!r}")
        self.dtype, self.layout = name, layout

    elem_bytes = property(lambda self: _TOKEN_DTYPES[self.dtype][0])
    typestr = property(lambda self: _TOKEN_DTYPES[self.dtype][1])

    def _check_fit(self, ids):                           # (what, value or None) of everything that goes into the tensor
        lo, hi = _TOKEN_DTYPES[self.dtype][2:]
        for what, v in ids:
            if v is not None and not lo <= v <= hi:
                raise ValueError(f"{what}, {v}, does not fit {self.dtype}")

    def _key(self):
        return tuple(getattr(self, f) for f in self._fields)

    def _derive(self):
        pass

    def __eq__(self, other):
        return isinstance(other, type(self)) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __reduce__(self):
        return _rule_from_key, (type(self), self._key())

    def _opts(self, o, row_width, row_stride):
        o.elem_bytes, o.layout = self.elem_bytes, TOKENS_PADDED if self.layout == "padded" else TOKENS_RAGGED
        o.row_width, o.row_stride, o.pad = int(row_width), int(row_stride), self.pad
        return o


def _rule_from_key(cls, key):
    rule = cls.__new__(cls)
    for f, v in zip(cls._fields, key):
        setattr(rule, f, v)
    rule._derive()
    return rule


class ProteinTokens(_TensorRule):
    """How ``translate_tokens`` / ``find_proteins_batch`` write proteins into a device tensor (``pga_token_opts``; the rule is in
    ``pyrodigal_amd.h``).

    ``vocabulary``: a string (the id of a letter is its position) or a ``{letter: id}`` mapping.  Every letter a translation can hold
    under the options needs an id -- the 20 amino acids, ``*`` with ``include_stop``, and ``unknown_residue`` -- its own or
    ``unknown``; any other letter without an id of its own (a ``*`` inside a gene read under a foreign table when ``include_stop`` is
    off) gets ``unknown``, or the id of ``unknown_residue``.  ``bos`` / ``eos``: ids put before / behind every protein, ``None``:
    none.  ``pad`` fills the rows of the padded layout.  ``dtype``: ``"uint8"``, ``"int32"`` or ``"int64"``; every id must fit it.
    ``max_length``: the most tokens of a gene, specials included (``eos`` survives the cut).  ``include_stop``, ``strict`` and
    ``unknown_residue`` are those of ``translate_genes``.  Everything that needs no device is checked here.  Hashable and picklable."""

    def __init__(self, vocabulary, *, unknown=None, bos=None, eos=None, pad=0, dtype="int64", layout="padded", max_length=None,
                 include_stop=False, strict=True, unknown_residue="X"):
        self._set_format(dtype, layout)
        unk = unknown_residue.decode("ascii", "replace") if isinstance(unknown_residue, (bytes, bytearray)) else unknown_residue
        if not isinstance(unk, str) or len(unk) != 1 or not 0 < ord(unk) < 128:
            raise ValueError("`unknown_residue` must be a single ASCII character")
        if isinstance(vocabulary, str):
            if len(set(vocabulary)) != len(vocabulary):
                raise ValueError("a letter occurs twice in the vocabulary string")
            given = {ch: k for k, ch in enumerate(vocabulary)}
        elif hasattr(vocabulary, "items"):
            given = {}
            for ch, v in vocabulary.items():
                ch = ch.decode("ascii", "replace") if isinstance(ch, (bytes, bytearray)) else ch
                if not isinstance(ch, str) or len(ch) != 1:
                    raise ValueError(f"vocabulary key {ch!r} is not one letter")
                given[ch] = _token_id(v, f"the id of {ch!r}")
        else:
            raise TypeError("vocabulary must be a string or a {letter: id} mapping, not %r" % type(vocabulary).__name__)
        for ch in given:
            if not 0 < ord(ch) < 128:
                raise ValueError(f"vocabulary letter {ch!r} is not a 7-bit ASCII character")
        self.unknown = None if unknown is None else _token_id(unknown, "unknown")
        self.bos = None if bos is None else _token_id(bos, "bos")
        self.eos = None if eos is None else _token_id(eos, "eos")
        self.pad = _token_id(pad, "pad")
        self.include_stop, self.strict, self.unknown_residue = bool(include_stop), bool(strict), unk
        for ch in AMINO_ACIDS + ("*" if self.include_stop else "") + unk:
            if ch not in given and self.unknown is None:
                raise ValueError(f"the vocabulary has no id for {ch!r}, a letter the translation can hold, and `unknown` is None")
        rest = self.unknown if self.unknown is not None else given[unk]
        self.vocab = tuple(given.get(chr(k), rest) for k in range(128))
        self._check_fit([(f"the id of {chr(k)!r}", self.vocab[k]) for k in range(128) if chr(k) in given] +
                        [("unknown", self.unknown), ("bos", self.bos), ("eos", self.eos), ("pad", self.pad)])
        self._derive()
        if max_length is not None:
            max_length = _token_id(max_length, "max_length")
            if max_length < self.specials + 1:
                raise ValueError(f"max_length = {max_length} leaves no room for a residue beside {self.specials} special tokens")
        self.max_length = max_length

    row, unit, per_contig = "gene", "tokens", "tables"
    _fields = ("vocab", "unknown", "bos", "eos", "pad", "dtype", "layout", "max_length", "include_stop", "strict", "unknown_residue")

    def _derive(self):
        self.specials = (self.bos is not None) + (self.eos is not None)

    def write(self, L, ctx_h, batch_h, device, genes, tables, out=None, stream=None):
        return tokens_into(L, ctx_h, batch_h, device, len(tables), genes, tables, self, out, stream)

    def __repr__(self):
        return "pyrodigal_amd.ProteinTokens(dtype=%r, layout=%r, bos=%r, eos=%r, max_length=%r)" % (
            self.dtype, self.layout, self.bos, self.eos, self.max_length)

    def lengths(self, genes):
        """Tokens of every gene record, specials included (int64): host arithmetic on the coordinates, as the library does it."""
        r = _residue_counts(genes, self.include_stop)
        if self.max_length is not None:
            r = np.minimum(r, self.max_length - self.specials)
        return (r + self.specials).astype(np.int64)

    def opts(self, row_width=0, row_stride=0):
        o = self._opts(TokenOpts(), row_width, row_stride)
        o.include_stop, o.strict, o.unknown_residue = int(self.include_stop), int(self.strict), ord(self.unknown_residue)
        o.max_length = 0 if self.max_length is None else self.max_length
        o.vocab[:] = self.vocab
        o.bos = TOKEN_NONE if self.bos is None else self.bos
        o.eos = TOKEN_NONE if self.eos is None else self.eos
        return o


class _ContigViews:
    """The per-contig views of a result (``proteins``, ``labels_of``, ``windows``, ``counts_of``, ``starts``): entry i is
    ``part(a, b)``, views of the tensors -- no copy -- for the rows ``a .. b`` of contig i: ``begin[i] .. begin[i + 1]``, its genes
    (``gene_begin``), or ``i .. i + 1`` where a contig is a row (``begin=None``: ``n`` of them)."""

    def __init__(self, part, begin, n=0):
        self.part, self.begin = part, np.arange(n + 1) if begin is None else begin

    def __len__(self):
        return len(self.begin) - 1

    def __getitem__(self, i):
        i = range(len(self))[i]
        return self.part(int(self.begin[i]), int(self.begin[i + 1]))


def _gene_views(d, *tensors):
    """``_ContigViews`` of the genes' rows (padded) or slice (ragged) of tensors that share ``d.offsets``."""
    if d.gene_begin is None:
        raise ValueError("the gene records were not in contig order: there are no per-contig views")
    cut = (lambda a, b: slice(a, b)) if d.offsets is None else (lambda a, b: slice(int(d.offsets[a]), int(d.offsets[b])))
    return _ContigViews((lambda a, b: tensors[0][cut(a, b)]) if len(tensors) == 1 else (lambda a, b: tuple(t[cut(a, b)] for t in tensors)),
                        d.gene_begin)


class DeviceProteins:
    """Proteins of gene records as token ids in device memory.  ``tokens``: the tensor (``[G, W]`` padded, 1-D ragged); ``lengths``:
    tokens of every gene (numpy int64, host); ``offsets``: ragged only, gene g is ``tokens[offsets[g]:offsets[g + 1]]``;
    ``gene_begin``: the genes of contig i are rows ``gene_begin[i] .. gene_begin[i + 1]`` (``None`` when the records were not in
    contig order); ``proteins[i]``: contig i's rows or slice as a view of ``tokens``."""

    def __init__(self, tokens, lengths, offsets, gene_begin, device, L=None, ctx_h=None):
        self.tokens, self.lengths, self.offsets, self.gene_begin, self.device = tokens, lengths, offsets, gene_begin, device
        self._L, self._ctx_h = L, ctx_h

    @property
    def proteins(self):
        return _gene_views(self, self.tokens)

    def align(self, pairs, spec, out=None, stream=None):
        """``(distance, passed)`` of every pair of proteins (``pga_align_pairs``): ``pairs`` is a contiguous int64 ``[P, 2]`` device
        tensor of gene indices -- the ``edges`` of a :class:`DeviceClusters`, say -- and ``spec`` a :class:`ProteinAlignments`.
        ``distance[p]`` is the edit distance of the two token rows, specials included, capped at ``spec.max_distance + 1``;
        ``passed[p]`` is 1 where it is within ``max_distance`` and the identity over the longer row is at least
        ``spec.min_identity``; a pair with an index outside ``0 .. G - 1`` gets -1 and 0.  Either layout: the pad of a padded
        tensor is not read.  ``out``: two contiguous int64 ``[P]`` objects with ``__cuda_array_interface__`` (``None`` for the
        second), omitted: torch tensors.  The context of the call that made the tokens must still be open."""
        if self._L is None:
            raise ValueError("this DeviceProteins names no context: use Context.align_pairs")
        n = len(self.lengths)
        if self.offsets is not None:
            begin = np.ascontiguousarray(self.offsets[:n], np.int64)
        else:
            shape, strides = _device_array(self.tokens, "tokens")[1:]
            eb = np.dtype(str(self.tokens.__cuda_array_interface__["typestr"])).itemsize
            begin = np.arange(n, dtype=np.int64) * (strides[0] // eb if n > 1 else (shape[1] if len(shape) > 1 else 0))
        return align_into(self._L, self._ctx_h, self.device, self.tokens, begin, self.lengths, pairs, spec, out, stream)

    def cu_seqlens(self):
        """The exclusive scan of ``lengths`` as an int32 tensor on the tokens' device (torch)."""
        return _cu_seqlens(self.lengths, self.tokens, self.device)


def _cu_seqlens(lengths, tensor, device):
    import torch
    cu = np.zeros(len(lengths) + 1, np.int64)
    np.cumsum(lengths, out=cu[1:])
    if cu[-1] >= 1 << 31:
        raise OverflowError("more than 2^31 elements do not fit an int32 cu_seqlens")
    dev = tensor.device if isinstance(tensor, torch.Tensor) else torch.device("cuda", device)
    return torch.from_numpy(cu.astype(np.int32)).to(dev)


def _contiguous_strides(shape, elem_bytes):
    return tuple(elem_bytes * int(np.prod(shape[k + 1:])) for k in range(len(shape)))


def _device_array(x, name, typestr=None, expects=None):
    """The one reader of ``__cuda_array_interface__``: (pointer, shape, strides in bytes -- those of a contiguous array where the
    interface gives none) of ``x``, which the messages call ``name``.  ``typestr``: the element type it must have, ``expects``: the
    caller's words for that.  What the shape must be is the caller's to say."""
    cai = getattr(x, "__cuda_array_interface__", None)
    if not isinstance(cai, dict):
        raise TypeError("%s must have a __cuda_array_interface__ (a device tensor or array), not %r" % (name, type(x).__name__))
    if typestr is not None and str(cai.get("typestr")) != typestr:
        raise TypeError(f"{name} has dtype {cai.get('typestr')}: {expects}")
    shape = tuple(int(v) for v in cai["shape"])
    strides = cai.get("strides")
    if strides is None:
        strides = _contiguous_strides(shape, np.dtype(str(cai["typestr"])).itemsize)
    ptr = cai["data"][0]
    return int(ptr) if ptr else 0, shape, tuple(int(v) for v in strides)


def _torch_outputs(device, stream, shapes_and_dtypes, how_many):
    """No ``out=``: new torch tensors on ``device``, and torch's current stream there unless the caller named one.  ``how_many``: the
    caller's words for what ``out=`` would have been."""
    try:
        import torch
    except ImportError:
        raise TypeError(f"torch is not installed: pass out=, {how_many} with __cuda_array_interface__") from None
    with torch.cuda.device(device):
        out = tuple(torch.empty(shape, dtype=getattr(torch, dtype), device="cuda") for shape, dtype in shapes_and_dtypes)
        if stream is None:
            stream = int(torch.cuda.current_stream().cuda_stream)
    return out, stream


def _device_output(spec, out, stream, device, lens, total, row, unit):
    """The device tensor a rule writes (``tokens_into`` and ``labels_into`` share this): ``out`` checked against the rule's element
    type and layout and against ``lens``, the elements of every row, or a new torch tensor under torch's current stream.  Returns
    (out, stream, its device pointer, W, S, the elements the layout may use)."""
    n, eb, padded = len(lens), spec.elem_bytes, spec.layout == "padded"
    longest = int(lens.max()) if n else 0
    if out is None:
        (out,), stream = _torch_outputs(device, stream, [((n, longest) if padded else (total,), spec.dtype)], "a device array")
    ptr, shape, strides = _device_array(out, "out", spec.typestr, f"the rule writes {spec.dtype} ({spec.typestr})")
    if shape[-1] > 1 and strides[-1] != eb:
        raise ValueError("the last dimension of out is not contiguous")
    width = stride = 0
    if padded:
        if len(shape) != 2 or shape[0] != n:
            raise ValueError(f"the padded layout needs a [{n}, W] tensor, not one of shape {shape}")
        width = shape[1]
        stride = width if n < 2 else strides[0] // eb
        if n > 1 and (strides[0] % eb or strides[0] < 0):
            raise ValueError("the rows of out do not lie a whole, positive number of elements apart")
        if width < longest:
            raise ValueError(f"out has {width} columns: {row} {int(np.argmax(lens))} has {longest} {unit}")
        n_out = (n - 1) * stride + width if n else 0
    else:
        if len(shape) != 1:
            raise ValueError(f"the ragged layout needs a 1-D tensor, not one of shape {shape}")
        if shape[0] < total:
            raise ValueError(f"out has {shape[0]} elements: the {row}s have {total} {unit}")
        n_out = shape[0]
    return out, stream, ptr, width, stride, n_out


def _rows_into(L, ctx_h, call, args, spec, lens, device, out, stream):
    """What ``tokens_into`` and ``labels_into`` share: ``out`` checked against the rows' ``lens`` under ``spec``, and the raw ``call``
    with ``args`` in front of the options.  Returns (out, offsets or None, the lengths the library reports)."""
    n = len(lens)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    out, stream, ptr, width, stride, n_out = _device_output(spec, out, stream, device, lens, int(off[-1]), spec.row, spec.unit)
    len_out = np.zeros(max(n, 1), np.int64)
    o = spec.opts(width, stride)
    rc = getattr(L, call)(ctx_h, *args, ctypes.byref(o), ctypes.c_void_p(ptr), n_out,
                          ctypes.c_void_p(DeviceSequences._stream_of(out, stream)), ctypes.c_void_p(len_out.ctypes.data))
    if rc != PGA_OK:
        _raise(L, ctx_h, rc, call)
    return out, None if spec.layout == "padded" else off, len_out[:n]


def tokens_into(L, ctx_h, batch_h, device, n_contigs, genes, tables, spec, out=None, stream=None):
    """``pga_translate_genes_tokens`` on raw handles (what ``Context.translate_tokens`` and the finder's device call share): the token
    ids of ``genes`` (GENE_DTYPE records of the resident batch) under ``tables`` into ``out``, or into a new torch tensor."""
    if not isinstance(spec, ProteinTokens):
        raise TypeError("the token rule must be a ProteinTokens, not %r" % type(spec).__name__)
    genes = np.ascontiguousarray(genes, dtype=GENE_DTYPE)
    tables, p_tab = _tables_arg(tables, n_contigs)
    n, lens = len(genes), spec.lengths(genes)
    args = (batch_h, n, ctypes.c_void_p(genes.ctypes.data), p_tab)
    out, off, len_out = _rows_into(L, ctx_h, "pga_translate_genes_tokens", args, spec, lens, device, out, stream)
    assert np.array_equal(len_out, lens)
    return DeviceProteins(out, lens, off, _gene_begin(genes, n_contigs), device, L, ctx_h)


def _translate_tokens(self, batch, result_or_genes, spec, out=None, tables=None, stream=None):
    """Proteins of gene records of the resident ``batch`` as token ids in device memory (``pga_translate_genes_tokens``): nothing of
    them comes to the host.  ``result_or_genes``: a result of ``find_genes`` on the batch, or gene records of one (any subset or
    order; then with ``tables``).  ``spec``: a :class:`ProteinTokens`.  ``out``: any object with ``__cuda_array_interface__`` --
    1-D for the ragged layout, ``[G, W]`` with a contiguous last dimension for the padded one; ``None``: a torch tensor is allocated
    on the context's device under torch's current stream.  ``tables``: translation table per contig (default: that of the model that
    won the contig).  ``stream``: the stream that last used ``out``, as in :class:`DeviceSequences`.  Returns a :class:`DeviceProteins`."""
    genes = getattr(result_or_genes, "genes", result_or_genes)
    tables = _tables_or_default(self, result_or_genes, tables)
    return tokens_into(self.L, self.h, batch.h, self.device, batch.n, genes, tables, spec, out, stream)


LABEL_PRESETS = ("raw", "coding", "strand", "frame")


def label_class_map(preset):
    """The 256 ids of a preset of :class:`BaseLabels`, indexed by the raw byte of the rule in ``pyrodigal_amd.h``."""
    ids = []
    for raw in range(256):
        fwd, rev = raw & 0x07, raw & 0x38
        if preset == "raw":
            ids.append(raw)
        elif preset == "coding":
            ids.append(1 if raw & 0x3f else 0)
        elif preset == "strand":
            ids.append((1 if fwd else 0) + (2 if rev else 0))
        elif preset == "frame":
            pos = raw & 0x3f
            ids.append(0 if not pos else 7 if pos & (pos - 1) else pos.bit_length())
        else:
            raise ValueError("classes must be 256 ids or one of %s, not %r" % (", ".join(map(repr, LABEL_PRESETS)), preset))
    return tuple(ids)


class BaseLabels(_TensorRule):
    """How ``label_bases`` / ``find_labels_batch`` write the annotation of every base into a device tensor (``pga_label_opts``; the
    rule is in ``pyrodigal_amd.h``).

    ``classes``: 256 ids, indexed by the raw byte of a base (codon position per strand, start and stop codon bits), or a preset:
    ``"raw"`` the byte itself; ``"coding"`` 0 or 1, by ``raw & 0x3f``; ``"strand"`` 0 none, 1 forward only, 2 reverse only, 3 both;
    ``"frame"`` 0 intergenic, 1-3 forward codon position, 4-6 reverse codon position, 7 when more than one of the six position bits
    is set.  ``pad`` fills the rows of the padded layout behind a contig's last base: -100 by default for the signed types (torch's
    ``ignore_index``); it must be given for ``uint8`` in the padded layout.  ``dtype``: ``"uint8"``, ``"int32"`` or ``"int64"``; every
    id must fit it.  Everything that needs no device is checked here.  Hashable and picklable."""

    def __init__(self, classes="frame", *, pad=None, dtype="int64", layout="padded"):
        self._set_format(dtype, layout)
        if isinstance(classes, str):
            self.class_map = label_class_map(classes)
        else:
            ids = list(classes)
            if len(ids) != 256:
                raise ValueError(f"classes has {len(ids)} ids: there is one for each of the 256 raw bytes")
            self.class_map = tuple(_token_id(v, f"the id of raw byte {k:#04x}") for k, v in enumerate(ids))
        self.classes = classes if isinstance(classes, str) else None
        if pad is None:
            if layout == "padded" and self.dtype == "uint8":
                raise ValueError("the padded layout of uint8 labels needs `pad`: the default, -100, does not fit")
            pad = -100 if self.dtype != "uint8" else 0
        self.pad = _token_id(pad, "pad")
        self._check_fit([(f"the id of raw byte {k:#04x}", v) for k, v in enumerate(self.class_map)] + [("pad", self.pad)])

    row, unit, per_contig = "contig", "bases", "lengths"
    _fields = ("class_map", "classes", "pad", "dtype", "layout")

    def write(self, L, ctx_h, batch_h, device, genes, lengths, out=None, stream=None):
        return labels_into(L, ctx_h, batch_h, device, lengths, genes, self, out, stream)

    def __repr__(self):
        return "pyrodigal_amd.BaseLabels(%s, pad=%r, dtype=%r, layout=%r)" % (
            repr(self.classes) if self.classes is not None else "<256 ids>", self.pad, self.dtype, self.layout)

    def opts(self, row_width=0, row_stride=0):
        o = self._opts(LabelOpts(), row_width, row_stride)
        o.class_map[:] = self.class_map
        return o


class DeviceLabels:
    """The annotation of every base of a batch in device memory.  ``labels``: the tensor (``[B, W]`` padded, 1-D ragged);
    ``lengths``: the bases of every contig as the batch holds it (numpy int64, host; the trimmed length of a record trimmed by
    ``trim_terminal_repeats``); ``offsets``: ragged only, contig i is ``labels[offsets[i]:offsets[i + 1]]``; ``labels_of[i]``:
    contig i's own elements as a view of ``labels``."""

    def __init__(self, labels, lengths, offsets, device):
        self.labels, self.lengths, self.offsets, self.device = labels, lengths, offsets, device

    @property
    def labels_of(self):
        # contig i's row (padded, its first ``lengths[i]`` elements) or slice (ragged)
        if self.offsets is None:
            return _ContigViews(lambda i, _: self.labels[i, :int(self.lengths[i])], None, len(self.lengths))
        return _ContigViews(lambda i, j: self.labels[int(self.offsets[i]):int(self.offsets[j])], None, len(self.lengths))

    def cu_seqlens(self):
        """The exclusive scan of ``lengths`` as an int32 tensor on the labels' device (torch)."""
        return _cu_seqlens(self.lengths, self.labels, self.device)


def labels_into(L, ctx_h, batch_h, device, lengths, genes, spec, out=None, stream=None):
    """``pga_label_bases`` on raw handles (what ``Context.label_bases`` and the finder's device call share): the labels of the bases
    of the resident batch, whose contigs have ``lengths`` bases, under ``genes`` (GENE_DTYPE records) into ``out``, or into a new
    torch tensor."""
    if not isinstance(spec, BaseLabels):
        raise TypeError("the label rule must be a BaseLabels, not %r" % type(spec).__name__)
    genes, lens = np.ascontiguousarray(genes, dtype=GENE_DTYPE), np.ascontiguousarray(lengths, np.int64)
    args = (batch_h, len(genes), ctypes.c_void_p(genes.ctypes.data))
    out, off, len_out = _rows_into(L, ctx_h, "pga_label_bases", args, spec, lens, device, out, stream)
    if not np.array_equal(len_out, lens):
        raise ValueError("`lengths` are not those of the batch")
    return DeviceLabels(out, lens, off, device)


def _label_bases(self, batch, result_or_genes, spec, out=None, stream=None):
    """The annotation of every base of the resident ``batch`` under gene records, as a device tensor in the shape of the input
    (``pga_label_bases``): nothing comes to the host.  ``result_or_genes``: a result of ``find_genes`` on the batch, or gene records
    of one (any subset or order).  ``spec``: a :class:`BaseLabels`.  ``out``: any object with ``__cuda_array_interface__`` -- 1-D for
    the ragged layout, ``[B, W]`` with a contiguous last dimension for the padded one; ``None``: a torch tensor is allocated on the
    context's device under torch's current stream.  ``stream``: the stream that last used ``out``, as in :class:`DeviceSequences`.
    Returns a :class:`DeviceLabels`."""
    genes = getattr(result_or_genes, "genes", result_or_genes)
    return labels_into(self.L, self.h, batch.h, self.device, batch.lengths, genes, spec, out, stream)


WINDOW_LETTERS = "ACGT"                                      # the public order of pga_window_opts.ids
WINDOW_CODONS_ACGT = tuple(a + b + c for a in WINDOW_LETTERS for b in WINDOW_LETTERS for c in WINDOW_LETTERS)
_WINDOW_ANCHORS = {"start": WINDOW_START, "end": WINDOW_END}
_WINDOW_MAX_DELTA = 1 << 30


class GeneWindows(_TensorRule):
    """How ``gene_windows`` / ``find_windows_batch`` write the nucleotides of every gene, or of a region around it, into a device
    tensor, one row per gene in the gene's own reading direction (``pga_window_opts``; the rule is in ``pyrodigal_amd.h``).

    ``begin`` / ``end``: ``(anchor, delta)`` with the anchor ``"start"`` (the gene's first base) or ``"end"`` (one past its last
    base); the window runs from ``begin`` up to but excluding ``end``, so the defaults are the gene itself, ``("start", -60)`` ..
    ``("start", 30)`` a 90-base start context and ``("end", 0)`` .. ``("end", 50)`` the downstream region.  A window that is empty or
    inverted on a gene is a row without bases.  ``unit``: ``"base"``, one token per base, or ``"codon"``, one per three bases (both
    deltas must then be multiples of 3).  ``vocabulary``: ``None`` gives A, C, G, T = 0 .. 3 and N = 4, or the 64 codons = 0 .. 63
    in ACGT order and unknown = 64; a string (bases only: the id of a letter is its position) or a ``{letter-or-codon: id}`` mapping
    must cover all four letters or all 64 codons, and may hold ``N`` / ``NNN`` for ``unknown``, the id of a letter that is not A, C,
    G or T or of a codon with one.  ``outside``: the id of a base (or of a codon that touches one) beyond the ends of a linear
    contig; by default that of ``unknown``.  On a circular contig a window wraps instead.  ``bos`` / ``eos``: ids put before /
    behind every row, ``None``: none.  ``pad`` fills the rows of the padded layout and must be given for it.  ``dtype``:
    ``"uint8"``, ``"int32"`` or ``"int64"``; every id must fit it.  ``max_length``: the most tokens of a row, specials included
    (``eos`` survives the cut).  Everything that needs no device is checked here.  Hashable and picklable."""

    def __init__(self, begin=("start", 0), end=("end", 0), *, unit="base", vocabulary=None, unknown=None, outside=None, bos=None,
                 eos=None, pad=None, dtype="int64", layout="padded", max_length=None):
        self._set_format(dtype, layout)
        if unit not in ("base", "codon"):
            raise ValueError(f"unit must be \"base\" or \"codon\", not {unit!r}")
        self.token_unit = unit                           # (`unit` is what a row is counted in, as for every rule)
        self.begin, self.end = self._bound("begin", begin), self._bound("end", end)
        keys = tuple(WINDOW_LETTERS) if unit == "base" else WINDOW_CODONS_ACGT
        unknown_key = "N" * len(keys[0])
        unknown = None if unknown is None else _token_id(unknown, "unknown")
        if vocabulary is None:
            given = {key: k for k, key in enumerate(keys)}
            if unknown is None:
                unknown = len(keys)
        elif isinstance(vocabulary, str):
            if unit != "base":
                raise TypeError("a vocabulary string names bases: the codon unit takes a {codon: id} mapping")
            if len(set(vocabulary.upper())) != len(vocabulary):
                raise ValueError("a letter occurs twice in the vocabulary string")
            given = {ch: k for k, ch in enumerate(vocabulary.upper()) if ch in keys or ch == unknown_key}      # (other letters: specials)
        elif hasattr(vocabulary, "items"):
            given = {}
            for key, v in vocabulary.items():
                key = key.decode("ascii", "replace") if isinstance(key, (bytes, bytearray)) else key
                if not isinstance(key, str):
                    raise ValueError(f"vocabulary key {key!r} is not a string")
                if key.upper() in given:
                    raise ValueError(f"vocabulary key {key!r} occurs twice")
                given[key.upper()] = _token_id(v, f"the id of {key!r}")
        else:
            raise TypeError("vocabulary must be None, a string or a {letter-or-codon: id} mapping, not %r" % type(vocabulary).__name__)
        for key in given:
            if key not in keys and key != unknown_key:
                raise ValueError(f"vocabulary key {key!r} is not one of {', '.join(keys[:4])}, ... or {unknown_key}")
        for key in keys:
            if key not in given:
                raise ValueError(f"the vocabulary has no id for {key!r}: it must cover all {len(keys)} {unit}s")
        if unknown is None:
            if unknown_key not in given:
                raise ValueError(f"the vocabulary has no id for {unknown_key!r} and `unknown` is None")
            unknown = given[unknown_key]
        self.unknown = unknown
        self.outside = unknown if outside is None else _token_id(outside, "outside")
        self.ids = tuple(given[key] for key in keys) + (self.unknown, self.outside)
        self.bos = None if bos is None else _token_id(bos, "bos")
        self.eos = None if eos is None else _token_id(eos, "eos")
        if pad is None:
            if layout == "padded":
                raise ValueError("the padded layout needs `pad`, the id that fills the rows behind their tokens")
            pad = 0
        self.pad = _token_id(pad, "pad")
        self._check_fit([(f"the id of {key!r}", v) for key, v in zip(keys, self.ids)] +
                        [("unknown", self.unknown), ("outside", self.outside), ("bos", self.bos), ("eos", self.eos), ("pad", self.pad)])
        self.specials = (self.bos is not None) + (self.eos is not None)
        if max_length is not None:
            max_length = _token_id(max_length, "max_length")
            if max_length < self.specials + 1:
                raise ValueError(f"max_length = {max_length} leaves no room for a {unit} beside {self.specials} special tokens")
        self.max_length = max_length

    def _bound(self, name, bound):
        try:
            anchor, delta = bound
        except (TypeError, ValueError):
            raise ValueError(f"{name} must be (anchor, delta), not {bound!r}") from None
        if anchor not in _WINDOW_ANCHORS:
            raise ValueError(f"the anchor of {name} must be \"start\" or \"end\", not {anchor!r}")
        delta = _token_id(delta, f"the delta of {name}")
        if abs(delta) > _WINDOW_MAX_DELTA:
            raise ValueError(f"the delta of {name}, {delta}, is beyond 2^30 in size")
        if self.token_unit == "codon" and delta % 3:
            raise ValueError(f"the delta of {name}, {delta}, is no multiple of 3, which the codon unit needs")
        return (anchor, delta)

    row, unit, per_contig = "gene", "tokens", "lengths"
    _fields = ("begin", "end", "token_unit", "ids", "bos", "eos", "pad", "dtype", "layout", "max_length")

    def _derive(self):
        self.unknown, self.outside = self.ids[-2:]
        self.specials = (self.bos is not None) + (self.eos is not None)

    def write(self, L, ctx_h, batch_h, device, genes, lengths, out=None, stream=None):
        return windows_into(L, ctx_h, batch_h, device, len(lengths), genes, self, out, stream)

    def __repr__(self):
        return "pyrodigal_amd.GeneWindows(%r, %r, unit=%r, dtype=%r, layout=%r, bos=%r, eos=%r, max_length=%r)" % (
            self.begin, self.end, self.token_unit, self.dtype, self.layout, self.bos, self.eos, self.max_length)

    def lengths(self, genes):
        """Tokens of every gene record's row, specials included (int64): host arithmetic on the coordinates, as the library does it."""
        n = genes["end"].astype(np.int64) - genes["begin"] + 1
        t_lo = np.where(self.begin[0] == "end", n, 0) + self.begin[1]
        t_hi = np.where(self.end[0] == "end", n, 0) + self.end[1]
        r = np.maximum(t_hi - t_lo, 0) // (3 if self.token_unit == "codon" else 1)
        if self.max_length is not None:
            r = np.minimum(r, self.max_length - self.specials)
        return (r + self.specials).astype(np.int64)

    def opts(self, row_width=0, row_stride=0):
        o = self._opts(WindowOpts(), row_width, row_stride)
        o.unit = WINDOW_CODONS if self.token_unit == "codon" else WINDOW_BASES
        o.from_anchor, o.from_delta = _WINDOW_ANCHORS[self.begin[0]], self.begin[1]
        o.to_anchor, o.to_delta = _WINDOW_ANCHORS[self.end[0]], self.end[1]
        o.max_length = 0 if self.max_length is None else self.max_length
        o.ids[:len(self.ids)] = self.ids
        o.bos = TOKEN_NONE if self.bos is None else self.bos
        o.eos = TOKEN_NONE if self.eos is None else self.eos
        return o


class DeviceWindows:
    """Nucleotide windows of gene records as token ids in device memory.  ``tokens``: the tensor (``[G, W]`` padded, 1-D ragged);
    ``lengths``: tokens of every row (numpy int64, host); ``offsets``: ragged only, gene g is ``tokens[offsets[g]:offsets[g + 1]]``;
    ``gene_begin``: the genes of contig i are rows ``gene_begin[i] .. gene_begin[i + 1]`` (``None`` when the records were not in
    contig order); ``windows[i]``: contig i's rows or slice as a view of ``tokens``."""

    def __init__(self, tokens, lengths, offsets, gene_begin, device):
        self.tokens, self.lengths, self.offsets, self.gene_begin, self.device = tokens, lengths, offsets, gene_begin, device

    @property
    def windows(self):
        return _gene_views(self, self.tokens)

    def cu_seqlens(self):
        """The exclusive scan of ``lengths`` as an int32 tensor on the tokens' device (torch)."""
        return _cu_seqlens(self.lengths, self.tokens, self.device)


def windows_into(L, ctx_h, batch_h, device, n_contigs, genes, spec, out=None, stream=None):
    """``pga_gene_windows`` on raw handles (what ``Context.gene_windows`` and the finder's device call share): the windows of
    ``genes`` (GENE_DTYPE records of the resident batch of ``n_contigs`` contigs) into ``out``, or into a new torch tensor."""
    if not isinstance(spec, GeneWindows):
        raise TypeError("the window rule must be a GeneWindows, not %r" % type(spec).__name__)
    genes = np.ascontiguousarray(genes, dtype=GENE_DTYPE)
    n, lens = len(genes), spec.lengths(genes)
    args = (batch_h, n, ctypes.c_void_p(genes.ctypes.data))
    out, off, len_out = _rows_into(L, ctx_h, "pga_gene_windows", args, spec, lens, device, out, stream)
    assert np.array_equal(len_out, lens)
    return DeviceWindows(out, lens, off, _gene_begin(genes, n_contigs), device)


def _gene_windows(self, batch, result_or_genes, spec, out=None, stream=None):
    """The nucleotides of gene records of the resident ``batch``, or of a region around each, as token ids in device memory, one row
    per record in the gene's reading direction (``pga_gene_windows``): nothing of them comes to the host.  ``result_or_genes``: a
    result of ``find_genes`` on the batch, or gene records of one (any subset or order).  ``spec``: a :class:`GeneWindows`.
    ``out``: any object with ``__cuda_array_interface__`` -- 1-D for the ragged layout, ``[G, W]`` with a contiguous last dimension
    for the padded one; ``None``: a torch tensor is allocated on the context's device under torch's current stream.  ``stream``:
    the stream that last used ``out``, as in :class:`DeviceSequences`.  Returns a :class:`DeviceWindows`."""
    genes = getattr(result_or_genes, "genes", result_or_genes)
    return windows_into(self.L, self.h, batch.h, self.device, batch.n, genes, spec, out, stream)


_COUNT_ROWS = {"contig": COUNT_CONTIG, "gene": COUNT_GENE, "contig_genes": COUNT_CONTIG_GENES}
COUNT_MAX_K, COUNT_MAX_BINS = 6, 4096
CODON_BIN_LETTERS = AMINO_ACIDS + "*"                        # the 21 bins of KmerCounts.codon_bins, in order


def kmer_of_code(code, k):
    """The k letters of a code in the public ACGT order, first base most significant."""
    return "".join(WINDOW_LETTERS[(code >> (2 * (k - 1 - j))) & 3] for j in range(k))


def kmer_rc(code, k):
    """The code of the reverse complement of a k-mer's code."""
    rc = 0
    for _ in range(k):
        rc = (rc << 2) | (3 - (code & 3))
        code >>= 2
    return rc


class KmerCounts(_TensorRule):
    """How ``kmer_counts`` / ``find_counts_batch`` count the k-mers of contigs or genes into an ``int32`` device tensor, one row of
    ``n_bins`` counts per contig or per gene (``pga_count_opts``; the rule is in ``pyrodigal_amd.h``).

    ``k``: 1 .. 6.  ``rows``: ``"contig"`` -- every window of the contig's forward strand, across the origin of a circular one;
    ``"gene"`` -- the windows inside every gene, read in the gene's own direction; ``"contig_genes"`` -- one row per contig, the sum
    of its genes' rows.  ``step``: 1, or 3 for gene rows: ``k=3, step=3`` is codon usage, ``k=6, step=3`` in-frame dicodons.  A
    window that holds a letter other than A, C, G, T is not counted.  ``canonical=True`` folds a k-mer with its reverse complement:
    the bin is the rank of ``min(code, rc(code))`` among the canonical codes in ascending order (136 bins for ``k=4``).  ``bins``: a
    table of the caller's instead, ``4^k`` integers indexed by the k-mer's code (ACGT order, first base most significant), ``-1`` =
    not counted.  Everything that needs no device is checked here.  Hashable and picklable."""

    def __init__(self, k=4, *, rows="contig", step=1, canonical=False, bins=None):
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)):
            raise TypeError(f"k must be an integer, not {type(k).__name__}")
        if not 1 <= k <= COUNT_MAX_K:
            raise ValueError(f"k must be 1 .. {COUNT_MAX_K}, not {k}")
        if rows not in _COUNT_ROWS:
            raise ValueError("rows must be \"contig\", \"gene\" or \"contig_genes\", not %r" % (rows,))
        if isinstance(step, bool) or not isinstance(step, (int, np.integer)):
            raise TypeError(f"step must be an integer, not {type(step).__name__}")
        if step not in (1, 3):
            raise ValueError(f"step must be 1 or 3, not {step}")
        if rows == "contig" and step != 1:
            raise ValueError("contig rows count every window: step must be 1 (step = 3 reads a gene's frame)")
        if not isinstance(canonical, (bool, np.bool_)):
            raise TypeError(f"canonical must be a bool, not {type(canonical).__name__}")
        self.k, self.rows, self.step, self.canonical, self.custom = int(k), rows, int(step), bool(canonical), bins is not None
        n_codes = 4 ** self.k
        if bins is not None:
            if canonical:
                raise ValueError("`bins` and `canonical` exclude each other: a table of the caller's says itself what it folds")
            table = list(bins)
            if len(table) != n_codes:
                raise ValueError(f"bins has {len(table)} entries: k = {self.k} has {n_codes} codes")
            table = tuple(_token_id(v, f"the bin of {kmer_of_code(x, self.k)}") for x, v in enumerate(table))
            for x, v in enumerate(table):
                if not -1 <= v < COUNT_MAX_BINS:
                    raise ValueError(f"the bin of {kmer_of_code(x, self.k)}, {v}, lies outside -1 .. {COUNT_MAX_BINS - 1}")
            if max(table) < 0:
                raise ValueError("bins drops every k-mer: there is nothing to count")
        elif canonical:
            rank = {c: r for r, c in enumerate(x for x in range(n_codes) if x <= kmer_rc(x, self.k))}
            table = tuple(rank[min(x, kmer_rc(x, self.k))] for x in range(n_codes))
        else:
            table = tuple(range(n_codes))
        self.table = table
        self.n_bins = max(table) + 1

    row, unit, per_contig = "row", "bins", "lengths"
    dtype, typestr, elem_bytes = "int32", "<i4", 4

    @staticmethod
    def codon_bins(translation_table=11):
        """The table of ``bins=`` that counts amino acids: the 64 codons onto 21 bins in the order ``ACDEFGHIKLMNPQRSTVWY*``, by the
        codon-to-residue map of the translation table -- no initiator rule: a GTG start counts as V."""
        from .tables import NCBI_CODES
        if isinstance(translation_table, bool) or not isinstance(translation_table, (int, np.integer)) or translation_table not in NCBI_CODES:
            raise ValueError("%r is not a valid translation table index" % (translation_table,))
        code, tcag = NCBI_CODES[int(translation_table)], "TCAG"
        at = lambda x: tcag.index(WINDOW_LETTERS[x])
        return tuple(CODON_BIN_LETTERS.index(code[16 * at(a) + 4 * at(b) + at(c)]) for a in range(4) for b in range(4) for c in range(4))

    @property
    def labels(self):
        """The k-mer of every bin, for folded bins the smaller member; ``None`` under a table of the caller's."""
        if self.custom:
            return None
        first = {}
        for x, b in enumerate(self.table):
            first.setdefault(b, x)
        return tuple(kmer_of_code(first[b], self.k) for b in range(self.n_bins))

    _fields = ("k", "rows", "step", "canonical", "custom", "table")

    def _derive(self):
        self.n_bins = max(self.table) + 1

    def write(self, L, ctx_h, batch_h, device, genes, lengths, out=None, stream=None):
        return counts_into(L, ctx_h, batch_h, device, len(lengths), genes, self, out, stream)

    def __repr__(self):
        return "pyrodigal_amd.KmerCounts(%d, rows=%r, step=%d, %s)" % (
            self.k, self.rows, self.step, "bins=<%d codes onto %d bins>" % (len(self.table), self.n_bins) if self.custom else "canonical=%r" % self.canonical)

    def windows(self, genes, lengths, circular=None):
        """The window positions of every row, counted or not (int64): host arithmetic on the lengths and coordinates, as the library
        does it.  ``genes``: GENE_DTYPE records (not read for contig rows); ``lengths``: the bases of every contig as the batch holds
        it; ``circular``: the contigs flagged circular (``None``: none, ``True``: all)."""
        lengths = np.ascontiguousarray(lengths, np.int64)
        k, step = self.k, self.step
        if self.rows == "contig":
            circ = np.zeros(len(lengths), bool) if circular is None or circular is False else np.broadcast_to(np.asarray(circular, bool), lengths.shape)
            return np.where(lengths < k, 0, np.where(circ, lengths, lengths - k + 1)).astype(np.int64)
        n = genes["end"].astype(np.int64) - genes["begin"] + 1
        w = np.where(n >= k, (n - k) // step + 1, 0).astype(np.int64)
        if self.rows == "gene":
            return w
        out = np.zeros(len(lengths), np.int64)
        np.add.at(out, genes["contig"].astype(np.int64), w)
        return out

    def opts(self, row_stride=0):
        o = CountOpts()
        o.rows, o.k, o.step, o.n_bins, o.row_stride = _COUNT_ROWS[self.rows], self.k, self.step, self.n_bins, int(row_stride)
        o._table = np.array(self.table, np.int32)            # (kept alive with the struct)
        o.bin_of_code = o._table.ctypes.data
        return o


class DeviceCounts:
    """K-mer counts of contigs or gene records in device memory.  ``counts``: the tensor, ``[R, n_bins]`` int32 (with ``out=``: the
    caller's ``[R, S]`` object, of which columns ``0 .. n_bins - 1`` were set); ``windows``: the window positions of every row, counted
    or not (numpy int64, host): the denominator of a frequency; ``gene_begin``: for gene rows, the genes of contig i are rows
    ``gene_begin[i] .. gene_begin[i + 1]`` (``None`` when the records were not in contig order, and for rows per contig);
    ``counts_of[i]``: contig i's gene rows, or its own row, as a view of ``counts``."""

    def __init__(self, counts, windows, gene_begin, rows, n_bins, n_contigs, device):
        self.counts, self.windows, self.gene_begin, self.rows, self.n_bins = counts, windows, gene_begin, rows, n_bins
        self.n_contigs, self.device = n_contigs, device

    offsets = None                                           # (the rows are always padded)

    @property
    def counts_of(self):
        if self.rows == "gene":
            return _gene_views(self, self.counts)
        return _ContigViews(lambda i, _: self.counts[i], None, self.n_contigs)


def counts_into(L, ctx_h, batch_h, device, n_contigs, genes, spec, out=None, stream=None):
    """``pga_count_kmers`` on raw handles (what ``Context.kmer_counts`` and the finder's device call share): the counts of the
    contigs of the resident batch, or of ``genes`` (GENE_DTYPE records of it), into ``out`` or into a new torch tensor."""
    if not isinstance(spec, KmerCounts):
        raise TypeError("the counting rule must be a KmerCounts, not %r" % type(spec).__name__)
    genes = np.ascontiguousarray(genes, dtype=GENE_DTYPE)
    n = len(genes)
    R = n if spec.rows == "gene" else n_contigs
    if out is None:
        (out,), stream = _torch_outputs(device, stream, [((R, spec.n_bins), "int32")], "a device array")
    ptr, shape, strides = _device_array(out, "out", spec.typestr, f"the rule writes int32 ({spec.typestr})")
    if len(shape) != 2 or shape[0] != R:
        raise ValueError(f"the counts need a [{R}, S] tensor, not one of shape {shape}")
    if shape[1] < spec.n_bins:
        raise ValueError(f"out has {shape[1]} columns: the rule has {spec.n_bins} bins")
    if shape[1] > 1 and strides[1] != 4:
        raise ValueError("the last dimension of out is not contiguous")
    if R > 1 and (strides[0] % 4 or strides[0] < 4 * shape[1]):
        raise ValueError("the rows of out do not lie a whole number of elements apart, at least a row's width")
    stride = shape[1] if R < 2 else strides[0] // 4
    n_out = (R - 1) * stride + shape[1] if R else 0
    win_out = np.zeros(max(R, 1), np.int64)
    o = spec.opts(stride)
    rc = L.pga_count_kmers(ctx_h, batch_h, n, ctypes.c_void_p(genes.ctypes.data), ctypes.byref(o), ctypes.c_void_p(ptr), n_out,
                           ctypes.c_void_p(DeviceSequences._stream_of(out, stream)), ctypes.c_void_p(win_out.ctypes.data))
    if rc != PGA_OK:
        _raise(L, ctx_h, rc, "pga_count_kmers")
    gene_begin = _gene_begin(genes, n_contigs) if spec.rows == "gene" else None
    return DeviceCounts(out, win_out[:R], gene_begin, spec.rows, spec.n_bins, n_contigs, device)


def _kmer_counts(self, batch, result_or_genes, spec, out=None, stream=None):
    """The k-mers of the contigs of the resident ``batch``, or of gene records on it, counted into an ``int32`` device tensor, one row
    per contig or per record (``pga_count_kmers``): nothing of them comes to the host.  ``result_or_genes``: a result of
    ``find_genes`` on the batch, or gene records of one (any subset or order; ``None`` will do for contig rows).  ``spec``: a
    :class:`KmerCounts`.  ``out``: any 2-D object with ``__cuda_array_interface__``, ``[R, S >= n_bins]`` int32 with a contiguous
    last dimension, of which columns ``0 .. n_bins - 1`` are set; ``None``: a ``[R, n_bins]`` torch tensor is allocated on the
    context's device under torch's current stream.  ``stream``: the stream that last used ``out``, as in :class:`DeviceSequences`.
    Returns a :class:`DeviceCounts`."""
    genes = getattr(result_or_genes, "genes", result_or_genes)
    if genes is None:
        genes = np.zeros(0, GENE_DTYPE)
    return counts_into(self.L, self.h, batch.h, self.device, batch.n, genes, spec, out, stream)


_GROUP_UNITS = {"protein": GROUP_PROTEIN, "gene": GROUP_GENE}
DIGEST_MODULUS = (1 << 61) - 1
DIGEST_BASES = (0x0123456789ABCDEF, 0x1BADB002C0FFEE11)


class ProteinGroups(_TensorRule):
    """How ``protein_groups`` / ``find_groups_batch`` group gene records with the same string (``pga_group_opts``; the rule is in
    ``pyrodigal_amd.h``).

    ``unit``: ``"protein"`` -- the string of a record is its translation, exactly the letters ``translate_genes`` yields under the
    contig's table, ``include_stop``, ``strict`` and ``unknown_residue``; ``"gene"`` -- all bases of the record in reading direction,
    upper case, anything but A, C, G, T as N (the three translation options are not read then).  Two records are in one group exactly
    when their strings are equal byte for byte.  Everything that needs no device is checked here.  Hashable and picklable."""

    def __init__(self, unit="protein", *, include_stop=False, strict=True, unknown_residue="X"):
        if unit not in _GROUP_UNITS:
            raise ValueError("unit must be \"protein\" or \"gene\", not %r" % (unit,))
        for name, v in (("include_stop", include_stop), ("strict", strict)):
            if not isinstance(v, (bool, np.bool_)):
                raise TypeError(f"{name} must be a bool, not {type(v).__name__}")
        if not isinstance(unknown_residue, str):
            raise TypeError(f"unknown_residue must be a str, not {type(unknown_residue).__name__}")
        if len(unknown_residue) != 1 or not 0 < ord(unknown_residue) < 128:
            raise ValueError("unknown_residue must be a single ASCII character, not %r" % (unknown_residue,))
        self.of, self.include_stop, self.strict, self.unknown_residue = unit, bool(include_stop), bool(strict), unknown_residue

    row, unit, per_contig = "gene", "groups", "tables"      # (`of` holds the constructor's unit)
    _fields = ("of", "include_stop", "strict", "unknown_residue")
    dtype, typestr, elem_bytes = "int64", "<i8", 8

    @staticmethod
    def digest_of(letters):
        """The digest of a string (``bytes`` or ASCII ``str``) as the device computes it, in Python integers: a caller can digest a
        protein from anywhere else and look it up among ``DeviceGroups.digests``."""
        if isinstance(letters, str):
            letters = letters.encode("ascii")
        out = []
        for b in DIGEST_BASES:
            h = 1
            for r in bytes(letters):
                h = (h * b + r) % DIGEST_MODULUS
            out.append(h)
        return tuple(out)

    def write(self, L, ctx_h, batch_h, device, genes, tables, out=None, stream=None):
        return groups_into(L, ctx_h, batch_h, device, len(tables), genes, tables, self, out, stream)

    def __repr__(self):
        return "pyrodigal_amd.ProteinGroups(%r, include_stop=%r, strict=%r, unknown_residue=%r)" % self._key()

    def opts(self):
        o = GroupOpts()
        o.unit, o.include_stop, o.strict, o.unknown_residue = _GROUP_UNITS[self.of], int(self.include_stop), int(self.strict), ord(self.unknown_residue)
        return o


class DeviceGroups:
    """Gene records grouped by their string, in device memory, all int64.  ``group``: ``[G]``, the group of every record, numbered in
    order of first appearance; ``representatives``: ``[U]``, the first record of every group; ``sizes``: ``[U]``, its members;
    ``digests``: ``[G, 2]``, the digest of every record's string (``ProteinGroups.digest_of``); ``n_groups``: U (host).
    ``representatives`` and ``sizes`` are the first U elements of capacity-G tensors (``None`` where ``out=`` gave ``None``, as
    ``digests``).  ``gene_begin``: the genes of contig i are records ``gene_begin[i] .. gene_begin[i + 1]`` (``None`` when the
    records were not in contig order)."""

    def __init__(self, group, representatives, sizes, digests, n_groups, gene_begin, device):
        self.group, self.representatives, self.sizes, self.digests = group, representatives, sizes, digests
        self.n_groups, self.gene_begin, self.device = n_groups, gene_begin, device


def _group_output(x, name, shape, required):
    """The device pointer of one int64 output of ``pga_group_proteins`` checked against the shape it needs, 0 for ``None``."""
    if x is None:
        if required:
            raise TypeError(f"out: {name} is required")
        return 0
    ptr, got, strides = _device_array(x, f"out: {name}", "<i8", "these tensors are int64 (<i8)")
    if len(got) != len(shape) or got[1:] != shape[1:] or got[0] < shape[0]:
        raise ValueError(f"out: {name} needs shape {list(shape)}{' or longer' if len(shape) == 1 else ''}, not {list(got)}")
    if int(np.prod(got)) > 1 and strides != _contiguous_strides(got, 8):
        raise ValueError(f"out: {name} is not contiguous")
    return ptr


def groups_into(L, ctx_h, batch_h, device, n_contigs, genes, tables, spec, out=None, stream=None):
    """``pga_group_proteins`` on raw handles (what ``Context.protein_groups`` and the finder's device call share): the groups of
    ``genes`` (GENE_DTYPE records of the resident batch) under ``tables`` into the four tensors of ``out``, or into new torch
    tensors."""
    if not isinstance(spec, ProteinGroups):
        raise TypeError("the grouping rule must be a ProteinGroups, not %r" % type(spec).__name__)
    genes = np.ascontiguousarray(genes, dtype=GENE_DTYPE)
    n = len(genes)
    tables, p_tab = _tables_arg(tables, n_contigs, spec.of)
    if out is None:
        out, stream = _torch_outputs(device, stream, [(n, "int64"), (n, "int64"), (n, "int64"), ((n, 2), "int64")], "four device arrays")
    out = tuple(out)
    if len(out) != 4:
        raise ValueError("out must be (group, representatives, sizes, digests), %d objects were given" % len(out))
    group, reps, sizes, digests = out
    p_group = _group_output(group, "group", (n,), True)
    p_reps, p_sizes = _group_output(reps, "representatives", (n,), False), _group_output(sizes, "sizes", (n,), False)
    p_dig = _group_output(digests, "digests", (n, 2), False)
    capacity = min([_device_array(x, "out")[1][0] for x in (reps, sizes) if x is not None] or [n])
    n_groups = ctypes.c_int64(0)
    o = spec.opts()
    rc = L.pga_group_proteins(ctx_h, batch_h, n, ctypes.c_void_p(genes.ctypes.data), p_tab, ctypes.byref(o), ctypes.c_void_p(p_group),
                              ctypes.c_void_p(p_reps), ctypes.c_void_p(p_sizes), ctypes.c_void_p(p_dig), capacity,
                              ctypes.c_void_p(DeviceSequences._stream_of(group, stream)), ctypes.byref(n_groups))
    if rc != PGA_OK:
        _raise(L, ctx_h, rc, "pga_group_proteins")
    U = int(n_groups.value)
    cut = lambda x: None if x is None else (x[:U] if hasattr(x, "__getitem__") else x)      # noqa: E731
    return DeviceGroups(group, cut(reps), cut(sizes), digests, U, _gene_begin(genes, n_contigs), device)


def _protein_groups(self, batch, result_or_genes, spec, tables=None, out=None, stream=None):
    """Gene records of the resident ``batch`` with the same protein (or the same bases) grouped on the device, exactly
    (``pga_group_proteins``): no letter comes to the host.  ``result_or_genes``: a result of ``find_genes`` on the batch, or gene
    records of one (any subset or order; then with ``tables`` for the protein unit).  ``spec``: a :class:`ProteinGroups`.  ``tables``:
    translation table per contig (default: that of the model that won the contig).  ``out``: a 4-tuple ``(group [G], representatives
    [>= G], sizes [>= G], digests [G, 2])`` of contiguous int64 objects with ``__cuda_array_interface__``, ``None`` allowed for the
    last three; omitted: torch tensors are allocated on the context's device under torch's current stream.  ``stream``: the stream
    that last used the outputs, as in :class:`DeviceSequences`.  Returns a :class:`DeviceGroups`."""
    genes = getattr(result_or_genes, "genes", result_or_genes)
    if isinstance(spec, ProteinGroups) and spec.of == "protein":
        tables = _tables_or_default(self, result_or_genes, tables)
    return groups_into(self.L, self.h, batch.h, self.device, batch.n, genes, tables, spec, out, stream)


def _protein_groups_stats(self):
    """How the context's last ``protein_groups`` call went (``pga_protein_groups_stats``): the verification rounds, and the pairs the
    sort put side by side whose strings differed."""
    out = (ctypes.c_int64 * 2)()
    rc = self.L.pga_protein_groups_stats(self.h, out)
    if rc != PGA_OK:
        _raise(self.L, self.h, rc, "pga_protein_groups_stats")
    return {"rounds": int(out[0]), "differing_pairs": int(out[1])}


_SKETCH_UNITS = {"protein": SKETCH_PROTEIN, "gene": SKETCH_GENE}
SKETCH_NONE = (1 << 63) - 1                                 # what a sketch row holds behind its count
SKETCH_SKIP = 255                                           # the class of a letter that no window may hold
_MASK64 = (1 << 64) - 1
_BASE_CODES = {"A": 0, "C": 1, "G": 2, "T": 3}


def _sketch_classes(classes, unknown_residue):
    """The 128-entry class table of a ``ProteinSketches``, as a tuple."""
    if classes is None:
        table = list(range(128))
        table[ord(unknown_residue)] = SKETCH_SKIP
        return tuple(table)
    if isinstance(classes, (bytes, bytearray)) or (isinstance(classes, (tuple, list, np.ndarray)) and len(classes) == 128
                                                   and not any(isinstance(v, str) for v in classes)):
        table = [int(v) for v in bytes(classes)] if isinstance(classes, (bytes, bytearray)) else [int(v) for v in classes]
        if len(table) != 128:
            raise ValueError(f"classes has {len(table)} entries: a class table has 128")
        if not all(0 <= v <= 255 for v in table):
            raise ValueError("a class is 0 .. 254, or 255 for a letter that is skipped")
        return tuple(table)
    if isinstance(classes, str):
        raise TypeError("classes must be None, 128 bytes or an iterable of strings of letters, not one string")
    table = [SKETCH_SKIP] * 128
    n = 0
    for n, letters in enumerate(classes):
        if not isinstance(letters, str) or not letters:
            raise TypeError("classes: every class is a non-empty string of letters, not %r" % (letters,))
        if n >= SKETCH_SKIP:
            raise ValueError("classes: more than 255 classes")
        for ch in letters:
            if not 0 < ord(ch) < 128:
                raise ValueError(f"classes: {ch!r} is not a 7-bit ASCII character")
            if table[ord(ch)] != SKETCH_SKIP:
                raise ValueError(f"classes: the letter {ch!r} is named twice")
            table[ord(ch)] = n
    return tuple(table)


class ProteinSketches(_TensorRule):
    """How ``protein_sketches`` / ``find_sketches_batch`` sketch the strings of gene records (``pga_sketch_opts``; the rule is in
    ``pyrodigal_amd.h``): the ``size`` smallest distinct hashes of the ``k``-letter windows of every record, a bottom-s MinHash.

    ``unit``: ``"protein"`` -- the string of a record is its translation under the contig's table, ``include_stop``, ``strict`` and
    ``unknown_residue`` (``1 <= k <= 8``); ``"gene"`` -- its bases in reading direction, N skipped (``1 <= k <= 32``; the three
    translation options and ``classes`` are not read).  ``classes``: ``None`` -- every letter is its own class and
    ``unknown_residue`` is skipped; 128 byte values -- the class 0 .. 254 of every letter, 255 to skip it; or an iterable of strings,
    each one class of a reduced alphabet, letters not named being skipped.  ``seed``: a uint32 that picks the hash function.
    Everything that needs no device is checked here.  Hashable and picklable."""

    def __init__(self, k=5, size=32, unit="protein", *, seed=0, classes=None, include_stop=False, strict=True, unknown_residue="X"):
        if unit not in _SKETCH_UNITS:
            raise ValueError("unit must be \"protein\" or \"gene\", not %r" % (unit,))
        for name, v in (("k", k), ("size", size), ("seed", seed)):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"{name} must be an int, not {type(v).__name__}")
        kmax = 8 if unit == "protein" else 32
        if not 1 <= k <= kmax:
            raise ValueError(f"k must be 1 .. {kmax} for the {unit} unit, not {k}")
        if not 1 <= size <= 64:
            raise ValueError(f"size must be 1 .. 64, not {size}")
        if not 0 <= seed < (1 << 32):
            raise ValueError(f"seed must be a uint32, not {seed}")
        for name, v in (("include_stop", include_stop), ("strict", strict)):
            if not isinstance(v, (bool, np.bool_)):
                raise TypeError(f"{name} must be a bool, not {type(v).__name__}")
        if not isinstance(unknown_residue, str):
            raise TypeError(f"unknown_residue must be a str, not {type(unknown_residue).__name__}")
        if len(unknown_residue) != 1 or not 0 < ord(unknown_residue) < 128:
            raise ValueError("unknown_residue must be a single ASCII character, not %r" % (unknown_residue,))
        self.k, self.size, self.of, self.seed = int(k), int(size), unit, int(seed)
        self.classes = _sketch_classes(classes, unknown_residue)
        self.include_stop, self.strict, self.unknown_residue = bool(include_stop), bool(strict), unknown_residue

    row, unit, per_contig = "gene", "sketches", "tables"    # (`of` holds the constructor's unit)
    dtype, typestr, elem_bytes = "int64", "<i8", 8

    def hash_of(self, x):
        """The hash of a window's key ``x`` under the rule's seed, in Python integers."""
        z = (x + (self.seed + 1) * 0x9E3779B97F4A7C15) & _MASK64
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
        return (z ^ (z >> 31)) >> 1

    def sketch_of(self, letters):
        """``(sketch, windows)`` of a string (``bytes`` or ASCII ``str``) as the device computes it, in Python integers: the
        ascending list of its at most ``size`` smallest distinct hashes -- ``len(sketch)`` is the device's count -- and its valid
        windows.  A caller can sketch a protein from anywhere else and compare it with rows of ``DeviceSketches.sketches``."""
        if isinstance(letters, str):
            letters = letters.encode("ascii")
        if self.of == "gene":
            bits, codes = 2, [_BASE_CODES.get(chr(b), SKETCH_SKIP) for b in bytes(letters)]
        else:
            bits, codes = 8, [self.classes[b] if b < 128 else SKETCH_SKIP for b in bytes(letters)]
        hashes, windows = set(), 0
        for j in range(len(codes) - self.k + 1):
            w = codes[j:j + self.k]
            if SKETCH_SKIP in w:
                continue
            x = 0
            for c in w:
                x = (x << bits) | c
            windows += 1
            hashes.add(self.hash_of(x))
        return sorted(hashes)[:self.size], windows

    def shared(self, row_a, row_b):
        """``(shared, m)`` of two sketches (the real entries of two rows): of the ``m = min(size, |union|)`` smallest hashes of their
        union, those that lie in both -- what ``DeviceSketches.compare`` gives.  Resemblance is about ``shared / m``."""
        a, b = set(int(v) for v in row_a), set(int(v) for v in row_b)
        low = sorted(a | b)[:self.size]
        return sum(1 for v in low if v in a and v in b), len(low)

    _fields = ("k", "size", "of", "seed", "classes", "include_stop", "strict", "unknown_residue")

    def write(self, L, ctx_h, batch_h, device, genes, tables, out=None, stream=None):
        return sketches_into(L, ctx_h, batch_h, device, len(tables), genes, tables, self, out, stream)

    def __repr__(self):
        return "pyrodigal_amd.ProteinSketches(%r, %r, %r, seed=%r, include_stop=%r, strict=%r, unknown_residue=%r)" % (
            self.k, self.size, self.of, self.seed, self.include_stop, self.strict, self.unknown_residue)

    def opts(self):
        o = SketchOpts()
        o.unit, o.k, o.size, o.seed = _SKETCH_UNITS[self.of], self.k, self.size, self.seed
        o.include_stop, o.strict, o.unknown_residue = int(self.include_stop), int(self.strict), ord(self.unknown_residue)
        o.classes[:] = self.classes
        return o


class DeviceSketches:
    """The sketches of gene records, in device memory, all int64.  ``sketches``: ``[G, size]``, every row ascending, ``INT64_MAX``
    behind its ``counts[g]`` real entries; ``counts``: ``[G]``; ``windows``: ``[G]``, the valid windows of every record (``None``
    where ``out=`` gave ``None``); ``spec``: the :class:`ProteinSketches`.  ``gene_begin``: the genes of contig i are records
    ``gene_begin[i] .. gene_begin[i + 1]`` (``None`` when the records were not in contig order)."""

    def __init__(self, sketches, counts, windows, gene_begin, spec, device, n, L=None, ctx_h=None):
        self.sketches, self.counts, self.windows, self.gene_begin = sketches, counts, windows, gene_begin
        self.spec, self.device, self.n = spec, device, n
        self._L, self._ctx_h = L, ctx_h

    def compare(self, pairs, out=None, stream=None):
        """``(shared, union)`` of every pair of rows (``pga_sketch_pairs``): ``pairs`` is a contiguous int64 ``[P, 2]`` device
        tensor of record indices; a pair with an index outside ``0 .. G - 1`` gets -1 in both.  ``out``: two contiguous int64
        ``[P]`` objects with ``__cuda_array_interface__``, omitted: torch tensors.  The context of the call that made the sketches
        must still be open."""
        shape = _device_array(pairs, "pairs")[1]
        if len(shape) != 2 or shape[1] != 2:
            raise ValueError(f"pairs needs shape [P, 2], not {list(shape)}")
        P = shape[0]
        p_pairs = _group_output(pairs, "pairs", (P, 2), True)
        if out is None:
            out, stream = _torch_outputs(self.device, stream, [(P, "int64"), (P, "int64")], "two device arrays")
        out = tuple(out)
        if len(out) != 2:
            raise ValueError("out must be (shared, union), %d objects were given" % len(out))
        p_shared, p_union = _group_output(out[0], "shared", (P,), True), _group_output(out[1], "union", (P,), True)
        p_sk = _group_output(self.sketches, "sketches", (self.n, self.spec.size), True)
        p_cnt = _group_output(self.counts, "counts", (self.n,), True)
        rc = self._L.pga_sketch_pairs(self._ctx_h, ctypes.c_void_p(p_sk), ctypes.c_void_p(p_cnt), self.n, self.spec.size, ctypes.c_void_p(p_pairs), P,
                                      ctypes.c_void_p(p_shared), ctypes.c_void_p(p_union), ctypes.c_void_p(DeviceSequences._stream_of(out[0], stream)))
        if rc != PGA_OK:
            _raise(self._L, self._ctx_h, rc, "pga_sketch_pairs")
        return out

    def cluster(self, spec, weights=None, out=None, stream=None):
        """The rows clustered by resemblance (``pga_cluster_sketches``): ``spec`` is a :class:`ProteinClusters` whose ``sketches``
        is the rule these rows were made under.  ``weights``: an int64 ``[G]`` device tensor, the heavier member of a bucket or a
        cluster being its centre or representative; default ``self.windows``, and equal weights where that is ``None``.  ``out``
        and ``stream`` as in :func:`clusters_into`.  The context of the call that made the sketches must still be open.  Returns a
        :class:`DeviceClusters`."""
        if not isinstance(spec, ProteinClusters):
            raise TypeError("the clustering rule must be a ProteinClusters, not %r" % type(spec).__name__)
        if spec.sketches != self.spec:
            raise ValueError("these sketches were made under %r, not under the rule's %r" % (self.spec, spec.sketches))
        return clusters_into(self._L, self._ctx_h, self.device, self.sketches, self.counts, self.windows if weights is None else weights,
                             spec, out, stream, sketches=self)


class ProteinClusters(_TensorRule):
    """How ``DeviceSketches.cluster`` / ``Context.cluster_sketches`` / ``find_clusters_batch`` cluster near-identical proteins from
    their sketches (``pga_cluster_opts``; the rule is in ``pyrodigal_amd.h``): every hash among a row's first ``probes`` entries
    proposes the row against the heaviest row that holds it too, a proposed pair is an edge when ``m >= max(min_union, 1)`` and
    ``shared / m >= min_resemblance`` for the ``(shared, m)`` of ``DeviceSketches.compare``, and the clusters are the connected
    components.  Single linkage chains, so it is meant for high thresholds; a pair whose common hashes all lie beyond the first
    ``probes`` entries of either row is not proposed.

    ``sketches``: the :class:`ProteinSketches` the rows are made under.  ``probes``: 1 .. ``sketches.size``.  ``min_resemblance``:
    a ``(num, den)`` pair of ints with ``1 <= num <= den <= 2**20``, or a ``fractions.Fraction`` -- not a float: the comparison is
    ``shared * den >= num * m`` in integers, so that the result depends on the arguments alone.  ``min_union``: 0 ..
    ``sketches.size``.  Everything that needs no device is checked here.  Hashable and picklable."""

    def __init__(self, sketches=None, probes=8, min_resemblance=(9, 10), min_union=8):
        if sketches is None:
            sketches = ProteinSketches(5, 32)
        if not isinstance(sketches, ProteinSketches):
            raise TypeError("sketches must be a ProteinSketches, not %r" % type(sketches).__name__)
        for name, v in (("probes", probes), ("min_union", min_union)):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"{name} must be an int, not {type(v).__name__}")
        if isinstance(min_resemblance, (float, np.floating)):
            raise TypeError("min_resemblance must be a (num, den) pair of ints or a fractions.Fraction, not a float: the threshold is "
                            "applied as shared * den >= num * m in integers, and a float names no such pair (0.9 is not 9 / 10)")
        if isinstance(min_resemblance, fractions.Fraction):
            min_resemblance = (min_resemblance.numerator, min_resemblance.denominator)
        try:
            num, den = min_resemblance
        except (TypeError, ValueError):
            raise TypeError("min_resemblance must be a (num, den) pair of ints or a fractions.Fraction, not %r" % (min_resemblance,)) from None
        for name, v in (("num", num), ("den", den)):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"min_resemblance: {name} must be an int, not {type(v).__name__}")
        if not 1 <= probes <= sketches.size:
            raise ValueError(f"probes must be 1 .. the sketch size {sketches.size}, not {probes}")
        if not 1 <= num <= den <= (1 << 20):
            raise ValueError(f"min_resemblance must have 1 <= num <= den <= 2**20, not {num} / {den}")
        if not 0 <= min_union <= sketches.size:
            raise ValueError(f"min_union must be 0 .. the sketch size {sketches.size}, not {min_union}")
        self.sketches, self.probes, self.min_resemblance, self.min_union = sketches, int(probes), (int(num), int(den)), int(min_union)

    row, unit = "gene", "clusters"
    per_contig = property(lambda self: self.sketches.per_contig)
    dtype, typestr, elem_bytes = "int64", "<i8", 8
    _fields = ("sketches", "probes", "min_resemblance", "min_union")

    def write(self, L, ctx_h, batch_h, device, genes, tables, out=None, stream=None):
        # (the finder's call: the sketches into new tensors, the clusters into `out`)
        sk = sketches_into(L, ctx_h, batch_h, device, len(tables), genes, tables, self.sketches, None, stream)
        return sk.cluster(self, None, out, stream)

    def __repr__(self):
        return "pyrodigal_amd.ProteinClusters(%r, probes=%r, min_resemblance=%r, min_union=%r)" % self._key()

    def opts(self):
        o = ClusterOpts()
        o.size, o.probes, o.min_union = self.sketches.size, self.probes, self.min_union
        o.num, o.den = self.min_resemblance
        return o


class DeviceClusters:
    """Sketch rows clustered by resemblance, in device memory, all int64.  ``cluster``: ``[G]``, the cluster of every row, numbered
    in increasing order of the clusters' smallest members; ``representatives``: ``[U]``, the heaviest row of every cluster (the
    smallest index on a tie); ``sizes``: ``[U]``, its members; ``edges``: ``[E, 2]``, the accepted pairs ``(a, b)``, ``a < b``, in
    ascending order, with ``edge_shared`` and ``edge_union`` ``[E]``, their ``(shared, m)`` -- for a caller's own linkage.
    ``n_clusters``: U; ``n_edges``: the true number of edges, of which the first ``min(n_edges, capacity of out=)`` were written.
    Tensors for which ``out=`` gave ``None`` are ``None``.  ``spec``: the :class:`ProteinClusters`; ``sketches``: the
    :class:`DeviceSketches` that were clustered (``None`` for tensors given to ``Context.cluster_sketches``)."""

    def __init__(self, cluster, representatives, sizes, n_clusters, edges, edge_shared, edge_union, n_edges, spec, sketches, device,
                 L=None, ctx_h=None):
        self.cluster, self.representatives, self.sizes, self.n_clusters = cluster, representatives, sizes, n_clusters
        self.edges, self.edge_shared, self.edge_union, self.n_edges = edges, edge_shared, edge_union, n_edges
        self.spec, self.sketches, self.device = spec, sketches, device
        self._L, self._ctx_h = L, ctx_h

    def relink(self, keep=None, weights=None, out=None, stream=None):
        """The components of the rows under the ``edges`` that ``keep`` names (``pga_cluster_edges``): ``keep`` is an int64 ``[E]``
        device tensor, nonzero where the edge is used -- the ``passed`` of ``DeviceProteins.align(self.edges, ...)``, say -- or
        ``None`` for all of them.  ``weights`` defaults as in ``DeviceSketches.cluster``: the ``windows`` of the sketches that were
        clustered, and equal weights where there are none.  ``out``: ``(cluster [G], representatives [>= G], sizes [>= G])``,
        ``None`` allowed for the last two; omitted: torch tensors.  Returns ``(cluster, representatives, sizes, n_clusters,
        n_used)``.  The context of the call that made the clusters must still be open."""
        if self._L is None:
            raise ValueError("this DeviceClusters names no context: use Context.cluster_edges")
        if self.edges is None:
            raise ValueError("this DeviceClusters has no edges: out= left them out")
        if weights is None and self.sketches is not None:
            weights = self.sketches.windows
        n = _device_array(self.cluster, "cluster")[1][0]
        return edges_into(self._L, self._ctx_h, self.device, self.edges, n, keep, weights, out, stream)


def clusters_into(L, ctx_h, device, sketch, count, weight, spec, out=None, stream=None, sketches=None):
    """``pga_cluster_sketches`` on raw handles (what ``DeviceSketches.cluster`` and ``Context.cluster_sketches`` share): int64
    device tensors ``sketch [G, size]``, ``count [G]`` and ``weight [G]`` or ``None`` under ``spec`` into the six tensors of
    ``out`` -- ``(cluster [G], representatives [>= G], sizes [>= G], edges [C, 2], edge_shared [C], edge_union [C])``, contiguous
    int64 objects with ``__cuda_array_interface__``, ``None`` allowed for the second and third and for the last three together --
    or into new torch tensors, the edge tensors with room for all ``G * probes`` candidates.  ``stream``: the stream that last
    used the tensors, as in :class:`DeviceSequences`."""
    if not isinstance(spec, ProteinClusters):
        raise TypeError("the clustering rule must be a ProteinClusters, not %r" % type(spec).__name__)
    shape = _device_array(sketch, "sketches")[1]
    if len(shape) != 2 or shape[1] != spec.sketches.size:
        raise ValueError(f"sketches needs shape [G, {spec.sketches.size}], not {list(shape)}")
    n = shape[0]
    p_sk, p_cnt = _group_output(sketch, "sketches", (n, spec.sketches.size), True), _group_output(count, "counts", (n,), True)
    p_w = _group_output(weight, "weights", (n,), False)
    if out is None:
        C = n * spec.probes
        out, stream = _torch_outputs(device, stream, [(n, "int64"), (n, "int64"), (n, "int64"), ((C, 2), "int64"), (C, "int64"), (C, "int64")],
                                     "six device arrays")
    out = tuple(out)
    if len(out) != 6:
        raise ValueError("out must be (cluster, representatives, sizes, edges, edge_shared, edge_union), %d objects were given" % len(out))
    cluster, reps, sizes, edges, eshared, eunion = out
    p_cluster = _group_output(cluster, "cluster", (n,), True)
    p_reps, p_sizes = _group_output(reps, "representatives", (n,), False), _group_output(sizes, "sizes", (n,), False)
    capacity = min([_device_array(x, "out")[1][0] for x in (reps, sizes) if x is not None] or [n])
    given = [x is not None for x in (edges, eshared, eunion)]
    if any(given) and not all(given):
        raise ValueError("out: edges, edge_shared and edge_union are given all three or not at all")
    edge_capacity, p_edges, p_eshared, p_eunion = 0, 0, 0, 0
    if all(given):
        eshape = _device_array(edges, "out: edges")[1]
        if len(eshape) != 2 or eshape[1] != 2:
            raise ValueError(f"out: edges needs shape [C, 2], not {list(eshape)}")
        edge_capacity = min(eshape[0], _device_array(eshared, "out: edge_shared")[1][0], _device_array(eunion, "out: edge_union")[1][0])
        p_edges = _group_output(edges, "edges", (edge_capacity, 2), True)
        p_eshared, p_eunion = _group_output(eshared, "edge_shared", (edge_capacity,), True), _group_output(eunion, "edge_union", (edge_capacity,), True)
    n_clusters, n_edges = ctypes.c_int64(0), ctypes.c_int64(0)
    o = spec.opts()
    rc = L.pga_cluster_sketches(ctx_h, ctypes.c_void_p(p_sk), ctypes.c_void_p(p_cnt), ctypes.c_void_p(p_w), n, ctypes.byref(o),
                                ctypes.c_void_p(p_cluster), ctypes.c_void_p(p_reps), ctypes.c_void_p(p_sizes), capacity,
                                ctypes.c_void_p(p_edges), ctypes.c_void_p(p_eshared), ctypes.c_void_p(p_eunion), edge_capacity,
                                ctypes.c_void_p(DeviceSequences._stream_of(cluster, stream)), ctypes.byref(n_clusters), ctypes.byref(n_edges))
    if rc != PGA_OK:
        _raise(L, ctx_h, rc, "pga_cluster_sketches")
    U, E = int(n_clusters.value), int(n_edges.value)
    cut = lambda x, k: None if x is None else (x[:k] if hasattr(x, "__getitem__") else x)      # noqa: E731
    W = min(E, edge_capacity)
    return DeviceClusters(cluster, cut(reps, U), cut(sizes, U), U, cut(edges, W), cut(eshared, W), cut(eunion, W), E, spec, sketches, device,
                          L, ctx_h)


def _cluster_sketches(self, sketches, counts, spec, weights=None, out=None, stream=None):
    """Sketch rows from anywhere -- the ``torch.cat`` of several calls' ``DeviceSketches.sketches`` and ``counts``, say -- clustered
    on the device (``pga_cluster_sketches``).  ``sketches`` ``[G, spec.sketches.size]`` and ``counts`` ``[G]``: contiguous int64
    device tensors; ``weights``: one more ``[G]``, or ``None`` for equal weights.  ``out`` and ``stream`` as in
    :func:`clusters_into`.  Returns a :class:`DeviceClusters`."""
    return clusters_into(self.L, self.h, self.device, sketches, counts, weights, spec, out, stream)


def _cluster_stats(self):
    """How the context's last ``cluster_sketches`` call went (``pga_cluster_stats``): the probes, the distinct candidate pairs, the
    edges and the clusters."""
    out = (ctypes.c_int64 * 4)()
    rc = self.L.pga_cluster_stats(self.h, out)
    if rc != PGA_OK:
        _raise(self.L, self.h, rc, "pga_cluster_stats")
    return {"probes": int(out[0]), "candidates": int(out[1]), "edges": int(out[2]), "clusters": int(out[3])}


class ProteinAlignments(_TensorRule):
    """How ``DeviceProteins.align`` / ``Context.align_pairs`` / ``find_verified_clusters_batch`` check a pair of token rows against
    each other (``pga_align_opts``; the rule is in ``pyrodigal_amd.h``): the unit-cost edit distance of the two rows, exact up to
    ``max_distance`` and ``max_distance + 1`` beyond it, and a pair passes when the distance is at most ``max_distance`` and the
    identity over the longer row, ``1 - distance / longer``, is at least ``min_identity``.

    ``max_distance``: 0 .. 255.  ``min_identity``: a ``(num, den)`` pair of ints with ``1 <= num <= den <= 2**20``, or a
    ``fractions.Fraction`` -- not a float: the comparison is ``distance * den <= (den - num) * longer`` in integers, so that the
    result depends on the arguments alone.  Everything that needs no device is checked here.  Hashable and picklable."""

    def __init__(self, max_distance=32, min_identity=(9, 10)):
        if isinstance(max_distance, (bool, np.bool_)) or not isinstance(max_distance, (int, np.integer)):
            raise TypeError(f"max_distance must be an int, not {type(max_distance).__name__}")
        if isinstance(min_identity, (float, np.floating)):
            raise TypeError("min_identity must be a (num, den) pair of ints or a fractions.Fraction, not a float: the threshold is "
                            "applied as distance * den <= (den - num) * longer in integers, and a float names no such pair (0.9 is not 9 / 10)")
        if isinstance(min_identity, fractions.Fraction):
            min_identity = (min_identity.numerator, min_identity.denominator)
        try:
            num, den = min_identity
        except (TypeError, ValueError):
            raise TypeError("min_identity must be a (num, den) pair of ints or a fractions.Fraction, not %r" % (min_identity,)) from None
        for name, v in (("num", num), ("den", den)):
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"min_identity: {name} must be an int, not {type(v).__name__}")
        if not 0 <= max_distance <= 255:
            raise ValueError(f"max_distance must be 0 .. 255, not {max_distance}")
        if not 1 <= num <= den <= (1 << 20):
            raise ValueError(f"min_identity must have 1 <= num <= den <= 2**20, not {num} / {den}")
        self.max_distance, self.min_identity = int(max_distance), (int(num), int(den))

    row, unit = "pair", "distances"
    dtype, typestr, elem_bytes = "int64", "<i8", 8
    _fields = ("max_distance", "min_identity")

    def __repr__(self):
        return "pyrodigal_amd.ProteinAlignments(max_distance=%r, min_identity=%r)" % self._key()

    def opts(self, elem_bytes):
        o = AlignOpts()
        o.elem_bytes, o.max_distance = int(elem_bytes), self.max_distance
        o.num, o.den = self.min_identity
        return o


def _host_rows(values, name):
    """``row_begin`` / ``row_len`` as a contiguous int64 array: an integer numpy array as it is, anything else through ``_host_ints``."""
    if isinstance(values, np.ndarray) and values.dtype.kind in "iu" and values.ndim == 1:
        return np.ascontiguousarray(values, np.int64)
    return _host_ints(values, name)


def align_into(L, ctx_h, device, tokens, row_begin, row_len, pairs, spec, out=None, stream=None):
    """``pga_align_pairs`` on raw handles (what ``DeviceProteins.align`` and ``Context.align_pairs`` share): ``tokens`` is a device
    tensor of uint8, int32 or int64 elements with a contiguous last dimension, row g its elements ``row_begin[g] .. row_begin[g] +
    row_len[g]`` (host integers, counted from the tensor's first element), ``pairs`` a contiguous int64 ``[P, 2]`` device tensor.
    ``out``: ``(distance [P], passed [P])``, contiguous int64 objects with ``__cuda_array_interface__``, ``None`` allowed for the
    second; omitted: torch tensors.  Returns ``(distance, passed)``."""
    if not isinstance(spec, ProteinAlignments):
        raise TypeError("the alignment rule must be a ProteinAlignments, not %r" % type(spec).__name__)
    p_tok, tshape, tstrides = _device_array(tokens, "tokens")
    typestr = str(tokens.__cuda_array_interface__["typestr"])
    if typestr not in _DEVICE_DTYPES:
        raise TypeError(f"tokens has dtype {typestr}: the rows are uint8, int32 or int64 elements")
    eb = _DEVICE_DTYPES[typestr]
    if any(st < 0 or st % eb for st in tstrides) or (tshape and tshape[-1] > 1 and tstrides[-1] != eb):
        raise ValueError("tokens needs a contiguous last dimension and rows a whole, positive number of elements apart")
    n_elems = 0 if not tshape or 0 in tshape else 1 + sum((n - 1) * (st // eb) for n, st in zip(tshape, tstrides))
    begin, lens = _host_rows(row_begin, "row_begin"), _host_rows(row_len, "row_len")
    if len(begin) != len(lens):
        raise ValueError(f"row_begin has {len(begin)} entries and row_len {len(lens)}")
    shape = _device_array(pairs, "pairs")[1]
    if len(shape) != 2 or shape[1] != 2:
        raise ValueError(f"pairs needs shape [P, 2], not {list(shape)}")
    P = shape[0]
    p_pairs = _group_output(pairs, "pairs", (P, 2), True)
    if out is None:
        out, stream = _torch_outputs(device, stream, [(P, "int64"), (P, "int64")], "two device arrays")
    out = tuple(out)
    if len(out) != 2:
        raise ValueError("out must be (distance, passed), %d objects were given" % len(out))
    p_dist, p_pass = _group_output(out[0], "distance", (P,), True), _group_output(out[1], "passed", (P,), False)
    o = spec.opts(eb)
    rc = L.pga_align_pairs(ctx_h, ctypes.c_void_p(p_tok), n_elems, ctypes.c_void_p(begin.ctypes.data), ctypes.c_void_p(lens.ctypes.data), len(lens),
                           ctypes.c_void_p(p_pairs), P, ctypes.byref(o), ctypes.c_void_p(p_dist), ctypes.c_void_p(p_pass),
                           ctypes.c_void_p(DeviceSequences._stream_of(out[0], stream)))
    if rc != PGA_OK:
        _raise(L, ctx_h, rc, "pga_align_pairs")
    return out


def _align_pairs(self, tokens, row_begin, row_len, pairs, spec, out=None, stream=None):
    """Rows of tokens from anywhere -- the ``torch.cat`` of several calls' ``DeviceProteins.tokens``, the tokens of
    ``gene_windows`` -- compared pair by pair on the device (``pga_align_pairs``).  ``tokens``: a device tensor of uint8, int32 or
    int64 elements; ``row_begin`` and ``row_len``: host integers, row g being elements ``row_begin[g] .. row_begin[g] + row_len[g]``
    of it; ``pairs``: a contiguous int64 ``[P, 2]`` device tensor; ``spec``: a :class:`ProteinAlignments`.  ``out`` and ``stream``
    as in :func:`align_into`.  Returns ``(distance, passed)``."""
    return align_into(self.L, self.h, self.device, tokens, row_begin, row_len, pairs, spec, out, stream)


def _align_stats(self):
    """How the context's last ``align_pairs`` call went (``pga_align_stats``): the pairs, those decided without a DP (an index out
    of range, a pair of a row with itself, lengths further apart than ``max_distance``), those that ran the DP, and those that passed."""
    out = (ctypes.c_int64 * 4)()
    rc = self.L.pga_align_stats(self.h, out)
    if rc != PGA_OK:
        _raise(self.L, self.h, rc, "pga_align_stats")
    return {"pairs": int(out[0]), "decided": int(out[1]), "aligned": int(out[2]), "passed": int(out[3])}


def edges_into(L, ctx_h, device, edges, n, keep=None, weights=None, out=None, stream=None):
    """``pga_cluster_edges`` on raw handles (what ``DeviceClusters.relink`` and ``Context.cluster_edges`` share): the components of
    the records ``0 .. n - 1`` under the int64 ``[E, 2]`` device tensor ``edges``, of which ``keep`` (int64 ``[E]``, or ``None``:
    all) names the ones to use; ``weights``: int64 ``[n]`` or ``None``.  ``out``: ``(cluster [n], representatives [>= n], sizes
    [>= n])``, ``None`` allowed for the last two; omitted: torch tensors.  Returns ``(cluster, representatives, sizes, n_clusters,
    n_used)``, the second and third cut to the clusters."""
    if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)):
        raise TypeError(f"n must be an int, not {type(n).__name__}")
    n = int(n)
    if n < 0:
        raise ValueError(f"n must not be negative: {n}")
    shape = _device_array(edges, "edges")[1]
    if len(shape) != 2 or shape[1] != 2:
        raise ValueError(f"edges needs shape [E, 2], not {list(shape)}")
    E = shape[0]
    p_edges = _group_output(edges, "edges", (E, 2), True)
    p_keep, p_w = _group_output(keep, "keep", (E,), False), _group_output(weights, "weights", (n,), False)
    if out is None:
        out, stream = _torch_outputs(device, stream, [(n, "int64"), (n, "int64"), (n, "int64")], "three device arrays")
    out = tuple(out)
    if len(out) != 3:
        raise ValueError("out must be (cluster, representatives, sizes), %d objects were given" % len(out))
    cluster, reps, sizes = out
    p_cluster = _group_output(cluster, "cluster", (n,), True)
    p_reps, p_sizes = _group_output(reps, "representatives", (n,), False), _group_output(sizes, "sizes", (n,), False)
    capacity = min([_device_array(x, "out")[1][0] for x in (reps, sizes) if x is not None] or [n])
    n_clusters, n_used = ctypes.c_int64(0), ctypes.c_int64(0)
    rc = L.pga_cluster_edges(ctx_h, ctypes.c_void_p(p_edges), ctypes.c_void_p(p_keep), E, n, ctypes.c_void_p(p_w), ctypes.c_void_p(p_cluster),
                             ctypes.c_void_p(p_reps), ctypes.c_void_p(p_sizes), capacity,
                             ctypes.c_void_p(DeviceSequences._stream_of(cluster, stream)), ctypes.byref(n_clusters), ctypes.byref(n_used))
    if rc != PGA_OK:
        _raise(L, ctx_h, rc, "pga_cluster_edges")
    U = int(n_clusters.value)
    cut = lambda x: None if x is None else (x[:U] if hasattr(x, "__getitem__") else x)      # noqa: E731
    return cluster, cut(reps), cut(sizes), U, int(n_used.value)


def _cluster_edges(self, edges, n, keep=None, weights=None, out=None, stream=None):
    """The connected components of the records ``0 .. n - 1`` under an edge list of the caller's, on the device
    (``pga_cluster_edges``): numbering, representatives and sizes as ``cluster_sketches`` gives them.  ``edges``: a contiguous int64
    ``[E, 2]`` device tensor; ``keep``: int64 ``[E]``, nonzero where the edge is used, ``None``: all; ``weights``: int64 ``[n]`` or
    ``None``.  An edge with an index outside ``0 .. n - 1`` is ignored.  ``out`` and ``stream`` as in :func:`edges_into`.  Returns
    ``(cluster, representatives, sizes, n_clusters, n_used)``."""
    return edges_into(self.L, self.h, self.device, edges, n, keep, weights, out, stream)


class VerifiedClusters(_TensorRule):
    """How ``find_verified_clusters_batch`` clusters near-identical proteins and checks every edge against the proteins themselves:
    ``clusters`` (a :class:`ProteinClusters` over the protein unit) proposes and accepts pairs from the sketches, ``alignments`` (a
    :class:`ProteinAlignments`) decides each accepted pair by the edit distance of the two proteins' tokens under ``tokens`` (a
    :class:`ProteinTokens`; default: the 20 amino acids and X as uint8, ragged), and the clusters are the components of the pairs
    that passed.  Hashable and picklable."""

    def __init__(self, clusters=None, alignments=None, tokens=None):
        clusters = ProteinClusters() if clusters is None else clusters
        alignments = ProteinAlignments() if alignments is None else alignments
        tokens = ProteinTokens(AMINO_ACIDS + "X", dtype="uint8", layout="ragged") if tokens is None else tokens
        for name, v, cls in (("clusters", clusters, ProteinClusters), ("alignments", alignments, ProteinAlignments), ("tokens", tokens, ProteinTokens)):
            if not isinstance(v, cls):
                raise TypeError("%s must be a %s, not %r" % (name, cls.__name__, type(v).__name__))
        if clusters.sketches.of != "protein":
            raise ValueError("clusters.sketches sketches the %r unit: the edges are verified on the proteins' tokens, so the sketches must "
                             "be those of the proteins (unit=\"protein\")" % (clusters.sketches.of,))
        self.clusters, self.alignments, self.tokens = clusters, alignments, tokens

    row, unit, per_contig = "gene", "clusters", "tables"
    dtype, typestr, elem_bytes = "int64", "<i8", 8
    _fields = ("clusters", "alignments", "tokens")

    def write(self, L, ctx_h, batch_h, device, genes, tables, out=None, stream=None):
        # (the finder's call: tokens, sketches, candidate clusters and distances into new tensors, the verified clusters into `out`)
        proteins = tokens_into(L, ctx_h, batch_h, device, len(tables), genes, tables, self.tokens, None, stream)
        sk = sketches_into(L, ctx_h, batch_h, device, len(tables), genes, tables, self.clusters.sketches, None, stream)
        cand = sk.cluster(self.clusters, None, None, stream)
        distance, passed = proteins.align(cand.edges, self.alignments, None, stream)
        cluster, reps, sizes, U, used = cand.relink(passed, None, out, stream)
        return DeviceVerifiedClusters(cluster, reps, sizes, U, distance, passed, used, cand, proteins, self)

    def __repr__(self):
        return "pyrodigal_amd.VerifiedClusters(%r, %r, %r)" % self._key()


class DeviceVerifiedClusters:
    """Clusters of proteins whose every edge was verified by edit distance, in device memory, all int64.  ``cluster`` ``[G]``,
    ``representatives`` ``[U]``, ``sizes`` ``[U]`` and ``n_clusters`` as in :class:`DeviceClusters`, over the edges that passed;
    ``edge_distance`` and ``edge_passed``: ``[E]``, the distance and the verdict of every edge of ``candidates.edges``;
    ``n_passed``: how many passed.  ``candidates``: the :class:`DeviceClusters` of the sketch stage, with its ``edges``;
    ``proteins``: the :class:`DeviceProteins` that were aligned; ``spec``: the :class:`VerifiedClusters`."""

    def __init__(self, cluster, representatives, sizes, n_clusters, edge_distance, edge_passed, n_passed, candidates, proteins, spec):
        self.cluster, self.representatives, self.sizes, self.n_clusters = cluster, representatives, sizes, n_clusters
        self.edge_distance, self.edge_passed, self.n_passed = edge_distance, edge_passed, n_passed
        self.candidates, self.proteins, self.spec = candidates, proteins, spec



def sketches_into(L, ctx_h, batch_h, device, n_contigs, genes, tables, spec, out=None, stream=None):
    """``pga_sketch_proteins`` on raw handles (what ``Context.protein_sketches`` and the finder's device call share): the sketches of
    ``genes`` (GENE_DTYPE records of the resident batch) under ``tables`` into the three tensors of ``out``, or into new torch
    tensors."""
    if not isinstance(spec, ProteinSketches):
        raise TypeError("the sketching rule must be a ProteinSketches, not %r" % type(spec).__name__)
    genes = np.ascontiguousarray(genes, dtype=GENE_DTYPE)
    n = len(genes)
    tables, p_tab = _tables_arg(tables, n_contigs, spec.of)
    s = spec.size
    if out is None:
        out, stream = _torch_outputs(device, stream, [((n, s), "int64"), (n, "int64"), (n, "int64")], "three device arrays")
    out = tuple(out)
    if len(out) != 3:
        raise ValueError("out must be (sketches, counts, windows), %d objects were given" % len(out))
    sketches, counts, windows = out
    p_sk, p_cnt = _group_output(sketches, "sketches", (n, s), True), _group_output(counts, "counts", (n,), True)
    p_win = _group_output(windows, "windows", (n,), False)
    o = spec.opts()
    rc = L.pga_sketch_proteins(ctx_h, batch_h, n, ctypes.c_void_p(genes.ctypes.data), p_tab, ctypes.byref(o), ctypes.c_void_p(p_sk),
                               ctypes.c_void_p(p_cnt), ctypes.c_void_p(p_win), ctypes.c_void_p(DeviceSequences._stream_of(sketches, stream)))
    if rc != PGA_OK:
        _raise(L, ctx_h, rc, "pga_sketch_proteins")
    return DeviceSketches(sketches, counts, windows, _gene_begin(genes, n_contigs), spec, device, n, L, ctx_h)


def _protein_sketches(self, batch, result_or_genes, spec, tables=None, out=None, stream=None):
    """Bottom-s MinHash sketches of gene records of the resident ``batch``, on the device (``pga_sketch_proteins``): no letter comes
    to the host.  ``result_or_genes``: a result of ``find_genes`` on the batch, or gene records of one (any subset or order -- the
    representatives of ``protein_groups``, say; then with ``tables`` for the protein unit).  ``spec``: a :class:`ProteinSketches`.
    ``tables``: translation table per contig (default: that of the model that won the contig).  ``out``: a 3-tuple ``(sketches
    [G, size], counts [G], windows [G])`` of contiguous int64 objects with ``__cuda_array_interface__``, ``None`` allowed for the
    last; omitted: torch tensors are allocated on the context's device under torch's current stream.  ``stream``: the stream that
    last used the outputs, as in :class:`DeviceSequences`.  Returns a :class:`DeviceSketches`."""
    genes = getattr(result_or_genes, "genes", result_or_genes)
    if isinstance(spec, ProteinSketches) and spec.of == "protein":
        tables = _tables_or_default(self, result_or_genes, tables)
    return sketches_into(self.L, self.h, batch.h, self.device, batch.n, genes, tables, spec, out, stream)


def _protein_sketch_passes(self):
    """The hashes that passed their record's threshold in the context's last ``protein_sketches`` call (``pga_sketch_passes``), -1
    unless the library was built with ``-DPGA_SKETCH_COUNT_PASSES``."""
    out = ctypes.c_int64(0)
    rc = self.L.pga_sketch_passes(self.h, ctypes.byref(out))
    if rc != PGA_OK:
        _raise(self.L, self.h, rc, "pga_sketch_passes")
    return int(out.value)


START_FIELDS = ("total", "cscore", "sscore", "rscore", "uscore", "tscore", "gc_cont")      # PGA_START_* order
START_TYPES = ("ATG", "GTG", "TTG", "Edge")                                                # the codes of DeviceStarts.types
_START_INDEX_DTYPES = {"int32": (4, "<i4"), "int64": (8, "<i8")}
_START_SCORE_DTYPES = {"float32": (4, "<f4"), "float64": (8, "<f8")}
_NO_START_CANDIDATES = ("start candidates are not available for circular sequences or with trim_terminal_repeats: the nodes of a "
                        "circle live in the coordinates of the rotated sequence, as for write_scores (-s cannot be combined with "
                        "--circular either: the start file is not written for circular sequences)")


class StartCandidates(_TensorRule):
    """How ``start_candidates`` / ``find_starts_batch`` write every candidate start site of a gene's ORF into three device tensors
    (``pga_start_opts``; the rule is in ``pyrodigal_amd.h``): ``positions``, ``types`` (0 ATG, 1 GTG, 2 TTG, 3 Edge) and ``scores``,
    one candidate after the other in the gene's reading direction, outermost first.

    ``fields``: the score columns, in order, out of ``total`` (``cscore + sscore``), ``cscore``, ``sscore``, ``rscore``, ``uscore``,
    ``tscore`` and ``gc_cont``; none twice.  ``dtype``: ``"float32"`` or ``"float64"``, the scores; ``index_dtype``: ``"int32"`` or
    ``"int64"``, positions and types.  ``layout``: ``"ragged"`` (``[T]``, ``[T]``, ``[T, F]``) or ``"padded"`` (``[G, W]``, ``[G, W]``,
    ``[G, W, F]``), which needs ``pad`` (positions and types behind a row's candidates) and ``score_pad`` (the scores there; NaN is
    fine).  Everything that needs no device is checked here.  Hashable and picklable."""

    def __init__(self, fields=START_FIELDS, *, dtype="float32", index_dtype="int64", layout="ragged", pad=None, score_pad=None):
        if isinstance(fields, str):
            fields = (fields,)
        fields = tuple(fields)
        if not 1 <= len(fields) <= len(START_FIELDS):
            raise ValueError(f"fields names {len(fields)} columns: 1 to {len(START_FIELDS)} are possible")
        for k, f in enumerate(fields):
            if f not in START_FIELDS:
                raise ValueError("field %r is not one of %s" % (f, ", ".join(START_FIELDS)))
            if f in fields[:k]:
                raise ValueError(f"field {f!r} occurs twice")
        dtype = dtype if isinstance(dtype, str) else np.dtype(dtype).name
        index_dtype = index_dtype if isinstance(index_dtype, str) else np.dtype(index_dtype).name
        if dtype not in _START_SCORE_DTYPES:
            raise ValueError(f"dtype must be float32 or float64, not {dtype!r}")
        if index_dtype not in _START_INDEX_DTYPES:
            raise ValueError(f"index_dtype must be int32 or int64, not {index_dtype!r}")
        if layout not in ("padded", "ragged"):
            raise ValueError(f"layout must be \"padded\" or \"ragged\", not {layout!r}")
        if layout == "padded" and (pad is None or score_pad is None):
            raise ValueError("the padded layout needs `pad` and `score_pad`, what fills the rows behind their candidates")
        pad = 0 if pad is None else _token_id(pad, "pad")
        if isinstance(score_pad, bool) or not (score_pad is None or isinstance(score_pad, (int, float, np.integer, np.floating))):
            raise TypeError(f"score_pad must be a number, not {type(score_pad).__name__}")
        score_pad = 0.0 if score_pad is None else float(score_pad)
        if index_dtype == "int32" and not -(1 << 31) <= pad < (1 << 31):
            raise ValueError(f"pad, {pad}, does not fit int32")
        if not -(1 << 63) <= pad < (1 << 63):
            raise ValueError(f"pad, {pad}, does not fit int64")
        if dtype == "float32" and np.isfinite(score_pad) and abs(score_pad) > float(np.finfo(np.float32).max):
            raise ValueError(f"score_pad, {score_pad}, does not fit float32")
        self.fields, self.dtype, self.index_dtype, self.layout, self.pad, self.score_pad = fields, dtype, index_dtype, layout, pad, score_pad

    row, unit, per_contig = "gene", "candidates", "lengths"
    needs_nodes = True                       # the finder keeps the node arena on the device for this rule (PGA_NODES_DEVICE)
    score_bytes = property(lambda self: _START_SCORE_DTYPES[self.dtype][0])
    index_bytes = property(lambda self: _START_INDEX_DTYPES[self.index_dtype][0])
    score_typestr = property(lambda self: _START_SCORE_DTYPES[self.dtype][1])
    index_typestr = property(lambda self: _START_INDEX_DTYPES[self.index_dtype][1])

    def write(self, L, ctx_h, batch_h, device, genes, lengths, out=None, stream=None):
        # (the finder's call: its context goes back to the pool when the request returns, so nothing of it may stay with the result)
        return starts_into(L, ctx_h, batch_h, device, len(lengths), genes, self, out, stream, keep_plan=False)

    _fields = ("fields", "dtype", "index_dtype", "layout", "pad", "score_pad")

    def _key(self):
        # (NaN is a legitimate score_pad and is not equal to itself: the key holds its bits)
        return _TensorRule._key(self)[:-1] + (np.float64(self.score_pad).tobytes(),)

    def _derive(self):
        self.score_pad = float(np.frombuffer(self.score_pad, np.float64)[0])

    def __repr__(self):
        return "pyrodigal_amd.StartCandidates(%r, dtype=%r, index_dtype=%r, layout=%r, pad=%r, score_pad=%r)" % (
            self.fields, self.dtype, self.index_dtype, self.layout, self.pad, self.score_pad)

    def opts(self, row_width=0, row_stride=0):
        o = StartOpts()
        o.index_bytes, o.score_bytes = self.index_bytes, self.score_bytes
        o.layout = TOKENS_PADDED if self.layout == "padded" else TOKENS_RAGGED
        o.n_fields, o.row_width, o.row_stride = len(self.fields), int(row_width), int(row_stride)
        for k, f in enumerate(self.fields):
            o.fields[k] = START_FIELDS.index(f)
        o.index_pad, o.score_pad = self.pad, self.score_pad
        return o


# (what pickles name that were made when every rule had a function of its own)
_protein_tokens_from_key = functools.partial(_rule_from_key, ProteinTokens)
_base_labels_from_key = functools.partial(_rule_from_key, BaseLabels)
_gene_windows_from_key = functools.partial(_rule_from_key, GeneWindows)
_kmer_counts_from_key = functools.partial(_rule_from_key, KmerCounts)
_protein_groups_from_key = functools.partial(_rule_from_key, ProteinGroups)
_protein_sketches_from_key = functools.partial(_rule_from_key, ProteinSketches)
_start_candidates_from_key = functools.partial(_rule_from_key, StartCandidates)


class DeviceStarts:
    """The candidate start sites of gene records in device memory.  ``positions``, ``types`` (``[T]`` ragged, ``[G, W]`` padded) and
    ``scores`` (``[T, F]`` / ``[G, W, F]``, the columns ``fields``): the tensors; ``lengths``: the candidates of every gene, and
    ``chosen``: the index of the record's own start among them (numpy int64, host); ``offsets``: ragged only, gene g owns candidates
    ``offsets[g] .. offsets[g + 1]``; ``gene_begin``: the genes of contig i are rows ``gene_begin[i] .. gene_begin[i + 1]`` (``None``
    when the records were not in contig order); ``starts[i]``: contig i's part of the three tensors as views."""

    def __init__(self, positions, types, scores, chosen, lengths, offsets, gene_begin, genes, fields, device, plan=None, stream=None,
                 nodes=None):
        self.positions, self.types, self.scores, self.chosen, self.lengths = positions, types, scores, chosen, lengths
        self.offsets, self.gene_begin, self.genes, self.fields, self.device = offsets, gene_begin, genes, fields, device
        # the node index of every candidate: on the host already (the finder's call), or still behind the plan (a Context's call)
        self.stream, self._plan, self._nodes, self._records = stream, plan, nodes, None

    @property
    def starts(self):
        return _gene_views(self, self.positions, self.types, self.scores)

    def cu_seqlens(self):
        """The exclusive scan of ``lengths`` as an int32 tensor on the tensors' device (torch)."""
        return _cu_seqlens(self.lengths, self.positions, self.device)

    def records(self):
        """One ``GENE_DTYPE`` record per candidate, in row order: the gene's record with ``begin`` / ``start_ndx`` (forward) or ``end`` /
        ``start_ndx`` (reverse) replaced by the candidate's.  ``positions`` comes to the host once for it, and so does the node index
        of every candidate (4 bytes each, ``pga_start_plan_nodes``).  The records go straight into ``Context.gene_windows`` for the
        sequence context of every candidate, or back into ``start_candidates``."""
        if self._records is None:
            if self._plan is None and self._nodes is None:
                raise ValueError("this DeviceStarts was released: it has no records any more")
            lens = self.lengths
            if self._nodes is None:
                self._nodes = self._plan.nodes(int(lens.sum()))
            pos = _read_device(self.positions, self.stream)       # the tensor's elements, host: [T], or [G, W]
            if self.offsets is None:                               # padded: the first lengths[g] candidates of every row
                pos = pos[np.arange(pos.shape[1])[None, :] < lens[:, None]] if len(lens) else pos.reshape(0)
            pos = pos[:int(lens.sum())].astype(np.int64)
            out = self.genes[np.repeat(np.arange(len(lens)), lens)].copy()
            fwd = out["strand"] == 1
            out["begin"] = np.where(fwd, pos, out["begin"])
            out["end"] = np.where(fwd, out["end"], pos)
            out["start_ndx"] = self._nodes
            self._records = out
            self.release()
        return self._records

    def release(self):
        """Gives the plan's device block back to its context now, not when this object is collected (a result of
        ``Context.start_candidates``: one of ``find_starts_batch`` holds no plan)."""
        if self._plan is not None:
            self._plan.close()
            self._plan = None


class _StartPlan:
    """A ``pga_start_plan`` and the context it was made on: freed when the object is collected.  ``owner``: the :class:`Context`
    of ``Context.start_candidates``, whose caller owns it and makes one call on it at a time; it is kept alive with the plan, since
    ``nodes`` goes through the context.  (A plan whose context was destroyed first is an orphan of the library's: freeing it is all
    that still works.)  The finder's pooled contexts never leave a plan behind: ``starts_into(..., keep_plan=False)``."""

    def __init__(self, L, ctx_h, h, owner=None):
        self.L, self.ctx_h, self.h, self.owner = L, ctx_h, h, owner

    def _context(self):
        if self.h is None or (isinstance(self.owner, Context) and self.owner.h is None):
            raise ValueError("the context that made this DeviceStarts was closed")
        return self.ctx_h

    def nodes(self, total):
        self._context()
        out = np.zeros(max(total, 1), np.int32)
        rc = self.L.pga_start_plan_nodes(self.ctx_h, self.h, ctypes.c_void_p(out.ctypes.data), total)
        if rc != PGA_OK:
            _raise(self.L, self.ctx_h, rc, "pga_start_plan_nodes")
        return out[:total]

    def close(self):
        if self.h is not None:
            self.L.pga_start_plan_free(self.ctx_h, self.h)
            self.h = None

    def __del__(self):
        self.close()


def _read_device(tensor, stream):
    """The elements of a device tensor with a contiguous last dimension as a numpy array of its shape (``pga_device_read`` without a
    context: the pointer names its device)."""
    ptr, shape, strides = _device_array(tensor, "the tensor")
    dt = np.dtype(str(tensor.__cuda_array_interface__["typestr"]))
    row = shape[-1] if len(shape) < 2 else strides[0] // dt.itemsize
    n = ((shape[0] - 1) * row + shape[1] if shape[0] and shape[1] else 0) if len(shape) == 2 else shape[0]
    flat = np.zeros(max(n, 1) if len(shape) == 1 else max(shape[0] * row, 1), dt)    # one buffer: whole rows, their gaps included
    rc = load().pga_device_read(None, ctypes.c_void_p(ptr), n * dt.itemsize, ctypes.c_void_p(flat.ctypes.data),
                                ctypes.c_void_p(DeviceSequences._stream_of(tensor, stream)))
    if rc == PGA_EINVAL:
        raise ValueError("pga_device_read: the tensor is not device memory")
    if rc != PGA_OK:
        raise PgaError(f"pga_device_read failed (code {rc})")
    if len(shape) == 1:
        return flat[:n]
    return flat[:shape[0] * row].reshape(shape[0], row)[:, :shape[1]]


def _start_outputs(spec, out, stream, device, lens):
    """The three device tensors of a :class:`StartCandidates` call: ``out`` checked against the rule's element types and layout and
    against ``lens``, the candidates of every gene, or new torch tensors under torch's current stream.  Returns (the triple, stream,
    their pointers, W, S, the elements of each the layout may use)."""
    n, padded, F = len(lens), spec.layout == "padded", len(spec.fields)
    total, longest = int(lens.sum()) if n else 0, int(lens.max()) if n else 0
    if out is None:
        shape = (n, longest) if padded else (total,)
        out, stream = _torch_outputs(device, stream, [(shape, spec.index_dtype), (shape, spec.index_dtype), (shape + (F,), spec.dtype)],
                                     "three device arrays")
    try:
        positions, types, scores = out
    except (TypeError, ValueError):
        raise TypeError("out must be a (positions, types, scores) triple of device arrays") from None
    ptrs, n_elems, width, stride = [], [], 0, None
    for name, t, typestr, eb, cols in (("positions", positions, spec.index_typestr, spec.index_bytes, 1),
                                       ("types", types, spec.index_typestr, spec.index_bytes, 1),
                                       ("scores", scores, spec.score_typestr, spec.score_bytes, F)):
        ptr, shape, strides = _device_array(t, name, typestr, f"the rule writes {typestr}")
        want_dims = (2 if padded else 1) + (cols > 1 or name == "scores")
        if len(shape) != want_dims or (name == "scores" and shape[-1] != F):
            raise ValueError("%s must be %s, not of shape %s" % (name, ("[%d, W" % n if padded else "[T") + (", %d]" % F if name == "scores" else "]"), shape))
        inner = shape[-1] if name == "scores" else 1                   # elements of one candidate
        if name == "scores" and F > 1 and strides[-1] != eb:
            raise ValueError("the last dimension of scores is not contiguous")
        cand = strides[-2] if name == "scores" else strides[-1]        # bytes from a candidate to the next
        if shape[-2 if name == "scores" else -1] > 1 and cand != eb * inner:
            raise ValueError(f"the candidates of {name} are not contiguous")
        if padded:
            if shape[0] != n:
                raise ValueError(f"the padded layout needs {n} rows: {name} has {shape[0]}")
            w = shape[1]
            s_ = w if n < 2 else strides[0] // (eb * inner)
            if n > 1 and (strides[0] % (eb * inner) or strides[0] < 0):
                raise ValueError(f"the rows of {name} do not lie a whole, positive number of candidates apart")
            if w < longest:
                raise ValueError(f"{name} has {w} columns: gene {int(np.argmax(lens))} has {longest} candidates")
            if stride is None:
                width, stride = w, s_
            elif (w, s_) != (width, stride) and n > 0:
                raise ValueError(f"{name} has {w} columns a stride of {s_} apart: positions has {width}, {stride} apart")
            n_elems.append(((n - 1) * s_ + w if n else 0) * inner)
        else:
            if shape[0] < total:
                raise ValueError(f"{name} has {shape[0]} candidates: the genes have {total}")
            n_elems.append(shape[0] * inner)
        ptrs.append(ctypes.c_void_p(ptr))
    return (positions, types, scores), stream, ptrs, width, stride or 0, n_elems


def starts_into(L, ctx_h, batch_h, device, n_contigs, genes, spec, out=None, stream=None, owner=None, keep_plan=True):
    """``pga_start_plan_create`` / ``pga_start_plan_write`` on raw handles (what ``Context.start_candidates`` and the finder's device
    call share): the candidate starts of ``genes`` (GENE_DTYPE records of the resident batch whose node arrays the context has on
    record) into ``out``, or into new torch tensors."""
    if not isinstance(spec, StartCandidates):
        raise TypeError("the start rule must be a StartCandidates, not %r" % type(spec).__name__)
    genes = np.ascontiguousarray(genes, dtype=GENE_DTYPE)
    n = len(genes)
    count, chosen = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    h = ctypes.c_void_p()
    rc = L.pga_start_plan_create(ctx_h, batch_h, n, ctypes.c_void_p(genes.ctypes.data), ctypes.byref(h), ctypes.c_void_p(count.ctypes.data),
                                 ctypes.c_void_p(chosen.ctypes.data))
    if rc != PGA_OK:
        _raise(L, ctx_h, rc, "pga_start_plan_create")
    plan = _StartPlan(L, ctx_h, h, owner)
    lens = count[:n].astype(np.int64)
    nodes = None
    try:
        out, stream, ptrs, width, stride, n_elems = _start_outputs(spec, out, stream, device, lens)
        o = spec.opts(width, stride)
        rc = L.pga_start_plan_write(ctx_h, plan.h, ctypes.byref(o), ptrs[0], ptrs[1], ptrs[2], n_elems[0], n_elems[1], n_elems[2],
                                    ctypes.c_void_p(DeviceSequences._stream_of(out[0], stream)))
        if rc != PGA_OK:
            _raise(L, ctx_h, rc, "pga_start_plan_write")
        if not keep_plan:                                          # the node indices now, 4 bytes per candidate
            nodes = plan.nodes(int(lens.sum()))
    except BaseException:
        # the plan never outlives a failed call: a traceback would keep it past the point where a pooled context changes hands
        plan.close()
        raise
    if not keep_plan:
        plan.close()
        plan = None
    off = None
    if spec.layout == "ragged":
        off = np.zeros(n + 1, np.int64)
        np.cumsum(lens, out=off[1:])
    return DeviceStarts(out[0], out[1], out[2], chosen[:n].astype(np.int64), lens, off, _gene_begin(genes, n_contigs), genes, spec.fields,
                        device, plan, stream, nodes)


def _start_candidates(self, batch, result_or_genes, spec, out=None, stream=None):
    """Every candidate start site of gene records of the resident ``batch`` -- all start nodes of the record's ORF, with their scores
    under the winning model -- as three device tensors (``pga_start_plan_create`` / ``pga_start_plan_write``): 8 bytes per gene come to
    the host.  The last ``find_genes`` on this context must have been on ``batch`` with ``want_nodes="device"`` (or True).
    ``result_or_genes``: that result, or gene records of it (any subset or order; any start node of a contig makes a record).
    ``spec``: a :class:`StartCandidates`.  ``out``: a ``(positions, types, scores)`` triple of objects with
    ``__cuda_array_interface__``, ``None``: torch tensors are allocated on the context's device under torch's current stream.
    ``stream``: the stream that last used ``out``, as in :class:`DeviceSequences`.  Returns a :class:`DeviceStarts`."""
    genes = getattr(result_or_genes, "genes", result_or_genes)
    return starts_into(self.L, self.h, batch.h, self.device, batch.n, genes, spec, out, stream, owner=self)


class RenderedText:
    """One format's text of a :meth:`Context.render_genes` call: ``data`` (bytes), ``contig_offsets`` (contig i is
    ``data[contig_offsets[i]:contig_offsets[i + 1]]``), ``fallback`` (lines the host rendered itself) and ``kernel_ms`` (device
    time of the format's passes)."""

    __slots__ = ("data", "contig_offsets", "fallback", "kernel_ms")

    def __init__(self, data, contig_offsets, fallback, kernel_ms):
        self.data, self.contig_offsets, self.fallback, self.kernel_ms = data, contig_offsets, fallback, kernel_ms

    def contig(self, i):
        return self.data[self.contig_offsets[i]:self.contig_offsets[i + 1]]


# the writers' defaults (Genes.write_gff / write_translations / write_genes / write_genbank / write_scores)
_WRITER_DEFAULTS = {
    "gff": {"header": True, "include_translation_table": False, "full_id": True, "version_separator": "_v"},
    "faa": {"width": 60, "translation_table": None, "include_stop": True, "strict_translation": True, "full_id": False},
    "fna": {"width": 70, "full_id": False},
    "gbk": {"division": "BCT", "date": None, "translation_table": None, "strict_translation": True},
    "scores": {"header": True},
}


def _render_formats(formats, writer_options):
    """The writer options of every requested format (``formats``: names, or a dict from names to options), checked as the host
    writers check them; no device needed."""
    import datetime
    if isinstance(formats, str):
        formats = (formats,)
    fmt_opts = {}
    for name in formats:
        if name not in _WRITER_DEFAULTS:
            raise ValueError("unknown format %r (expected one of %s)" % (name, ", ".join(RENDER_FORMATS)))
        o = dict(_WRITER_DEFAULTS[name])
        o.update({k: v for k, v in writer_options.items() if k in o})
        if isinstance(formats, dict) and formats[name]:
            bad = set(formats[name]) - set(o)
            if bad:
                raise TypeError("%s: unexpected option(s) %s" % (name, ", ".join(sorted(bad))))
            o.update(formats[name])
        fmt_opts[name] = o
    bad = set(writer_options) - set().union(*[set(v) for v in _WRITER_DEFAULTS.values()])
    if bad:
        raise TypeError("unexpected option(s) %s" % ", ".join(sorted(bad)))
    if "gbk" in fmt_opts:
        # as write_genbank: a table among the known ones, a datetime.date (today when None), the division as given
        from .cli import TRANSLATION_TABLES
        g = fmt_opts["gbk"]
        tt = g["translation_table"]
        if tt is not None and tt not in TRANSLATION_TABLES:
            raise ValueError("%r is not a valid translation table index" % (tt,))
        date = g["date"]
        if date is None:
            date = datetime.date.today()
        elif not isinstance(date, datetime.date):
            raise TypeError("Expected datetime.date, found %s" % type(date).__name__)
        if not isinstance(g["division"], str):
            raise TypeError("Expected str, found %s" % type(g["division"]).__name__)
        g["date"] = date
    return fmt_opts


def _render_genes(self, batch, result, ids, formats=RENDER_FORMATS, *, meta=False, model_of_contig=None, descriptions=None,
                  first_seqnum=1, fallback_margin=1e-9, unbinned_model=None, seqnums=None, **writer_options):
    """GFF / protein FASTA / gene FASTA of ``result`` (a result of ``find_genes`` on the resident ``batch``), rendered on the
    device: byte for byte what ``Genes.write_gff`` / ``write_translations`` / ``write_genes`` write for these genes, contig
    after contig.

    ``ids``: the sequence id of every contig; ``first_seqnum``: the seqnum of contig 0 (``seqnums``: one per contig instead, for a
    batch whose contigs are not consecutive records of their file).  ``formats``: names among "gff", "faa",
    "fna", or a dict from those names to the writer's keyword arguments (``header``, ``include_translation_table``, ``full_id``,
    ``version_separator`` / ``width``, ``translation_table``, ``include_stop``, ``strict_translation``, ``full_id`` /
    ``width``, ``full_id``); ``writer_options`` apply to every format that takes them.  ``meta``: the models are metagenomic
    bins (``descriptions`` gives theirs) and contig i was called with ``result.contigs[i]["model"]``; else single mode with
    model 0, or with ``model_of_contig[i]``.  ``unbinned_model`` (meta mode): the model whose data the GFF header of a contig
    without genes, which no bin won, reports (Prodigal writes bin 5's); None: such a contig is an error for GFF, as it is for
    ``write_gff``.  Returns ``{name: RenderedText}``.

    "gbk" (``division``, ``date``, ``translation_table``, ``strict_translation``) is ``Genes.write_genbank``'s record.  "scores"
    (``header``) is ``Genes.write_scores``' start file: it needs the node arrays of ``result`` on the device, i.e. ``result`` is
    the last ``find_genes`` on this context and was called with ``want_nodes="device"`` (or True); a contig no bin won gets
    ``unbinned_model``'s header and an empty body."""
    from . import __version__ as version
    fmt_opts = _render_formats(formats, writer_options)
    n = batch.n
    ids = [str(x) for x in ids]
    if len(ids) != n:
        raise ValueError("%d ids for %d contigs" % (len(ids), n))
    contigs = np.ascontiguousarray(result.contigs)
    genes = np.ascontiguousarray(result.genes)
    if model_of_contig is None:
        moc = contigs["model"].astype(np.int32) if meta else np.zeros(n, np.int32)
        if meta and unbinned_model is not None:
            if not 0 <= int(unbinned_model) < len(self._models):
                raise ValueError("`unbinned_model` %r is not a loaded model" % (unbinned_model,))
            moc[moc < 0] = int(unbinned_model)
    else:
        moc = np.ascontiguousarray(model_of_contig, np.int32)
    moc = np.ascontiguousarray(moc, np.int32)
    nm = len(self._models)
    if descriptions is None:
        descriptions = [""] * nm if meta else ["Ab initio"] * nm
    if len(descriptions) != nm:
        raise ValueError("%d descriptions for %d models" % (len(descriptions), nm))
    id_bytes = [x.encode("utf-8") for x in ids]
    id_off = np.zeros(n + 1, np.int64)
    np.cumsum([len(b) for b in id_bytes], out=id_off[1:])
    id_arena = b"".join(id_bytes)
    desc = (ctypes.c_char_p * max(nm, 1))(*[d.encode("utf-8") for d in descriptions])
    o = RenderOpts()
    o.meta = int(bool(meta))
    o.first_seqnum = int(first_seqnum)
    o.model_desc = desc
    o.fallback_margin = float(fallback_margin)
    sep = fmt_opts.get("gff", _WRITER_DEFAULTS["gff"])["version_separator"]
    o.source = ("pyrodigal_amd%s%s" % (sep, version)).encode("utf-8")
    o.version = ("pyrodigal_amd.v%s" % version).encode("utf-8")
    for k, name in enumerate(RENDER_FORMATS):
        if name in fmt_opts:
            o.formats |= 1 << k
    if "gff" in fmt_opts:
        g = fmt_opts["gff"]
        o.gff_header, o.gff_include_translation_table, o.gff_full_id = int(bool(g["header"])), int(bool(g["include_translation_table"])), int(bool(g["full_id"]))
    if "faa" in fmt_opts:
        a = fmt_opts["faa"]
        tt = a["translation_table"]
        if tt is not None and (not isinstance(tt, int) or tt <= 0):
            raise ValueError("%r is not a valid translation table index" % (tt,))
        o.faa_width, o.faa_translation_table = _width(a["width"]), 0 if tt is None else int(tt)
        o.faa_include_stop, o.faa_strict, o.faa_full_id = int(bool(a["include_stop"])), int(bool(a["strict_translation"])), int(bool(a["full_id"]))
    if "fna" in fmt_opts:
        o.fna_width, o.fna_full_id = _width(fmt_opts["fna"]["width"]), int(bool(fmt_opts["fna"]["full_id"]))
    if "gbk" in fmt_opts:
        g = fmt_opts["gbk"]
        o.gbk_division = g["division"].encode("utf-8")
        o.gbk_date = g["date"].strftime("%d-%b-%y").upper().encode("utf-8")
        o.gbk_version = version.encode("utf-8")
        o.gbk_translation_table = 0 if g["translation_table"] is None else int(g["translation_table"])
        o.gbk_strict = int(bool(g["strict_translation"]))
    if "scores" in fmt_opts:
        o.sco_header = int(bool(fmt_opts["scores"]["header"]))
    res = _P(RenderResult)()
    if seqnums is not None:
        seqnums = np.ascontiguousarray(seqnums, np.int64)
        if seqnums.shape != (n,):
            raise ValueError("%d seqnums for %d contigs" % (seqnums.size, n))
        self.L.pga_render_seqnums(self.h, n, ctypes.c_void_p(seqnums.ctypes.data))
    try:
        rc = self.L.pga_render_genes(self.h, batch.h, contigs.ctypes.data, len(genes), genes.ctypes.data if len(genes) else None,
                                     moc.ctypes.data, id_arena or None, id_off.ctypes.data, ctypes.byref(o), ctypes.byref(res))
    finally:
        if seqnums is not None:
            self.L.pga_render_seqnums(self.h, 0, None)
    if rc != PGA_OK:
        _raise(self.L, self.h, rc, "pga_render_genes")
    try:
        out = {}
        r = res.contents
        for k, name in enumerate(RENDER_FORMATS):
            if name not in fmt_opts:
                continue
            t = r.text[k]
            data = ctypes.string_at(t.data, t.size) if t.size else b""
            coff = np.ctypeslib.as_array(t.contig_off, (n + 1,)).copy()
            nf = int(t.n_fallback)
            if nf and name in ("gbk", "scores"):
                raise PgaError("pga_render_genes: %d %s line(s) hold a value the device cannot print exactly" % (nf, name))
            if nf:
                fb = np.ctypeslib.as_array(t.fallback, (3 * nf,)).reshape(nf, 3).copy()
                data, coff = _splice_fallback(self, name, fmt_opts[name], data, coff, fb, genes, contigs, moc, ids, first_seqnum, seqnums)
            out[name] = RenderedText(data, coff, nf, float(r.t_kernels_ms[k]))
        return out
    finally:
        self.L.pga_render_free(res)


def _width(w):
    if not isinstance(w, (int, np.integer)) or w < 1:
        raise ValueError("`width` must be a positive integer")
    return int(w)


def _splice_fallback(ctx, name, opts, data, coff, fb, genes, contigs, moc, ids, first_seqnum, seqnums=None):
    """The lines the device flagged, rendered by the host writers' own code and put in place of the device's guesses."""
    from . import lib
    tinfs = {}
    pieces, at = [], 0
    shift = np.zeros(len(coff), np.int64)
    starts = coff[:-1]
    for gi, b, e in fb.tolist():
        c = int(genes["contig"][gi])
        m = int(moc[c])
        if m not in tinfs:
            tinfs[m] = lib.TrainingInfo(raw=ctx._models[m].tobytes())
        line = lib._render_gene_line(name, genes[gi:gi + 1].tobytes(), tinfs[m], ids[c], first_seqnum + c if seqnums is None else int(seqnums[c]),
                                     gi - int(contigs["gene_begin"][c]), full_id=opts["full_id"],
                                     include_translation_table=opts.get("include_translation_table", False),
                                     version_separator=opts.get("version_separator", "_v"))
        new = line.encode("utf-8")
        pieces.append(data[at:b]); pieces.append(new)
        at = e
        shift[np.searchsorted(starts, b, side="right"):] += len(new) - (e - b)
    pieces.append(data[at:])
    return b"".join(pieces), coff + shift


Context.render_genes = _render_genes
Context.translate_genes = _translate_genes
Context.translate_tokens = _translate_tokens
Context.label_bases = _label_bases
Context.gene_windows = _gene_windows
Context.start_candidates = _start_candidates
Context.kmer_counts = _kmer_counts
Context.protein_groups = _protein_groups
Context.protein_groups_stats = _protein_groups_stats
Context.protein_sketches = _protein_sketches
Context.protein_sketch_passes = _protein_sketch_passes
Context.cluster_sketches = _cluster_sketches
Context.cluster_stats = _cluster_stats
Context.align_pairs = _align_pairs
Context.align_stats = _align_stats
Context.cluster_edges = _cluster_edges
Context.train = _train
Context.train_batch = _train_batch
Context.upload = _upload
Context.upload_packed = _upload_packed
Context.upload_device = _upload_device
Context.nodes_stage = _nodes_stage
Context.find_genes = _find_genes
Context.find_genes_batch = _find_genes_batch
Context.replicate = _replicate
Context.find_coding_bases = _find_coding_bases


class FastaReader:
    """Multi-record FASTA reader of the C library (ref: tests/fasta.py:59-86 `parse`, 16-57 `zopen`): plain files are mapped and
    parsed by several threads, gzip is inflated by zlib, bz2 / xz (and lz4 / zstd when their modules are installed) by the Python
    module of the format feeding the same C parser.

    ``batches()`` yields lists of ``(id, description, sequence_bytes)`` bounded by a base / record budget, the
    shape ``Context.find_genes_batch`` takes; ``records()`` yields them one by one."""

    _MAGIC = ((b"BZh", "bz2"), (b"\xfd7zXZ", "lzma"), (b"\x04\x22\x4d\x18", "lz4.frame"), (b"\x28\xb5\x2f\xfd", "zstandard"))

    def __init__(self, path):
        self.L = load()
        self.h = ctypes.c_void_p()
        self._stream = self._cb = self._cb_error = None
        with open(path, "rb") as f:
            head = f.read(8)
        module = next((m for magic, m in self._MAGIC if head.startswith(magic)), None)
        if module is None:
            # plain (mapped, parsed by several threads) or gzip (zlib)
            rc = self.L.pga_fasta_open(os.fsencode(path), ctypes.byref(self.h))
        else:
            # the formats the reference's reader sniffs (tests/fasta.py:16-57): decompressed by the Python module, parsed by the C reader
            import importlib
            try:
                mod = importlib.import_module(module)
            except ImportError as err:
                raise RuntimeError("File compression is %s but %s is not installed" % (module.split(".")[0].upper(), module.split(".")[0])) from err
            self._stream = mod.ZstdDecompressor().stream_reader(open(path, "rb")) if module == "zstandard" else mod.open(path, "rb")
            stream = self._stream

            def read(_user, buf, cap):
                # ctypes swallows whatever a callback raises (KeyboardInterrupt included) and hands 0 -- "end of stream" -- to the C
                # reader: a truncated record set without an error.  So everything is caught here, kept, and reported as a failure;
                # batches() / packed_batches() raise it again, chained.
                try:
                    data = stream.read(int(cap))
                except BaseException as err:
                    self._cb_error = err
                    return -1
                ctypes.memmove(buf, data, len(data))
                return len(data)
            self._cb = FASTA_READ_FN(read)
            rc = self.L.pga_fasta_open_callback(self._cb, None, ctypes.byref(self.h))
        if rc != PGA_OK:
            raise (MemoryError if rc == PGA_ENOMEM else OSError)("cannot open %r" % (path,))

    def close(self):
        if getattr(self, "h", None):
            self.L.pga_fasta_close(self.h)
            self.h = None
        if getattr(self, "_stream", None) is not None:
            self._stream.close()
            self._stream = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def batches(self, max_bases=64 << 20, max_records=0):
        n = ctypes.c_int32()
        hdr = _P(ctypes.c_char_p)(); seq = _P(ctypes.c_void_p)(); lens = _P(ctypes.c_int64)()
        while True:
            rc = self.L.pga_fasta_next(self.h, max_bases, max_records, ctypes.byref(n), ctypes.byref(hdr), ctypes.byref(seq), ctypes.byref(lens))
            if rc != PGA_OK:
                self._raise(rc)
            if n.value == 0:
                return
            out = []
            for i in range(n.value):
                fields = hdr[i].decode("utf-8", "replace").split(maxsplit=1)
                out.append((fields[0] if fields else "", fields[1] if len(fields) > 1 else "", ctypes.string_at(seq[i], lens[i])))
            yield out

    def _raise(self, rc):
        """The reader's error; what the decompressor raised inside the read callback comes with it (an interrupt comes back as itself)."""
        cause, self._cb_error = self._cb_error, None
        if cause is not None and not isinstance(cause, Exception):
            raise cause
        err = (MemoryError if rc == PGA_ENOMEM else ValueError)(self.L.pga_fasta_error(self.h).decode("utf-8", "replace"))
        if cause is not None:
            raise err from cause
        raise err

    def records(self):
        for batch in self.batches():
            yield from batch

    def packed_batches(self, max_bases=64 << 20, max_records=0, n_arenas=3):
        """Yield :class:`PackedRecords`: the reader copies every batch into one of ``n_arenas`` pinned staging arenas, filled
        in turn.  A batch's arena is reused ``n_arenas`` batches later, and only after ``release()`` was called on it --
        parsing batch k + 1 overlaps the upload and the device work of batch k."""
        import threading
        n_arenas = max(2, min(8, int(n_arenas)))
        self._free = [threading.Event() for _ in range(n_arenas)]
        for e in self._free:
            e.set()
        n = ctypes.c_int32()
        hdr = _P(ctypes.c_char_p)(); packed = ctypes.c_void_p(); offs = _P(ctypes.c_int64)(); lens = _P(ctypes.c_int64)()
        k = 0
        while True:
            arena = k % n_arenas
            self._free[arena].wait()
            self._free[arena].clear()
            rc = self.L.pga_fasta_next_packed(self.h, max_bases, max_records, n_arenas, ctypes.byref(n), ctypes.byref(hdr),
                                              ctypes.byref(packed), ctypes.byref(offs), ctypes.byref(lens))
            if rc != PGA_OK:
                self._free[arena].set()
                self._raise(rc)
            if n.value == 0:
                self._free[arena].set()
                return
            ids, descs = [], []
            for i in range(n.value):
                fields = hdr[i].decode("utf-8", "replace").split(maxsplit=1)
                ids.append(fields[0] if fields else ""); descs.append(fields[1] if len(fields) > 1 else "")
            o = np.ctypeslib.as_array(offs, (n.value + 1,)).copy()
            ln = np.ctypeslib.as_array(lens, (n.value,)).copy()
            yield PackedRecords(self, n.value, ids, descs, packed.value, o, ln, arena)
            k += 1
