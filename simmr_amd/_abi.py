"""ctypes mirror of include/simmr_hip.h and loader for libsimmr_hip.so.

This is plumbing only: the product is the C-ABI shared library built from
simmr_amd/csrc (hand-written HIP for gfx950).  There is no Python or CPU
fallback — if the library is missing, `load()` raises.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

ROOT = Path(__file__).resolve().parent
LIB_PATH = ROOT / "csrc" / "libsimmr_hip.so"

# status codes
OK, EINVAL, ENOMEM, ENODEV, ERANGE, ESTATE, EGENOME, ENOTSUP = 0, -22, -12, -19, -34, -1, -61, -95

# enum simmr_profile_kind
PERFECT_SHORT, MINIMAL_SHORT, PERFECT_LONG, MINIMAL_LONG, CUSTOM = range(5)
COMM_ID_BYTES = 128
# enum simmr_rng_mode
RNG_REFERENCE, RNG_PHILOX, RNG_PHILOX_FULL = 0, 1, 2
# enum simmr_length_mode
LEN_REFERENCE, LEN_PER_READ = 0, 1
# enum simmr_long_start_mode
START_REFERENCE, START_UNIFORM = 0, 1

FLAG_REVCOMP, FLAG_QSEED_SUBST, FLAG_MSEED_SUBST, FLAG_REDRAWN = 1, 2, 4, 8

(CNT_READS, CNT_BASES, CNT_ACGT_BASES, CNT_SUBSTITUTIONS, CNT_OUTER_REJECTS, CNT_REDRAWN,
 CNT_SEED_SUBST, CNT_QUAL_SUM) = range(8)
N_COUNTERS = 8

U64_MAX = (1 << 64) - 1


class ErrorProfilePOD(C.Structure):
    """struct simmr_error_profile"""
    _fields_ = [
        ("kind", C.c_uint32),
        ("rng_mode", C.c_uint32),
        ("length_mode", C.c_uint32),
        ("read_length", C.c_uint16),
        ("insert_size", C.c_uint16),
        ("mean_phred", C.c_uint8),
        ("long_start_mode", C.c_uint8),
        ("reserved0", C.c_uint8 * 2),
        ("read_length_std", C.c_double),
        ("insert_size_std", C.c_double),
        ("gamma_shape", C.c_float),
        ("gamma_scale", C.c_float),
        ("custom_model", C.c_void_p),
        ("custom_model_bytes", C.c_uint64),
    ]


class Range(C.Structure):
    """struct simmr_range"""
    _fields_ = [("first", C.c_uint64), ("count", C.c_uint64)]


class PlanInfo(C.Structure):
    """struct simmr_plan_info"""
    _fields_ = [
        ("n_units", C.c_uint64),
        ("n_reads", C.c_uint64),
        ("total_bases", C.c_uint64),
        ("seed_used", C.c_uint64),
        ("outer_slots", C.c_uint64),
        ("const_read_length", C.c_uint32),
        ("slot_bytes", C.c_uint32),
    ]


class ReadsOut(C.Structure):
    """struct simmr_reads_out (pointers are raw addresses: device for the HIP
    library, host for the test oracle)."""
    _fields_ = [
        ("seq", C.c_void_p),
        ("qual", C.c_void_p),
        ("seq_off", C.c_void_p),
        ("start", C.c_void_p),
        ("end", C.c_void_p),
        ("contig", C.c_void_p),
        ("genome", C.c_void_p),
        ("read_id", C.c_void_p),
        ("flags", C.c_void_p),
        ("seq_capacity", C.c_uint64),
        ("reads_capacity", C.c_uint64),
        ("qual_offset", C.c_uint32),
        ("slot_bytes", C.c_uint32),
    ]


class OuterSummary(C.Structure):
    """struct simmr_outer_summary"""
    _fields_ = [("units", C.c_uint64 * 2), ("end_state", C.c_uint32 * 2)]


class FastqNames(C.Structure):
    """struct simmr_fastq_names"""
    _fields_ = [
        ("n_genomes", C.c_uint32),
        ("genome_idx", C.POINTER(C.c_uint32)),
        ("genome_id", C.POINTER(C.c_char_p)),
        ("n_contigs", C.POINTER(C.c_uint32)),
        ("sequence_id", C.POINTER(C.c_char_p)),
    ]


class TruthOut(C.Structure):
    """struct simmr_truth_out (device pointers as raw addresses)"""
    _fields_ = [
        ("nm", C.c_void_p),
        ("edit_off", C.c_void_p),
        ("edit_pos", C.c_void_p),
        ("edit_ref", C.c_void_p),
        ("edit_alt", C.c_void_p),
        ("edit_qual", C.c_void_p),
        ("reads_capacity", C.c_uint64),
        ("edits_capacity", C.c_uint64),
    ]


STATS_CYCLES, STATS_NM_BINS = 512, 64


class RunStats(C.Structure):
    """struct simmr_run_stats (host memory)"""
    _fields_ = [
        ("reads", C.c_uint64 * 2),
        ("bases", C.c_uint64 * 2),
        ("qual_n", C.c_uint64 * 256),
        ("qual_mismatch", C.c_uint64 * 256),
        ("pair", C.c_uint64 * 5 * 5),
        ("nm_hist", C.c_uint64 * STATS_NM_BINS),
        ("gc_hist", C.c_uint64 * 101),
        ("cycle_n", C.c_uint64 * STATS_CYCLES * 2),
        ("cycle_qsum", C.c_uint64 * STATS_CYCLES * 2),
        ("cycle_mismatch", C.c_uint64 * STATS_CYCLES * 2),
        ("cycle_base", C.c_uint64 * 5 * STATS_CYCLES * 2),
    ]


DEPTH_HIST_BINS = 256


class DepthContig(C.Structure):
    """struct simmr_depth_contig (host memory)"""
    _fields_ = [
        ("genome", C.c_uint32),
        ("contig", C.c_uint32),
        ("first", C.c_uint64),
        ("len", C.c_uint64),
        ("covered", C.c_uint64),
        ("depth_sum", C.c_uint64),
        ("depth_max", C.c_uint32),
        ("reserved0", C.c_uint32),
        ("first_window", C.c_uint64),
    ]


class DepthWindows(C.Structure):
    """struct simmr_depth_windows (device pointers as raw addresses)"""
    _fields_ = [
        ("sum", C.c_void_p),
        ("covered", C.c_void_p),
        ("max", C.c_void_p),
        ("capacity", C.c_uint64),
        ("n_windows", C.c_uint64),
    ]


class StrainOut(C.Structure):
    """struct simmr_strain_out (device pointers as raw addresses)"""
    _fields_ = [
        ("contig", C.c_void_p),
        ("pos", C.c_void_p),
        ("ref", C.c_void_p),
        ("alt", C.c_void_p),
        ("capacity", C.c_uint64),
    ]


class RegionsOut(C.Structure):
    """struct simmr_regions_out (device pointers as raw addresses)"""
    _fields_ = [
        ("genome", C.c_void_p),
        ("contig", C.c_void_p),
        ("start", C.c_void_p),
        ("len", C.c_void_p),
        ("depth_sum", C.c_void_p),
        ("seq_off", C.c_void_p),
        ("capacity", C.c_uint64),
        ("seq", C.c_void_p),
        ("seq_capacity", C.c_uint64),
    ]


class PileupSites(C.Structure):
    """struct simmr_pileup_sites (device pointers as raw addresses)"""
    _fields_ = [
        ("genome", C.c_void_p),
        ("contig", C.c_void_p),
        ("pos", C.c_void_p),
        ("n", C.c_uint64),
    ]


class FitInfo(C.Structure):
    """struct simmr_fit_info (host memory)"""
    _fields_ = [(n, C.c_uint64) for n in ("n_ref_kmers", "n_pairs", "n_positions", "n_length_bins", "n_insert_bins", "n_reads",
                                         "n_inserts", "length_bin_width", "insert_bin_width")] + \
               [(n, C.c_double) for n in ("read_length_mean", "read_length_std", "insert_size_mean", "insert_size_std")] + \
               [(n, C.c_uint32) for n in ("is_long", "k", "max_alt_kmers", "pad")]


FIT_COLUMNS = ("kmer_ref", "kmer_first", "pair_alt", "pair_count", "pair_prob", "qual_hist", "qual_density", "length_hist",
               "insert_hist", "length_density", "length_lo", "length_hi", "insert_density", "insert_lo", "insert_hi")
FIT_QUALS, FIT_DENSITIES, FIT_MAX_L, FIT_MAX_INSERT = 94, 71, 65535, 5000


class FitOut(C.Structure):
    """struct simmr_fit_out (device pointers as raw addresses)"""
    _fields_ = [(n, C.c_void_p) for n in FIT_COLUMNS] + \
               [(n, C.c_uint64) for n in ("ref_capacity", "pair_capacity", "position_capacity", "length_bin_capacity",
                                          "insert_bin_capacity")]


FIT_SAM_COUNTS = ("lines", "header_lines", "records", "taken_quality", "taken_alignment", "skip_no_sequence", "skip_secondary",
                  "skip_too_long", "skip_unmapped", "skip_mapq0", "skip_mate_unmapped", "skip_no_md", "skip_insert", "skip_cigar_op",
                  "skip_inconsistent")


class FitSamCounts(C.Structure):
    """struct simmr_fit_sam_counts (host memory)"""
    _fields_ = [(n, C.c_uint64) for n in FIT_SAM_COUNTS]


MAPEVAL_COUNTS = ("truth_lines", "truth_header", "truth_entries", "truth_skipped", "lines", "header", "records", "secondary", "cigar_op",
                  "unknown_read", "unknown_ref", "unmapped", "correct", "wrong", "missing", "multiple", "reads_correct", "reads_wrong",
                  "reads_unmapped")


class MapevalCounts(C.Structure):
    """struct simmr_mapeval_counts (host memory)"""
    _fields_ = [(n, C.c_uint64) for n in MAPEVAL_COUNTS]


OVLEVAL_COUNTS = ("truth_lines", "truth_entries", "truth_reads", "lines", "records", "unknown_read", "self", "no_pair", "wrong_strand",
                  "wrong_interval", "correct", "wrong", "pairs_found", "pairs_wrong", "pairs_missed", "pairs_multiple")
OVLEVAL_LEN_ROWS = 41  # SIMMR_OVLEVAL_LEN_ROWS


class OvlevalCounts(C.Structure):
    """struct simmr_ovleval_counts (host memory)"""
    _fields_ = [(n, C.c_uint64) for n in OVLEVAL_COUNTS]


VCFEVAL_COUNTS = ("truth_lines", "truth_header", "truth_entries", "lines", "header", "records", "filtered", "qual_missing", "ref_call", "symbolic",
                  "indel", "long_allele", "ref_call_allele", "calls", "unknown_contig", "no_site", "ref_mismatch", "wrong_allele", "correct", "wrong",
                  "sites_found", "sites_wrong", "sites_missed", "sites_multiple")
VCFEVAL_AD_ROWS = 33  # SIMMR_VCFEVAL_AD_ROWS


class VcfevalCounts(C.Structure):
    """struct simmr_vcfeval_counts (host memory)"""
    _fields_ = [(n, C.c_uint64) for n in VCFEVAL_COUNTS]


class VcfevalConfig(C.Structure):
    """struct simmr_vcfeval_config (host memory)"""
    _fields_ = [("n_names", C.c_uint32), ("use_filtered", C.c_uint32), ("rname", C.POINTER(C.c_char_p))]


TAXEVAL_COUNTS = ("truth_lines", "truth_header", "truth_entries", "truth_paired", "lines", "header", "records", "unknown_read", "unclassified",
                  "unknown_taxon", "scored", "missing", "multiple")
TAXEVAL_RANKS = 8        # SIMMR_TAXEVAL_RANKS
TAXEVAL_CLASSES = 5      # SIMMR_TAXEVAL_CLASSES
TAXEVAL_MAX_DEPTH = 255  # SIMMR_TAXEVAL_MAX_DEPTH


class TaxevalCounts(C.Structure):
    """struct simmr_taxeval_counts (host memory)"""
    _fields_ = [(n, C.c_uint64) for n in TAXEVAL_COUNTS]


class TaxevalConfig(C.Structure):
    """struct simmr_taxeval_config (host memory)"""
    _fields_ = [("n_nodes", C.c_uint64), ("taxid", C.POINTER(C.c_uint32)), ("parent", C.POINTER(C.c_uint32)), ("rank", C.POINTER(C.c_uint8)),
                ("n_genomes", C.c_uint64), ("genome_id", C.POINTER(C.c_char_p)), ("genome_taxid", C.POINTER(C.c_uint32))]


ASMEVAL_COUNTS = ("truth_records", "truth_bases", "truth_invalid", "truth_kmers", "truth_distinct", "truth_shared_distinct", "records", "bases",
                  "invalid", "kmers", "found", "shared", "novel", "contigs_short", "contigs_novel", "contigs_pure", "contigs_mixed",
                  "contigs_shared_only")
ASMEVAL_GENOME_COLS = ("distinct", "distinct_found", "over", "contigs", "contig_bases")  # SIMMR_ASMEVAL_GENOME_COLS
ASMEVAL_MAX_BYTES = 0x7fffffff  # SIMMR_ASMEVAL_MAX_BYTES


class AsmevalCounts(C.Structure):
    """struct simmr_asmeval_counts (host memory)"""
    _fields_ = [(n, C.c_uint64) for n in ASMEVAL_COUNTS]


class AsmevalConfig(C.Structure):
    """struct simmr_asmeval_config (host memory)"""
    _fields_ = [("n_genomes", C.c_uint32), ("k", C.c_uint32), ("plain_search", C.c_uint32), ("genome", C.POINTER(C.c_char_p))]


ASMMAP_COUNTS = ("truth_records", "truth_bases", "truth_invalid", "truth_kmers", "truth_anchors", "truth_repeats", "records", "bases", "invalid", "kmers",
                 "hits", "stray_hits", "repeat_hits", "runs", "runs_dropped", "blocks", "block_bases", "breaks_inter_genome", "breaks_inter_record",
                 "breaks_inversion", "breaks_relocation", "breaks_local", "contigs_unplaced", "contigs_clean", "contigs_local_only", "contigs_misassembled",
                 "misassembled_bases")
ASMMAP_GENOME_COLS = ("truth_bases", "truth_anchors", "blocks", "block_bases", "longest_block")  # SIMMR_ASMMAP_GENOME_COLS
ASMMAP_BLOCK_COLS = ("contig", "truth_record", "strand", "q_start", "q_end", "p_start", "p_end", "hits", "join")  # SIMMR_ASMMAP_BLOCK_COLS
ASMMAP_JOINS = ("none", "inter_genome", "inter_record", "inversion", "relocation", "local")  # SIMMR_ASMMAP_INTER_GENOME .. _LOCAL are 1 .. 5


class AsmmapCounts(C.Structure):
    """struct simmr_asmmap_counts (host memory)"""
    _fields_ = [(n, C.c_uint64) for n in ASMMAP_COUNTS]


class AsmmapConfig(C.Structure):
    """struct simmr_asmmap_config (host memory)"""
    _fields_ = [("n_genomes", C.c_uint32), ("k", C.c_uint32), ("band", C.c_uint32), ("relocation", C.c_uint32), ("min_anchors", C.c_uint32),
                ("genome", C.POINTER(C.c_char_p))]


BINEVAL_COUNTS = ("truth_records", "truth_bases", "truth_none", "records", "unknown_contig", "repeated", "assigned", "assigned_bases", "bins", "cells",
                  "sum_top_bases", "sum_best_bases", "pairs_cells", "pairs_bins", "pairs_genomes", "bins_c90_x5", "bins_c70_x5", "bins_c50_x5",
                  "bins_c90_x10", "bins_c70_x10", "bins_c50_x10")
BINEVAL_GENOME_COLS = ("truth_contigs", "truth_bases", "assigned_contigs", "assigned_bases", "bins", "best_bin", "best_bases")  # SIMMR_BINEVAL_GENOME_COLS
BINEVAL_MAX_BYTES = 0x7fffffff  # SIMMR_BINEVAL_MAX_BYTES


class BinevalCounts(C.Structure):
    """struct simmr_bineval_counts (host memory)"""
    _fields_ = [(n, C.c_uint64) for n in BINEVAL_COUNTS]


CORREVAL_COUNTS = ("truth_lines", "truth_header", "truth_records", "truth_entries", "truth_skipped", "lines", "records", "unknown_read", "scored",
                   "trimmed_records", "longer_records", "compared", "kept", "damaged", "fixed", "left", "miscorrected", "ambiguous", "trimmed_error",
                   "trimmed_clean", "extra", "missing", "multiple", "clean_kept", "clean_damaged", "fixed_all", "improved", "unchanged", "worse")
CORREVAL_CLASSES = ("kept", "damaged", "fixed", "left", "miscorrected")  # SIMMR_CORREVAL_CLASSES
CORREVAL_POS = 512   # SIMMR_CORREVAL_POS
CORREVAL_QUALS = 95  # SIMMR_CORREVAL_QUALS
CORREVAL_NO_HIT = 0xffffffff  # SIMMR_CORREVAL_NO_HIT


class CorrevalCounts(C.Structure):
    """struct simmr_correval_counts (host memory)"""
    _fields_ = [(n, C.c_uint64) for n in CORREVAL_COUNTS]


class CorrevalConfig(C.Structure):
    """struct simmr_correval_config (host memory)"""
    _fields_ = [("lines_per_record", C.c_uint32), ("reserved", C.c_uint32)]


class BinevalConfig(C.Structure):
    """struct simmr_bineval_config (host memory)"""
    _fields_ = [("n_genomes", C.c_uint32), ("hash_bits", C.c_uint32), ("genome", C.POINTER(C.c_char_p))]


class MapevalConfig(C.Structure):
    """struct simmr_mapeval_config (host memory)"""
    _fields_ = [("n_names", C.c_uint32), ("min_overlap_pct", C.c_uint32), ("rname", C.POINTER(C.c_char_p))]


class SamNames(C.Structure):
    """struct simmr_sam_names (host memory)"""
    _fields_ = [
        ("n_genomes", C.c_uint32),
        ("genome_idx", C.POINTER(C.c_uint32)),
        ("n_contigs", C.POINTER(C.c_uint32)),
        ("rname", C.POINTER(C.c_char_p)),
    ]


class OverlapCols(C.Structure):
    """struct simmr_overlap_cols (device pointers as raw addresses)"""
    _fields_ = [
        ("a", C.c_void_p),
        ("b", C.c_void_p),
        ("ref_start", C.c_void_p),
        ("ref_end", C.c_void_p),
        ("row", C.c_void_p),
        ("capacity", C.c_uint64),
    ]


# every symbol include/simmr_hip.h declares: name -> (restype, argtypes)
_P = C.POINTER
SYMBOLS = {
    "simmr_abi_version": (C.c_int, []),
    "simmr_engine_create": (C.c_int, [C.c_int, _P(C.c_void_p)]),
    "simmr_engine_destroy": (None, [C.c_void_p]),
    "simmr_last_error": (C.c_char_p, [C.c_void_p]),
    "simmr_engine_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "simmr_engine_set_read_slots": (C.c_int, [C.c_void_p, C.c_uint32]),
    "simmr_engine_set_plan_overlap": (C.c_int, [C.c_void_p, C.c_int]),
    "simmr_stage_genome": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, _P(C.c_void_p),
                                     _P(C.c_uint64), _P(C.c_uint64)]),
    "simmr_stage_fasta": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, _P(C.c_void_p), _P(C.c_uint64), C.c_int,
                                    C.c_uint64, _P(C.c_uint64), _P(C.c_uint32)]),
    "simmr_stage_synthetic": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, _P(C.c_uint64),
                                        C.c_uint64]),
    "simmr_unstage_contig": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64,
                                       C.c_uint64, C.c_void_p]),
    "simmr_genome_info": (C.c_int, [C.c_void_p, C.c_uint32, _P(C.c_uint32), _P(C.c_uint64)]),
    "simmr_pe_plan": (C.c_int, [C.c_void_p, C.c_uint32, _P(ErrorProfilePOD), C.c_uint64, C.c_int,
                                C.c_uint64, Range, _P(PlanInfo)]),
    "simmr_outer_summarize": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, _P(OuterSummary)]),
    "simmr_pe_plan_at": (C.c_int, [C.c_void_p, C.c_uint32, _P(ErrorProfilePOD), C.c_uint64, C.c_uint64, Range,
                                   C.c_uint64, C.c_uint64, _P(PlanInfo)]),
    "simmr_pe_plan_multi": (C.c_int, [C.c_void_p, C.c_uint32, _P(C.c_uint32), _P(C.c_uint64), _P(ErrorProfilePOD),
                                      C.c_int, C.c_uint64, Range, _P(PlanInfo)]),
    "simmr_pe_emit": (C.c_int, [C.c_void_p, C.c_uint32, _P(ReadsOut)]),
    "simmr_long_plan": (C.c_int, [C.c_void_p, C.c_uint32, _P(C.c_uint32), _P(C.c_uint64),
                                  _P(ErrorProfilePOD), C.c_int, C.c_uint64, Range, _P(PlanInfo)]),
    "simmr_long_emit": (C.c_int, [C.c_void_p, C.c_uint32, _P(ReadsOut)]),
    "simmr_counters": (C.c_int, [C.c_void_p, C.c_void_p, _P(C.c_uint64)]),
    "simmr_counters_reset": (C.c_int, [C.c_void_p]),
    "simmr_comm_unique_id": (C.c_int, [C.c_void_p]),
    "simmr_comm_init": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int]),
    "simmr_allreduce_counts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "simmr_last_emit_kernel_ms": (C.c_int, [C.c_void_p, _P(C.c_float)]),
    "simmr_emit_kernel_ms_mean": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_float)]),
    "simmr_last_plan_ms": (C.c_int, [C.c_void_p, _P(C.c_float)]),
    "simmr_entropy_substitute": (C.c_uint64, [C.c_uint64, C.c_uint32]),
    "simmr_fastq_plan": (C.c_int, [C.c_void_p, C.c_char_p, _P(FastqNames), _P(ReadsOut), C.c_uint64, C.c_int,
                                   _P(C.c_uint64)]),
    "simmr_fastq_emit": (C.c_int, [C.c_void_p, _P(ReadsOut), C.c_void_p, C.c_uint64]),
    "simmr_fastq_plan_direct": (C.c_int, [C.c_void_p, C.c_char_p, _P(FastqNames), C.c_uint32, _P(C.c_uint64)]),
    "simmr_emit_fastq": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "simmr_last_fastq_plan_ms": (C.c_int, [C.c_void_p, _P(C.c_float)]),
    "simmr_truth_plan": (C.c_int, [C.c_void_p, _P(ReadsOut), C.c_uint64, _P(C.c_uint64)]),
    "simmr_truth_emit": (C.c_int, [C.c_void_p, _P(ReadsOut), _P(TruthOut)]),
    "simmr_last_truth_ms": (C.c_int, [C.c_void_p, _P(C.c_float)]),
    "simmr_stats_reset": (C.c_int, [C.c_void_p]),
    "simmr_stats_add": (C.c_int, [C.c_void_p, _P(ReadsOut), C.c_uint64, C.c_uint32]),
    "simmr_stats_read": (C.c_int, [C.c_void_p, _P(RunStats)]),
    "simmr_last_stats_ms": (C.c_int, [C.c_void_p, _P(C.c_float)]),
    "simmr_depth_reset": (C.c_int, [C.c_void_p, _P(C.c_uint64), _P(C.c_uint64)]),
    "simmr_depth_add": (C.c_int, [C.c_void_p, _P(ReadsOut), C.c_uint64]),
    "simmr_depth_emit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "simmr_depth_contig_first": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, _P(C.c_uint64)]),
    "simmr_depth_summarize": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, _P(DepthContig), C.c_uint64, _P(C.c_uint64),
                                        _P(DepthWindows)]),
    "simmr_last_depth_ms": (C.c_int, [C.c_void_p, _P(C.c_float)]),
    "simmr_strain_plan": (C.c_int, [C.c_void_p, C.c_uint32, C.c_double, C.c_uint64, _P(C.c_uint64)]),
    "simmr_strain_apply": (C.c_int, [C.c_void_p, C.c_uint32, _P(StrainOut)]),
    "simmr_last_strain_ms": (C.c_int, [C.c_void_p, _P(C.c_float)]),
    "simmr_regions_plan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, _P(C.c_uint64), _P(C.c_uint64)]),
    "simmr_regions_emit": (C.c_int, [C.c_void_p, C.c_void_p, _P(RegionsOut)]),
    "simmr_last_regions_ms": (C.c_int, [C.c_void_p, _P(C.c_float)]),
    "simmr_pileup_reset": (C.c_int, [C.c_void_p, _P(PileupSites)]),
    "simmr_pileup_add": (C.c_int, [C.c_void_p, _P(ReadsOut), C.c_uint64]),
    "simmr_pileup_read": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "simmr_last_pileup_ms": (C.c_int, [C.c_void_p, _P(C.c_float)]),
    "simmr_sam_plan": (C.c_int, [C.c_void_p, _P(SamNames), _P(ReadsOut), _P(TruthOut), C.c_uint64, C.c_int, _P(C.c_uint64)]),
    "simmr_sam_emit": (C.c_int, [C.c_void_p, _P(ReadsOut), _P(TruthOut), C.c_void_p, C.c_uint64]),
    "simmr_last_sam_ms": (C.c_int, [C.c_void_p, _P(C.c_float)]),
    "simmr_sam_sort_key_bits": (C.c_int, [C.c_uint64, C.c_uint64, _P(C.c_uint32), _P(C.c_uint32)]),
    "simmr_sam_sort_plan": (C.c_int, [C.c_void_p, _P(SamNames), _P(ReadsOut), _P(TruthOut), C.c_uint64, C.c_int, _P(C.c_uint64)]),
    "simmr_sam_sort_emit": (C.c_int, [C.c_void_p, _P(ReadsOut), _P(TruthOut), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "simmr_last_sam_sort_ms": (C.c_int, [C.c_void_p, _P(C.c_float)]),
    "simmr_bam_plan": (C.c_int, [C.c_void_p, _P(SamNames), _P(ReadsOut), _P(TruthOut), C.c_uint64, C.c_int, _P(C.c_uint64)]),
    "simmr_bam_emit": (C.c_int, [C.c_void_p, _P(ReadsOut), _P(TruthOut), C.c_void_p, C.c_uint64]),
    "simmr_last_bam_ms": (C.c_int, [C.c_void_p, _P(C.c_float)]),
    "simmr_bgzf_bound": (C.c_uint64, [C.c_uint64]),
    "simmr_bgzf_frame": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, _P(C.c_uint64)]),
    "simmr_bam_sort_create": (C.c_int, [C.c_void_p, _P(C.c_void_p)]),
    "simmr_bam_sort_destroy": (None, [C.c_void_p]),
    "simmr_bam_sort_plan": (C.c_int, [C.c_void_p, _P(SamNames), _P(ReadsOut), _P(TruthOut), C.c_uint64, C.c_int, _P(C.c_uint64)]),
    "simmr_bam_sort_emit": (C.c_int, [C.c_void_p, _P(ReadsOut), _P(TruthOut), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "simmr_last_bam_sort_ms": (C.c_int, [C.c_void_p, _P(C.c_float)]),
    "simmr_bam_sort_ref_lengths": (C.c_int, [C.c_void_p, _P(C.c_uint64), C.c_uint64, _P(C.c_uint64)]),
    "simmr_bai_plan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, _P(C.c_uint64), C.c_uint64, _P(C.c_uint64)]),
    "simmr_bai_emit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "simmr_overlap_reset": (C.c_int, [C.c_void_p, C.c_int]),
    "simmr_overlap_add": (C.c_int, [C.c_void_p, _P(ReadsOut), C.c_uint64]),
    "simmr_overlap_plan": (C.c_int, [C.c_void_p, C.c_uint64, _P(C.c_uint64), _P(C.c_uint64), _P(C.c_uint64)]),
    "simmr_overlap_window": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, _P(C.c_uint64), _P(C.c_uint64), _P(C.c_uint64)]),
    "simmr_overlap_emit": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, _P(OverlapCols), C.c_void_p, C.c_uint64]),
    "simmr_last_overlap_ms": (C.c_int, [C.c_void_p, _P(C.c_float)]),
    "simmr_fit_reset": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64]),
    "simmr_fit_add": (C.c_int, [C.c_void_p, _P(ReadsOut), C.c_uint64, C.c_uint32]),
    "simmr_fit_plan": (C.c_int, [C.c_void_p, _P(FitInfo)]),
    "simmr_fit_emit": (C.c_int, [C.c_void_p, _P(FitOut)]),
    "simmr_last_fit_ms": (C.c_int, [C.c_void_p, _P(C.c_float)]),
    "simmr_fit_add_sam": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32]),
    "simmr_fit_sam_counts_read": (C.c_int, [C.c_void_p, _P(FitSamCounts)]),
    "simmr_mapeval_create": (C.c_int, [C.c_void_p, _P(C.c_void_p)]),
    "simmr_mapeval_destroy": (None, [C.c_void_p]),
    "simmr_mapeval_reset": (C.c_int, [C.c_void_p, _P(MapevalConfig)]),
    "simmr_mapeval_truth_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "simmr_mapeval_truth_plan": (C.c_int, [C.c_void_p, _P(C.c_uint64)]),
    "simmr_mapeval_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "simmr_mapeval_read": (C.c_int, [C.c_void_p, _P(MapevalCounts), _P(C.c_uint64)]),
    "simmr_mapeval_emit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "simmr_last_mapeval_ms": (C.c_int, [C.c_void_p, _P(C.c_float)]),
    "simmr_ovleval_create": (C.c_int, [C.c_void_p, _P(C.c_void_p)]),
    "simmr_ovleval_destroy": (None, [C.c_void_p]),
    "simmr_ovleval_reset": (C.c_int, [C.c_void_p, C.c_uint32]),
    "simmr_ovleval_truth_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "simmr_ovleval_truth_plan": (C.c_int, [C.c_void_p, _P(C.c_uint64), _P(C.c_uint64)]),
    "simmr_ovleval_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "simmr_ovleval_read": (C.c_int, [C.c_void_p, _P(OvlevalCounts), _P(C.c_uint64)]),
    "simmr_ovleval_emit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "simmr_last_ovleval_ms": (C.c_int, [C.c_void_p, _P(C.c_float)]),
    "simmr_vcfeval_create": (C.c_int, [C.c_void_p, _P(C.c_void_p)]),
    "simmr_vcfeval_destroy": (None, [C.c_void_p]),
    "simmr_vcfeval_reset": (C.c_int, [C.c_void_p, _P(VcfevalConfig)]),
    "simmr_vcfeval_truth_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "simmr_vcfeval_truth_plan": (C.c_int, [C.c_void_p, _P(C.c_uint64)]),
    "simmr_vcfeval_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "simmr_vcfeval_read": (C.c_int, [C.c_void_p, _P(VcfevalCounts), _P(C.c_uint64), _P(C.c_uint64)]),
    "simmr_vcfeval_emit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "simmr_last_vcfeval_ms": (C.c_int, [C.c_void_p, _P(C.c_float)]),
    "simmr_asmeval_create": (C.c_int, [C.c_void_p, _P(C.c_void_p)]),
    "simmr_asmeval_destroy": (None, [C.c_void_p]),
    "simmr_asmeval_reset": (C.c_int, [C.c_void_p, _P(AsmevalConfig)]),
    "simmr_asmeval_truth_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "simmr_asmeval_truth_plan": (C.c_int, [C.c_void_p, _P(C.c_uint64)]),
    "simmr_asmeval_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "simmr_asmeval_read": (C.c_int, [C.c_void_p, _P(AsmevalCounts), _P(C.c_uint64)]),
    "simmr_asmeval_emit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "simmr_asmeval_contigs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, _P(C.c_uint64)]),
    "simmr_last_asmeval_ms": (C.c_int, [C.c_void_p, _P(C.c_float), _P(C.c_float)]),
    "simmr_asmmap_create": (C.c_int, [C.c_void_p, _P(C.c_void_p)]),
    "simmr_asmmap_destroy": (None, [C.c_void_p]),
    "simmr_asmmap_reset": (C.c_int, [C.c_void_p, _P(AsmmapConfig)]),
    "simmr_asmmap_truth_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "simmr_asmmap_truth_plan": (C.c_int, [C.c_void_p, _P(C.c_uint64)]),
    "simmr_asmmap_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "simmr_asmmap_read": (C.c_int, [C.c_void_p, _P(AsmmapCounts), _P(C.c_uint64)]),
    "simmr_asmmap_anchors": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "simmr_asmmap_blocks": (C.c_int, [C.c_void_p, _P(C.c_void_p), C.c_uint64, _P(C.c_uint64)]),
    "simmr_asmmap_contigs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, _P(C.c_uint64)]),
    "simmr_last_asmmap_ms": (C.c_int, [C.c_void_p, _P(C.c_float)]),
    "simmr_correval_create": (C.c_int, [C.c_void_p, _P(C.c_void_p)]),
    "simmr_correval_destroy": (None, [C.c_void_p]),
    "simmr_correval_reset": (C.c_int, [C.c_void_p, _P(CorrevalConfig)]),
    "simmr_correval_truth_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "simmr_correval_truth_plan": (C.c_int, [C.c_void_p, _P(C.c_uint64)]),
    "simmr_correval_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "simmr_correval_read": (C.c_int, [C.c_void_p, _P(CorrevalCounts), _P(C.c_uint64), _P(C.c_uint64), _P(C.c_uint64)]),
    "simmr_correval_emit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "simmr_last_correval_ms": (C.c_int, [C.c_void_p, _P(C.c_float)]),
    "simmr_bineval_create": (C.c_int, [C.c_void_p, _P(C.c_void_p)]),
    "simmr_bineval_destroy": (None, [C.c_void_p]),
    "simmr_bineval_reset": (C.c_int, [C.c_void_p, _P(BinevalConfig)]),
    "simmr_bineval_truth_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "simmr_bineval_truth_plan": (C.c_int, [C.c_void_p, _P(C.c_uint64)]),
    "simmr_bineval_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "simmr_bineval_read": (C.c_int, [C.c_void_p, _P(BinevalCounts), _P(C.c_uint64)]),
    "simmr_bineval_bins": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, _P(C.c_uint64)]),
    "simmr_bineval_cells": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, _P(C.c_uint64)]),
    "simmr_bineval_contigs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, _P(C.c_uint64)]),
    "simmr_last_bineval_ms": (C.c_int, [C.c_void_p, _P(C.c_float), _P(C.c_float)]),
    "simmr_taxeval_create": (C.c_int, [C.c_void_p, _P(C.c_void_p)]),
    "simmr_taxeval_destroy": (None, [C.c_void_p]),
    "simmr_taxeval_reset": (C.c_int, [C.c_void_p, _P(TaxevalConfig)]),
    "simmr_taxeval_lineage": (C.c_int, [C.c_void_p, C.c_uint32, _P(C.c_uint32), _P(C.c_uint32)]),
    "simmr_taxeval_truth_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "simmr_taxeval_truth_plan": (C.c_int, [C.c_void_p, _P(C.c_uint64)]),
    "simmr_taxeval_add": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "simmr_taxeval_read": (C.c_int, [C.c_void_p, _P(TaxevalCounts), _P(C.c_uint64), _P(C.c_uint64)]),
    "simmr_taxeval_emit": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "simmr_taxeval_taxa": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "simmr_last_taxeval_ms": (C.c_int, [C.c_void_p, _P(C.c_float)]),
}

_lib = None


class SimmrError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"simmr error {code}: {msg}")
        self.code = code
        self.msg = msg


def load(path: os.PathLike | None = None) -> C.CDLL:
    """dlopen libsimmr_hip.so and bind every declared symbol.  Raises if the
    HIP extension has not been built — there is deliberately no fallback."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    # One HIP runtime per process: PyTorch bundles its own libamdhip64 / HSA
    # runtime.  If libsimmr_hip.so is dlopen'ed first it binds (RTLD_NOW) to
    # /opt/rocm's copy and the second runtime to initialise finds no device.
    # Loading torch first puts its runtime in the global scope, and ours binds
    # to that one.  Without torch in the process the /opt/rocm runtime is used.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    # SIMMR_HIP_LIB: another build of the same library (A/B timing of a kernel change on one box)
    p = Path(path or os.environ.get("SIMMR_HIP_LIB") or LIB_PATH)
    if not p.exists():
        raise ImportError(
            f"{p} not found: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()' or make -C simmr_amd/csrc)")
    lib = C.CDLL(str(p))
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib
