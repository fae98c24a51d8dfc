"""ctypes declarations of the C ABI in include/basevar_amd.h.

The shared library is the product: it is built in-tree by ``__graft_entry__.build()``
(``make -C basevar_amd/csrc``) and lives at basevar_amd/lib/libbasevar_amd.so.  There is
no Python or CPU implementation behind this module -- if the library is missing, loading
fails loudly.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BASEVAR_AMD_LIB") or os.path.join(HERE, "lib", "libbasevar_amd.so")  # override: A/B builds

BV_MAX_ALT = 4
BV_MAX_GROUPS = 255
BV_NO_GROUP = 0xFF
BV_MEM_DEVICE, BV_MEM_HOST = 0, 1
BV_SLAB_RPR_TAGGED, BV_RPR_TAG_MAX_RANK = 0x1, 0x1FFF  # bv_slab.layout
BV_FLAG_LANES = 0x10000000
BV_FLAG_SPARSE_TIMING = 0x20000000  # include/basevar_amd.h
BV_FORM_SHORT_ROWS, BV_FORM_ONE_KERNEL, BV_FORM_PASS2_FUSED = 0x1, 0x2, 0x4  # include/basevar_amd_diag.h
# bv_engine_config.flags (include/basevar_amd.h)
BV_FLAG_TALLY_ONLY, BV_FLAG_SKIP_FISHER, BV_FLAG_SKIP_LRT, BV_FLAG_TILE_STATE, BV_FLAG_WAVE_SOLVER = 0x1, 0x2, 0x4, 0x8, 0x10
BV_OK, BV_ERR_INVALID_ARG, BV_ERR_NO_DEVICE, BV_ERR_HIP, BV_ERR_TOO_LARGE, BV_ERR_SITE = 0, -1, -2, -3, -4, -5

BV_SITE_COVERED, BV_SITE_VARIANT, BV_SITE_BAD_QUAL = 0x1, 0x2, 0x4
BV_SITE_ZERO_FREQ, BV_SITE_RANKSUM, BV_SITE_SOR_OVERFLOW, BV_SITE_RPR_RANGE = 0x8, 0x10, 0x20, 0x40

# cell encoding of the base_strand plane
BV_CELL_REV, BV_CELL_NOCALL, BV_CELL_N, BV_CELL_INS, BV_CELL_DEL = 0x04, 0x08, 0x08, 0x09, 0x0A

SITE_DTYPE = np.dtype([
    ("depth", "<u4", 4), ("total_depth", "<u4"), ("status", "<u4"),
    ("cvg_sb", "<u4", 4), ("cvg_fs", "<f8"), ("cvg_sor", "<f8"),
    ("n_alt", "u1"), ("alt", "u1", 4), ("n_em", "u1"), ("em_iters", "<u2"),
    ("af", "<f8", 4), ("caf", "<f8", 4), ("qual", "<f8"), ("chi2", "<f8"), ("qd", "<f8"),
    ("var_sb", "<u4", 4), ("var_fs", "<f8"), ("var_sor", "<f8"),
    ("mq_ranksum", "<f8"), ("rpr_ranksum", "<f8"), ("bq_ranksum", "<f8"),
])
GROUP_DTYPE = np.dtype([("n_alt", "u1"), ("alt", "u1", 4), ("reserved", "u1", 3), ("total_depth", "<u4"),
                        ("reserved2", "<u4"), ("af", "<f8", 4)])
assert SITE_DTYPE.itemsize == 208 and GROUP_DTYPE.itemsize == 48


class Slab(C.Structure):
    _fields_ = [("n_sites", C.c_uint32), ("n_samples", C.c_uint32), ("pitch", C.c_uint64),
                ("base_strand", C.c_void_p), ("qual", C.c_void_p), ("mapq", C.c_void_p), ("rpr", C.c_void_p),
                ("ref_base", C.c_void_p), ("group_id", C.c_void_p), ("n_groups", C.c_uint32),
                ("mem_kind", C.c_uint32), ("layout", C.c_uint32), ("reserved_", C.c_uint32)]


class SparseTile(C.Structure):
    _fields_ = [("n_sites", C.c_uint32), ("n_samples", C.c_uint32), ("n_entries", C.c_uint32), ("n_groups", C.c_uint32),
                ("row_start", C.c_void_p), ("sample", C.c_void_p), ("base_strand", C.c_void_p), ("qual", C.c_void_p), ("mapq", C.c_void_p),
                ("rpr", C.c_void_p), ("group_id", C.c_void_p), ("mem_kind", C.c_uint32), ("layout", C.c_uint32)]


class TextRows(C.Structure):  # bv_text_rows
    _fields_ = [("text", C.c_void_p), ("row_off", C.c_void_p), ("file_samples", C.c_void_p), ("text_bytes", C.c_uint64),
                ("n_positions", C.c_uint32), ("n_files", C.c_uint32), ("reserved_", C.c_uint32)]


BV_TEXT_SKIP, BV_TEXT_HOST, BV_TEXT_INDEL = 1, 2, 4  # bv_engine_text_parse row states


class BgzfMembers(C.Structure):  # bv_bgzf_members (include/basevar_amd_bgzf.h)
    _fields_ = [("data", C.c_void_p), ("member_off", C.c_void_p), ("data_bytes", C.c_uint64), ("n_members", C.c_uint32),
                ("reserved_", C.c_uint32)]


class BgzfRows(C.Structure):  # bv_bgzf_rows
    _fields_ = [("data", C.c_void_p), ("member_off", C.c_void_p), ("data_bytes", C.c_uint64), ("file_member", C.c_void_p),
                ("file_samples", C.c_void_p), ("skip_bytes", C.c_void_p), ("skip_lines", C.c_void_p), ("n_files", C.c_uint32),
                ("max_positions", C.c_uint32), ("at_end", C.c_uint32), ("reserved_", C.c_uint32)]


class BgzfCursor(C.Structure):  # bv_bgzf_cursor
    _fields_ = [("member", C.c_uint32), ("offset", C.c_uint32)]


class TextRegion(C.Structure):  # bv_text_region (include/basevar_amd_region.h)
    _fields_ = [("name", C.c_char_p), ("name_len", C.c_uint32), ("beg", C.c_uint32), ("end", C.c_uint32), ("reserved_", C.c_uint32)]


class VcfLines(C.Structure):  # bv_vcf_lines (include/basevar_amd_vcf.h)
    _fields_ = [("slab", C.POINTER(Slab)), ("site", C.c_void_p), ("head", C.c_void_p), ("head_off", C.c_void_p), ("gt", C.c_void_p),
                ("n_lines", C.c_uint32), ("reserved_", C.c_uint32)]


class RecordLines(C.Structure):  # bv_record_lines (include/basevar_amd_record_text.h)
    _fields_ = [("records", C.c_void_p), ("groups", C.c_void_p), ("pos", C.c_void_p), ("ref_char", C.c_void_p), ("chrom", C.c_void_p),
                ("group_names", C.c_void_p), ("group_name_off", C.c_void_p), ("host_text", C.c_void_p), ("host_text_off", C.c_void_p),
                ("indel", C.c_void_p), ("indel_off", C.c_void_p), ("slab", C.POINTER(Slab)), ("site", C.c_void_p),
                ("n_lines", C.c_uint32), ("n_groups", C.c_uint32), ("chrom_len", C.c_uint32), ("mem_kind", C.c_int32), ("reserved_", C.c_uint32)]


RECORD_TEXT_NAME_MAX, RECORD_TEXT_INDEL_MAX = 255, 16384


class IndelTokens(C.Structure):  # bv_indel_tokens (include/basevar_amd_indel.h)
    _fields_ = [("tokens", C.c_void_p), ("text", C.c_void_p), ("n_tokens", C.c_uint64), ("text_bytes", C.c_uint64), ("mem_kind", C.c_int32),
                ("reserved_", C.c_uint32)]


class PileupReads(C.Structure):  # bv_pileup_reads (include/basevar_amd_pileup.h)
    _fields_ = [("records", C.c_void_p), ("run_off", C.c_void_p), ("run_sample", C.c_void_p), ("pitch", C.c_uint64),
                ("n_runs", C.c_uint32), ("n_samples", C.c_uint32), ("tid", C.c_int32), ("region_beg", C.c_uint32), ("region_end", C.c_uint32),
                ("beg", C.c_uint32), ("end", C.c_uint32), ("mapq_thd", C.c_int32), ("mem_kind", C.c_uint32), ("reserved_", C.c_uint32)]


class PileupResult(C.Structure):  # bv_pileup_result
    _fields_ = [("cell", C.c_void_p), ("qual", C.c_void_p), ("mapq", C.c_void_p), ("rank", C.c_void_p), ("depth", C.c_void_p), ("tokens", C.c_void_p),
                ("text", C.c_void_p), ("cells_capacity", C.c_uint64), ("rows_capacity", C.c_uint64), ("tokens_capacity", C.c_uint64),
                ("text_capacity", C.c_uint64), ("cells", C.c_uint64), ("rows", C.c_uint64), ("n_tokens", C.c_uint64), ("text_bytes", C.c_uint64),
                ("mem_kind", C.c_uint32), ("reserved_", C.c_uint32)]


class PileupBgzfRun(C.Structure):  # bv_pileup_bgzf_run (include/basevar_amd_pileup_bgzf.h)
    _fields_ = [("sample", C.c_uint32), ("first_member", C.c_uint32), ("n_members", C.c_uint32), ("begin", C.c_uint32), ("end", C.c_uint32),
                ("reserved_", C.c_uint32)]


class PileupBgzf(C.Structure):  # bv_pileup_bgzf
    _fields_ = [("members", BgzfMembers), ("runs", C.c_void_p), ("pitch", C.c_uint64), ("n_runs", C.c_uint32), ("n_samples", C.c_uint32),
                ("tid", C.c_int32), ("region_beg", C.c_uint32), ("region_end", C.c_uint32), ("beg", C.c_uint32), ("end", C.c_uint32),
                ("mapq_thd", C.c_int32), ("reserved_", C.c_uint32)]


PILEUP_BGZF_RUN_DTYPE = np.dtype([("sample", "<u4"), ("first_member", "<u4"), ("n_members", "<u4"), ("begin", "<u4"), ("end", "<u4"), ("reserved_", "<u4")])
assert PILEUP_BGZF_RUN_DTYPE.itemsize == C.sizeof(PileupBgzfRun) == 24


class PileupTile(C.Structure):  # bv_pileup_tile (include/basevar_amd_pileup_text.h)
    _fields_ = [("cell", C.c_void_p), ("qual", C.c_void_p), ("mapq", C.c_void_p), ("rank", C.c_void_p), ("tokens", C.c_void_p), ("text", C.c_void_p),
                ("pitch", C.c_uint64), ("n_tokens", C.c_uint64), ("text_bytes", C.c_uint64), ("beg", C.c_uint32), ("rows", C.c_uint32),
                ("n_samples", C.c_uint32), ("mem_kind", C.c_uint32)]


class PileupText(C.Structure):  # bv_pileup_text
    _fields_ = [("tile", C.POINTER(PileupTile)), ("chrom", C.c_char_p), ("chrom_len", C.c_uint32), ("first_row", C.c_uint32), ("n_rows", C.c_uint32),
                ("reserved_", C.c_uint32)]


class PileupTextParts(C.Structure):  # bv_pileup_text_parts (include/basevar_amd_pileup_text_parts.h)
    _fields_ = [("rows", C.POINTER(PileupText)), ("part_first", C.c_void_p), ("n_parts", C.c_uint32), ("reserved_", C.c_uint32)]


PILEUP_TOKEN_DTYPE = np.dtype([("pos", "<u4"), ("sample", "<u4"), ("text_off", "<u8"), ("text_len", "<u4"), ("reserved_", "<u4")])  # bv_pileup_token
assert PILEUP_TOKEN_DTYPE.itemsize == 24

BV_ERR_DATA = -6  # include/basevar_amd_bgzf.h
BV_BGZF_OK, BV_BGZF_BAD_HEADER, BV_BGZF_BAD_DEFLATE, BV_BGZF_BAD_SIZE, BV_BGZF_BAD_CRC = 0, 1, 2, 3, 4
BV_DEFLATE_FAST, BV_DEFLATE_SMALL = 0, 1
DEFLATE_LEVELS = {"fast": BV_DEFLATE_FAST, "small": BV_DEFLATE_SMALL}


class EngineConfig(C.Structure):
    _fields_ = [("device", C.c_int32), ("max_sites", C.c_uint32), ("max_samples", C.c_uint32),
                ("flags", C.c_uint32), ("min_af", C.c_double)]


class SynthParams(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("site_offset", C.c_uint64), ("coverage", C.c_float),
                ("indel_frac", C.c_float), ("qual_mean", C.c_float), ("qual_sd", C.c_float),
                ("qual_min", C.c_uint32), ("qual_max", C.c_uint32), ("layout", C.c_uint32), ("reserved_", C.c_uint32)]


# every symbol include/basevar_amd.h declares
EXPORTS = ["bv_version", "bv_min_af", "bv_engine_create", "bv_engine_destroy", "bv_engine_submit", "bv_engine_submit_many", "bv_engine_submit_many_g", "bv_engine_wait", "bv_engine_join",
           "bv_engine_tiles_begin", "bv_engine_tiles_add", "bv_engine_tiles_add_many", "bv_engine_tiles_add_sparse", "bv_engine_tiles_add_sparse_many", "bv_sparse_tile_packed_layout", "bv_engine_tiles_finish", "bv_tile_packed_layout", "bv_engine_stream",
           "bv_engine_kernel_ms", "bv_engine_timing_reset", "bv_engine_timing_get", "bv_engine_timing_get_ex",
           "bv_host_log_probe", "bv_host_log_eval", "bv_engine_host_log_exact", "bv_engine_host_log_eval",
           "bv_engine_last_variant_count", "bv_last_error", "bv_synth_fill", "bv_device_numa_node", "bv_bind_thread_to_device_node", "bv_engine_last_launch_form", "bv_engine_text_last_layout",
           "bv_engine_text_parse", "bv_engine_text_submit", "bv_engine_deflate_code_lengths", "bv_vcf_tile_samples"]

# every symbol include/basevar_amd_bgzf.h declares
BGZF_EXPORTS = ["bv_engine_bgzf_inflate", "bv_engine_text_parse_bgzf", "bv_engine_text_rows_fetch", "bv_engine_bgzf_deflate", "bv_engine_bgzf_deflate_level"]

# every symbol include/basevar_amd_region.h declares
REGION_EXPORTS = ["bv_engine_text_parse_bgzf_region"]

# every symbol include/basevar_amd_vcf.h declares
VCF_EXPORTS = ["bv_engine_vcf_format", "bv_engine_vcf_fetch", "bv_engine_vcf_deflate"]

# every symbol include/basevar_amd_record_text.h declares
RECORD_TEXT_EXPORTS = ["bv_record_text_on_device", "bv_engine_cvg_format", "bv_engine_cvg_fetch", "bv_engine_cvg_deflate", "bv_engine_vcf_format_records"]

# every symbol include/basevar_amd_indel.h declares
INDEL_EXPORTS = ["bv_indel_row_tokens_max", "bv_engine_indel_tally", "bv_engine_indel_fetch", "bv_engine_cvg_format_tallied"]

# every symbol include/basevar_amd_text_tokens.h declares
TEXT_TOKENS_EXPORTS = ["bv_engine_text_tokens_enable", "bv_engine_text_tokens", "bv_engine_text_tokens_fetch", "bv_engine_text_heads_fetch"]

# every symbol include/basevar_amd_text_job.h declares
TEXT_JOB_EXPORTS = ["bv_engine_text_job_begin", "bv_engine_text_job_add", "bv_engine_text_job_finish"]

# every symbol include/basevar_amd_pileup.h declares
PILEUP_EXPORTS = ["bv_pileup_max_rows", "bv_engine_pileup_set_reference", "bv_engine_pileup", "bv_engine_pileup_fetch", "bv_engine_pileup_rows", "bv_engine_pileup_submit"]

# every symbol include/basevar_amd_pileup_bgzf.h declares
PILEUP_BGZF_EXPORTS = ["bv_engine_pileup_bgzf"]

# every symbol include/basevar_amd_pileup_text.h declares
PILEUP_TEXT_EXPORTS = ["bv_pileup_text_tile_samples", "bv_engine_pileup_text", "bv_engine_pileup_text_fetch", "bv_engine_pileup_text_deflate"]

# every symbol include/basevar_amd_pileup_text_parts.h declares
PILEUP_TEXT_PARTS_EXPORTS = ["bv_engine_pileup_text_parts"]

_lib = None


def load():
    """Load the C-ABI library (once).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "basevar_amd: %s is missing. Build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C basevar_amd/csrc`. There is no CPU fallback." % LIB_PATH)
    # One HIP runtime per process: PyTorch-ROCm wheels bundle their own libamdhip64.  If this
    # library were loaded first it would bind the system runtime, torch would then bring a second
    # one, and the two cannot both own the device.  Importing torch first (when it is installed)
    # lets the dynamic loader resolve libamdhip64.so.* to the copy already in the process.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(LIB_PATH)
    L.bv_version.restype = C.c_char_p
    L.bv_version.argtypes = []
    L.bv_min_af.restype = C.c_double
    L.bv_min_af.argtypes = [C.c_uint32, C.c_float]
    L.bv_engine_create.restype = C.c_int
    L.bv_engine_create.argtypes = [C.POINTER(EngineConfig), C.POINTER(C.c_void_p)]
    L.bv_engine_destroy.restype = C.c_int
    L.bv_engine_destroy.argtypes = [C.c_void_p]
    L.bv_engine_submit.restype = C.c_int
    L.bv_engine_submit.argtypes = [C.c_void_p, C.POINTER(Slab), C.c_void_p, C.c_void_p, C.c_void_p]
    L.bv_engine_submit_many.restype = C.c_int
    L.bv_engine_submit_many.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(Slab), C.POINTER(C.c_void_p), C.c_void_p]
    L.bv_engine_submit_many_g.restype = C.c_int
    L.bv_engine_submit_many_g.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(Slab), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_void_p]
    L.bv_engine_join.restype = C.c_int
    L.bv_engine_join.argtypes = [C.c_void_p, C.c_void_p]
    L.bv_engine_tiles_begin.restype = C.c_int
    L.bv_engine_tiles_begin.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int]
    L.bv_engine_tiles_add.restype = C.c_int
    L.bv_engine_tiles_add.argtypes = [C.c_void_p, C.POINTER(Slab), C.c_void_p]
    L.bv_engine_tiles_add_many.restype = C.c_int
    L.bv_engine_tiles_add_many.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(Slab), C.c_void_p]
    L.bv_engine_tiles_add_sparse.restype = C.c_int
    L.bv_engine_tiles_add_sparse.argtypes = [C.c_void_p, C.POINTER(SparseTile), C.c_void_p]
    L.bv_engine_tiles_add_sparse_many.restype = C.c_int
    L.bv_engine_tiles_add_sparse_many.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(SparseTile), C.c_void_p]
    L.bv_sparse_tile_packed_layout.restype = C.c_int
    L.bv_sparse_tile_packed_layout.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.bv_tile_packed_layout.restype = C.c_int
    L.bv_tile_packed_layout.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.POINTER(C.c_uint64),
                                        C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.bv_engine_tiles_finish.restype = C.c_int
    L.bv_engine_tiles_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.bv_engine_stream.restype = C.c_void_p
    L.bv_engine_stream.argtypes = [C.c_void_p]
    L.bv_engine_wait.restype = C.c_int
    L.bv_engine_wait.argtypes = [C.c_void_p]
    L.bv_engine_kernel_ms.restype = C.c_int
    L.bv_engine_kernel_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.bv_engine_timing_reset.restype = C.c_int
    L.bv_engine_timing_reset.argtypes = [C.c_void_p]
    L.bv_engine_timing_get.restype = C.c_int
    L.bv_engine_timing_get.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint32)]
    L.bv_engine_timing_get_ex.restype = C.c_int
    L.bv_engine_timing_get_ex.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                          C.POINTER(C.c_uint32)]
    L.bv_host_log_probe.restype = C.c_int
    L.bv_host_log_probe.argtypes = [C.POINTER(C.c_double)]
    L.bv_host_log_eval.restype = C.c_double
    L.bv_host_log_eval.argtypes = [C.POINTER(C.c_double), C.c_double]
    L.bv_engine_host_log_exact.restype = C.c_int
    L.bv_engine_host_log_exact.argtypes = [C.c_void_p]
    L.bv_engine_host_log_eval.restype = C.c_int
    L.bv_engine_host_log_eval.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]
    L.bv_engine_last_variant_count.restype = C.c_int
    L.bv_engine_last_variant_count.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    L.bv_last_error.restype = C.c_char_p
    L.bv_last_error.argtypes = [C.c_void_p]
    L.bv_synth_fill.restype = C.c_int
    L.bv_synth_fill.argtypes = [C.c_int, C.POINTER(SynthParams), C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bv_engine_last_launch_form.restype = C.c_int
    L.bv_engine_last_launch_form.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    L.bv_device_numa_node.restype = C.c_int
    L.bv_device_numa_node.argtypes = [C.c_int, C.c_char_p, C.c_size_t]
    L.bv_bind_thread_to_device_node.restype = C.c_int
    L.bv_bind_thread_to_device_node.argtypes = [C.c_int]
    L.bv_engine_text_parse.restype = C.c_int
    L.bv_engine_text_parse.argtypes = [C.c_void_p, C.POINTER(TextRows), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    L.bv_engine_text_submit.restype = C.c_int
    L.bv_engine_text_submit.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Slab), C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p]
    L.bv_engine_bgzf_inflate.restype = C.c_int
    L.bv_engine_bgzf_inflate.argtypes = [C.c_void_p, C.POINTER(BgzfMembers), C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bv_engine_text_parse_bgzf.restype = C.c_int
    L.bv_engine_text_parse_bgzf.argtypes = [C.c_void_p, C.POINTER(BgzfRows), C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p, C.c_void_p, C.c_void_p]
    L.bv_engine_text_parse_bgzf_region.restype = C.c_int
    L.bv_engine_text_parse_bgzf_region.argtypes = [C.c_void_p, C.POINTER(BgzfRows), C.POINTER(TextRegion), C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p,
                                                   C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p]
    L.bv_engine_text_rows_fetch.restype = C.c_int
    L.bv_engine_text_rows_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p]
    L.bv_engine_bgzf_deflate.restype = C.c_int
    L.bv_engine_bgzf_deflate.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    L.bv_engine_bgzf_deflate_level.restype = C.c_int
    L.bv_engine_bgzf_deflate_level.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p,
                                               C.c_void_p]
    L.bv_engine_deflate_code_lengths.restype = C.c_int
    L.bv_engine_deflate_code_lengths.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p]
    L.bv_vcf_tile_samples.restype = C.c_uint32
    L.bv_vcf_tile_samples.argtypes = []
    L.bv_engine_vcf_format.restype = C.c_int
    L.bv_engine_vcf_format.argtypes = [C.c_void_p, C.POINTER(VcfLines), C.c_void_p, C.c_void_p]
    L.bv_engine_vcf_fetch.restype = C.c_int
    L.bv_engine_vcf_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]
    L.bv_engine_vcf_deflate.restype = C.c_int
    L.bv_engine_vcf_deflate.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    L.bv_record_text_on_device.restype = C.c_int
    L.bv_record_text_on_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32]
    for name in ("bv_engine_cvg_format", "bv_engine_vcf_format_records"):
        getattr(L, name).restype = C.c_int
        getattr(L, name).argtypes = [C.c_void_p, C.POINTER(RecordLines), C.c_void_p, C.c_void_p]
    L.bv_engine_cvg_fetch.restype = C.c_int
    L.bv_engine_cvg_fetch.argtypes = L.bv_engine_vcf_fetch.argtypes
    L.bv_engine_cvg_deflate.restype = C.c_int
    L.bv_engine_cvg_deflate.argtypes = L.bv_engine_vcf_deflate.argtypes
    L.bv_indel_row_tokens_max.restype = C.c_uint32
    L.bv_indel_row_tokens_max.argtypes = []
    L.bv_engine_indel_tally.restype = C.c_int
    L.bv_engine_indel_tally.argtypes = [C.c_void_p, C.POINTER(IndelTokens), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bv_engine_indel_fetch.restype = C.c_int
    L.bv_engine_indel_fetch.argtypes = L.bv_engine_vcf_fetch.argtypes
    L.bv_engine_cvg_format_tallied.restype = C.c_int
    L.bv_engine_cvg_format_tallied.argtypes = [C.c_void_p, C.POINTER(RecordLines), C.c_void_p, C.c_void_p]
    L.bv_engine_text_last_layout.restype = C.c_int
    L.bv_engine_text_last_layout.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    L.bv_engine_text_job_begin.restype = C.c_int
    L.bv_engine_text_job_begin.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    L.bv_engine_text_job_add.restype = C.c_int
    L.bv_engine_text_job_add.argtypes = [C.c_void_p, C.POINTER(TextRows), C.c_uint32, C.c_void_p, C.c_void_p]
    L.bv_engine_text_job_finish.restype = C.c_int
    L.bv_engine_text_job_finish.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.bv_engine_text_tokens_enable.restype = C.c_int
    L.bv_engine_text_tokens_enable.argtypes = [C.c_void_p, C.c_int]
    L.bv_engine_text_tokens.restype = C.c_int
    L.bv_engine_text_tokens.argtypes = [C.c_void_p, C.POINTER(IndelTokens)]
    L.bv_engine_text_tokens_fetch.restype = C.c_int
    L.bv_engine_text_tokens_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p]
    L.bv_engine_text_heads_fetch.restype = C.c_int
    L.bv_engine_text_heads_fetch.argtypes = L.bv_engine_text_rows_fetch.argtypes
    L.bv_pileup_max_rows.restype = C.c_uint32
    L.bv_pileup_max_rows.argtypes = []
    L.bv_engine_pileup_set_reference.restype = C.c_int
    L.bv_engine_pileup_set_reference.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.bv_engine_pileup.restype = C.c_int
    L.bv_engine_pileup.argtypes = [C.c_void_p, C.POINTER(PileupReads), C.POINTER(C.c_uint32), C.c_void_p]
    L.bv_engine_pileup_fetch.restype = C.c_int
    L.bv_engine_pileup_fetch.argtypes = [C.c_void_p, C.POINTER(PileupResult), C.c_void_p]
    L.bv_engine_pileup_rows.restype = C.c_int
    L.bv_engine_pileup_rows.argtypes = [C.c_void_p, C.c_int, C.POINTER(Slab), C.c_void_p, C.c_void_p]
    L.bv_engine_pileup_submit.restype = C.c_int
    L.bv_engine_pileup_submit.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.bv_engine_pileup_bgzf.restype = C.c_int
    L.bv_engine_pileup_bgzf.argtypes = [C.c_void_p, C.POINTER(PileupBgzf), C.POINTER(C.c_uint32), C.c_void_p]
    L.bv_pileup_text_tile_samples.restype = C.c_uint32
    L.bv_pileup_text_tile_samples.argtypes = []
    L.bv_engine_pileup_text.restype = C.c_int
    L.bv_engine_pileup_text.argtypes = [C.c_void_p, C.POINTER(PileupText), C.c_void_p, C.c_void_p]
    L.bv_engine_pileup_text_fetch.restype = C.c_int
    L.bv_engine_pileup_text_fetch.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]
    L.bv_engine_pileup_text_deflate.restype = C.c_int
    L.bv_engine_pileup_text_deflate.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    L.bv_engine_pileup_text_parts.restype = C.c_int
    L.bv_engine_pileup_text_parts.argtypes = [C.c_void_p, C.POINTER(PileupTextParts), C.c_void_p, C.c_void_p]
    _lib = L
    return L
