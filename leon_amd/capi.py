"""ctypes binding of include/leon_dna.h.  Mirrors the C-ABI one to one; no compute happens in Python."""
import ctypes as C
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

ABI_VERSION = 5          # include/leon_dna.h LEON_DNA_ABI_VERSION this binding (Stats, _EXPORTS) was written for
HEADER_TEXT_DEVICE_CAP = 4096   # the longest header k_hdr_text builds on the device (kernels.h LEON_HT_HEADER_CAP); longer ones go to the host decoder
LEON_F_KEEP_TRACE = 1
LEON_F_DICT_ON_DEVICE = 2
LEON_F_DICT_PIECES = 4
DICT_PIECE_ANCHORS_DEFAULT, DICT_PIECE_ANCHORS_MAX = 1024, 1 << 20


class LeonDnaError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("leon_dna error %d: %s" % (code, msg))
        self.code = code


def lib_path():
    return os.path.join(_HERE, "lib", "libleon_dna.so")


class _Cfg(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("kmer_size", C.c_uint32), ("reads_per_block", C.c_uint32),
                ("bloom_n_hash", C.c_uint32), ("bloom_block_nbits", C.c_uint32), ("device_id", C.c_int32),
                ("bloom_tai", C.c_uint64), ("random_values", C.POINTER(C.c_uint64)), ("resolve_window", C.c_uint64),
                ("flags", C.c_uint32), ("dict_piece_anchors", C.c_uint32)]


class Stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("n_reads", "n_bases", "n_blocks", "n_anchors", "n_no_anchor", "n_symbols",
                                           "payload_bytes", "resolve_rounds", "resolve_windows")] + \
               [(n, C.c_float) for n in ("ms_pack", "ms_resolve", "ms_sort", "ms_walk", "ms_symbols", "ms_rangecoder",
                                         "ms_d2h", "ms_total")] + \
               [("walk_launches", C.c_uint32), ("reserved", C.c_uint32), ("ms_anchor_wait", C.c_float),
                ("ms_chain_busy", C.c_float)] + \
               [(n, C.c_float) for n in ("ms_exchange", "ms_exchange_call", "ms_emulated", "ms_emulated_lookups")] + \
               [(n, C.c_uint64) for n in ("xch_words_sent", "xch_words_received", "walk_reads", "resolve_chain_reads", "resolve_chain_windows")] + \
               [("ms_resolve_chain", C.c_float), ("ms_gather_call", C.c_float)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_ if not n.startswith("reserved")}


SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint8), C.c_uint64, C.c_uint32)
# leon_exchange_fn: (user, d_send, send_counts[world], world, &d_recv, &recv_total) -> 0 on success
EXCHANGE = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64))
XCH_OFF, XCH_BY_ANCHOR, XCH_EMULATE = 0, 1, 2
# leon_gather_fn: (user, d_buf, part_bytes, world) -> 0 on success
GATHER = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32)

# leon_piece_sink: (user, offset, bytes, size) -> 0 to go on
PIECE_SINK = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64)


class RecordLayout(C.Structure):
    """leon_record_layout"""
    _fields_ = [("struct_size", C.c_uint32), ("lead", C.c_uint8), ("fastq", C.c_uint8), ("plus_kind", C.c_uint8), ("reserved", C.c_uint8),
                ("wrap", C.c_uint32), ("reserved2", C.c_uint32), ("first_read_index", C.c_uint64), ("hdr_bytes", C.c_uint64)]


class FastqSplitResult(C.Structure):
    """leon_fastq_split_result"""
    _fields_ = [("n_records", C.c_uint64), ("consumed", C.c_uint64), ("header_bytes", C.c_uint64), ("base_bytes", C.c_uint64),
                ("stop", C.c_uint32), ("reason", C.c_uint32), ("plus_bare", C.c_uint64), ("plus_header", C.c_uint64)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


FASTQ_MAX, FASTQ_END, FASTQ_IRREGULAR = 0, 1, 2
FASTQ_R_NONE, FASTQ_R_HEADER, FASTQ_R_PLUS, FASTQ_R_LENGTH, FASTQ_R_PLUS_TEXT, FASTQ_R_PARTIAL = range(6)
FASTQ_TILE, FASTQ_MAX_GROUPS = 4096, 1024      # kernels.h: k_fq_newlines' tile and the cap of its grid


class FastaSplitResult(C.Structure):
    """leon_fasta_split_result"""
    _fields_ = [("n_records", C.c_uint64), ("consumed", C.c_uint64), ("header_bytes", C.c_uint64), ("base_bytes", C.c_uint64),
                ("stop", C.c_uint32), ("reason", C.c_uint32), ("single_max", C.c_uint64), ("next_header", C.c_uint64)]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


FASTA_ANY_WIDTH = (1 << 64) - 1
FASTA_MAX, FASTA_END, FASTA_IRREGULAR = 0, 1, 2
FASTA_R_NONE, FASTA_R_HEADER, FASTA_R_NO_SEQUENCE, FASTA_R_EMPTY_LINE, FASTA_R_WIDTH, FASTA_R_MULTILINE = range(6)

_u8p, _u32p, _i32p, _u64p = (C.POINTER(t) for t in (C.c_uint8, C.c_uint32, C.c_int32, C.c_uint64))

_EXPORTS = {
    "leon_dna_abi_version": (C.c_int, []),
    "leon_last_error": (C.c_char_p, [C.c_void_p]),
    "leon_dna_ctx_create": (C.c_int, [C.POINTER(_Cfg), C.POINTER(C.c_void_p)]),
    "leon_dna_ctx_destroy": (None, [C.c_void_p]),
    "leon_dna_bloom_nbytes": (C.c_int, [C.c_void_p, _u64p]),
    "leon_dna_bloom_upload": (C.c_int, [C.c_void_p, _u8p, C.c_uint64]),
    "leon_dna_bloom_download": (C.c_int, [C.c_void_p, _u8p, C.c_uint64]),
    "leon_dna_bloom_clear": (C.c_int, [C.c_void_p]),
    "leon_dna_bloom_insert": (C.c_int, [C.c_void_p, _u64p, C.c_uint64]),
    "leon_dna_bloom_insert_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "leon_dna_bloom_device_ptr": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), _u64p]),
    "leon_dna_bloom_upload_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "leon_dna_bloom_download_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "leon_dna_bloom_contains4": (C.c_int, [C.c_void_p, _u64p, C.c_uint64, C.c_int, _u8p]),
    "leon_dna_bloom_contains": (C.c_int, [C.c_void_p, _u64p, C.c_uint64, _u8p]),
    "leon_dna_encode_batch": (C.c_int, [C.c_void_p, C.c_void_p, _u64p, C.c_uint64, C.c_uint64, SINK, C.c_void_p]),
    "leon_dna_encode_batch_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, SINK,
                                                C.c_void_p]),
    "leon_dna_decode_blocks": (C.c_int, [C.c_void_p, _u64p, C.c_uint64, _u8p, _u64p, _u32p, _u64p, C.c_uint64, _u8p, C.c_uint64,
                                          _u32p]),
    "leon_dna_decode_blocks_device": (C.c_int, [C.c_void_p, _u64p, C.c_uint64, _u8p, _u64p, _u32p, _u64p, C.c_uint64, C.c_void_p, C.c_uint64,
                                                 C.c_void_p, _u32p]),
    "leon_records_format_device": (C.c_int, [C.c_int, C.POINTER(RecordLayout), C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, _u64p]),
    "leon_records_bam_device": (C.c_int, [C.c_int, C.POINTER(RecordLayout), C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, _u64p]),
    "leon_host_records_bam": (C.c_int, [C.POINTER(RecordLayout), C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_uint64, C.c_void_p, _u64p, C.c_uint32]),
    "leon_bam_header": (C.c_int, [C.c_void_p, C.c_uint64, _u64p]),
    "leon_device_download_pieces": (C.c_int, [C.c_int, C.c_void_p, C.c_uint64, PIECE_SINK, C.c_void_p]),
    "leon_host_anchor_dict_decode": (C.c_int, [_u8p, C.c_uint64, C.c_uint64, C.c_uint32, _u64p]),
    "leon_dna_finish": (C.c_int, [C.c_void_p, C.POINTER(_u8p), _u64p, _u64p]),
    "leon_dna_reset_stream": (C.c_int, [C.c_void_p]),
    "leon_dna_reserve": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64]),
    "leon_header_decode_symbols": (C.c_int, [C.c_void_p, _u8p, _u64p, _u32p, C.c_uint64, C.POINTER(C.c_void_p)]),
    "leon_header_text_from_symbols": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, _u32p, C.c_char_p, C.c_uint64, _u8p, C.c_uint64, _u64p, _u64p, C.c_uint32]),
    "leon_header_symbols_free": (None, [C.c_void_p]),
    "leon_header_decode_blocks_device": (C.c_int, [C.c_void_p, _u8p, _u64p, _u32p, C.c_uint64, C.c_char_p, C.c_uint64, _u8p, C.c_uint64, _u64p, _u64p,
                                                    C.c_uint32, _u64p]),
    "leon_header_decode_text": (C.c_int, [C.c_void_p, _u8p, _u64p, _u32p, _u64p, C.c_uint64, C.c_char_p, C.c_uint64, C.POINTER(C.c_void_p)]),
    "leon_header_text_fetch": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, _u8p, C.c_uint64, _u64p, _u64p]),
    "leon_header_text_device_ptr": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), _u64p]),
    "leon_header_text_free": (None, [C.c_void_p]),
    "leon_dna_set_shard": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32]),
    "leon_dna_set_exchange": (C.c_int, [C.c_void_p, C.c_uint32, EXCHANGE, C.c_void_p]),
    "leon_dna_set_gather": (C.c_int, [C.c_void_p, GATHER, C.c_void_p]),
    "leon_dna_debug_walk_order": (C.c_int, [C.c_void_p, C.c_void_p]),
    "leon_kmer_solid_device": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64,
                                          C.POINTER(C.c_void_p), _u64p, _u64p]),
    "leon_kmer_solid": (C.c_int, [C.c_int, C.c_char_p, _u64p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64, _u64p, C.c_uint64,
                                   _u64p, _u64p]),
    "leon_device_free": (None, [C.c_void_p]),
    "leon_host_anchor_dict_encode": (C.c_int, [_u64p, C.c_uint64, C.c_uint32, _u8p, C.c_uint64, _u64p]),
    "leon_dna_get_stats": (C.c_int, [C.c_void_p, C.POINTER(Stats)]),
    "leon_dna_trace_anchors": (C.c_int, [C.c_void_p, _i32p, _u32p, _u8p, C.c_uint64]),
    "leon_dna_trace_events": (C.c_int, [C.c_void_p, _u8p, C.c_uint64]),
    "leon_dna_anchor_kmers": (C.c_int, [C.c_void_p, _u64p, C.c_uint64]),
    "leon_rc_encode_streams": (C.c_int, [C.c_void_p, _u8p, _u64p, C.c_uint64, _u8p, C.c_uint64, _u64p]),
    "leon_header_encode_batch": (C.c_int, [C.c_void_p, C.c_char_p, _u64p, C.c_uint64, C.c_uint64, C.c_char_p, C.c_uint64, SINK,
                                            C.c_void_p]),
    "leon_header_encode_batch_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_char_p, C.c_uint64,
                                                   SINK, C.c_void_p]),
    "leon_host_header_decode_blocks": (C.c_int, [_u8p, _u64p, _u32p, C.c_uint64, C.c_char_p, C.c_uint64, _u8p, C.c_uint64, _u64p,
                                                  _u64p, C.c_uint32]),
    "leon_header_decode_blocks": (C.c_int, [C.c_void_p, _u8p, _u64p, _u32p, C.c_uint64, C.c_char_p, C.c_uint64, _u8p, C.c_uint64, _u64p,
                                             _u64p, C.c_uint32]),
    "leon_qual_smooth_batch": (C.c_int, [C.c_void_p, C.c_char_p, _u64p, C.c_uint64, _u8p]),
    "leon_qual_smooth_batch_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "leon_kmer_auto_cutoff": (C.c_int, [_u64p, _u32p]),
    "leon_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "leon_device_alloc": (C.c_int, [C.c_int, C.c_uint64, C.POINTER(C.c_void_p)]),
    "leon_device_upload": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_uint64]),
    "leon_device_copy": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_uint64]),
    "leon_device_download": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_uint64]),
    "leon_host_qual_encode_blocks": (C.c_int, [C.c_char_p, _u64p, C.c_uint64, C.c_uint32, C.c_int, C.c_uint32, SINK, C.c_void_p,
                                                C.c_uint64]),
    "leon_qual_deflate_blocks_device": (C.c_int, [C.c_int, C.c_void_p, _u64p, C.c_uint64, C.c_uint32, SINK, C.c_void_p, C.c_uint64]),
    "leon_qual_deflate_release": (None, []),
    "leon_text_bgzf_device": (C.c_int, [C.c_int, C.c_void_p, C.c_uint64, C.c_int, PIECE_SINK, C.c_void_p, _u64p, _u64p, _u64p]),
    "leon_text_bgzf_records_device": (C.c_int, [C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, PIECE_SINK, C.c_void_p,
                                                 _u64p, _u64p, C.c_void_p, C.c_void_p, C.c_uint64, _u64p]),
    "leon_text_bgzf_device_ex": (C.c_int, [C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, PIECE_SINK, C.c_void_p,
                                            _u64p, _u64p, C.c_void_p, C.c_void_p, C.c_uint64, _u64p, C.c_uint32]),
    "leon_host_bgzf_record_cuts": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, _u64p, _u64p]),
    "leon_fastq_split_device": (C.c_int, [C.c_int, C.c_void_p, C.c_uint64, C.c_int, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]),
    "leon_host_fastq_split": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_uint64, C.c_uint64, C.c_void_p]),
    "leon_fasta_split_device": (C.c_int, [C.c_int, C.c_void_p, C.c_uint64, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_uint64, C.c_uint64, C.c_void_p]),
    "leon_host_fasta_split": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_uint64, C.c_uint64, C.c_void_p]),
    "leon_device_trim": (None, []),
    "leon_host_qual_decode_blocks": (C.c_int, [_u8p, _u64p, _u32p, _u64p, C.c_uint64, _u8p, C.c_uint64, _u64p, C.c_uint32]),
    "leon_qual_inflate_blocks_device": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                                   C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64)]),
    "leon_crc32_segments_device": (C.c_int, [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]),
    "leon_host_crc32_segments": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p]),
    "leon_host_bgzf_members": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, _u64p, _u64p, _u64p, _u32p]),
    "leon_host_bgzf_inflate": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32]),
    "leon_bgzf_inflate_device": (C.c_int, [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32,
                                            C.c_void_p]),
    "leon_host_pinned_alloc": (C.c_int, [C.c_int, C.c_uint64, C.POINTER(C.c_void_p)]),
    "leon_host_pinned_free": (None, [C.c_void_p]),
    "leon_letters_count_device": (C.c_int, [C.c_int, C.c_void_p, C.c_uint64, _u64p, _u64p]),
    "leon_letters_take_device": (C.c_int, [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64]),
    "leon_letters_apply_device": (C.c_int, [C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64]),
    "leon_host_letters_apply": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32]),
    "leon_dna_dict_pieces": (C.c_int, [C.c_void_p, C.POINTER(_u64p), _u64p, _u32p]),
    "leon_anchor_dict_encode_pieces_device": (C.c_int, [C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    "leon_anchor_dict_decode_pieces_device": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p]),
    "leon_host_anchor_dict_encode_pieces": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32]),
    "leon_host_anchor_dict_decode_pieces": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32]),
}
EXPORTED_SYMBOLS = tuple(_EXPORTS)
_lib = None


def load_library():
    """dlopen libleon_dna.so and bind every symbol include/leon_dna.h declares.  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise LeonDnaError(-2, "%s is missing: build it with leon_amd.build_library() (hipcc, gfx950); "
                               "there is no CPU fallback" % path)
    lib = C.CDLL(path)
    for name, (res, args) in _EXPORTS.items():
        f = getattr(lib, name)
        f.restype, f.argtypes = res, args
    if lib.leon_dna_abi_version() != ABI_VERSION:
        # (a stale library under a new binding reads wrong stats and misses symbols; a new one under an old binding overruns Stats)
        raise LeonDnaError(-2, "%s has ABI %d, this binding is written for %d: rebuild it (leon_amd.build_library())"
                           % (path, lib.leon_dna_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def _ptr(a, t):
    return a.ctypes.data_as(t)


def kmer_words(k):
    """64-bit words per k-mer at the C-ABI: 1 below k = 32, 2 from 32 to 63"""
    return 2 if k >= 32 else 1


def anchor_dict_decode(payload, n_anchors, kmer_size):
    """Leon::decodeAnchorDict on the host: the anchors' k-mers (n_anchors * W words) from the dictionary stream"""
    lib = load_library()
    out = np.zeros(max(n_anchors * kmer_words(kmer_size), 1), dtype=np.uint64)
    buf = np.frombuffer(bytes(payload) + b"\0", dtype=np.uint8)
    rc = lib.leon_host_anchor_dict_decode(_ptr(buf, _u8p), len(payload), n_anchors, kmer_size, _ptr(out, _u64p))
    if rc:
        raise LeonDnaError(rc, (lib.leon_last_error(None) or b"").decode())
    return out[:n_anchors * kmer_words(kmer_size)]


def host_anchor_dict_encode(kmers, k):
    """the dictionary stream for a list of anchors (host-only entry point; runs without a GPU).
    kmers: flat uint64 array, kmer_words(k) words per anchor."""
    lib = load_library()
    kmers = np.ascontiguousarray(kmers, dtype=np.uint64).reshape(-1)
    n = len(kmers) // kmer_words(k)
    cap = n * k + 64
    out = np.zeros(cap, dtype=np.uint8)
    size = C.c_uint64()
    rc = lib.leon_host_anchor_dict_encode(_ptr(kmers, _u64p), n, k, _ptr(out, _u8p), cap, C.byref(size))
    if rc:
        raise LeonDnaError(rc, "leon_host_anchor_dict_encode failed")
    return out[:size.value].tobytes()


def dict_piece_count(n_anchors, piece_anchors=0):
    """pieces a dictionary of n_anchors anchors is cut into (piece_anchors = 0: the default of 1024)"""
    P = piece_anchors or DICT_PIECE_ANCHORS_DEFAULT
    return (int(n_anchors) + P - 1) // P


def _dict_pieces_encode(call, kmers_arg, n_anchors, k, piece_anchors, out_cap, tail):
    """the two encode calls: (stream bytes, piece_off uint64[n_pieces + 1]); LEON_E_OVERFLOW is answered with a buffer of the size asked for"""
    lib = load_library()
    off = np.zeros(dict_piece_count(n_anchors, min(piece_anchors, DICT_PIECE_ANCHORS_MAX)) + 1, dtype=np.uint64)
    size = C.c_uint64()
    cap = int(n_anchors) * k // 3 + 64 if out_cap is None else int(out_cap)
    for _ in range(2):
        out = np.zeros(max(cap, 1), dtype=np.uint8)
        rc = call(kmers_arg, int(n_anchors), k, piece_anchors, C.c_void_p(out.ctypes.data), cap, C.c_void_p(off.ctypes.data),
                  C.c_void_p(C.addressof(size)), *tail)
        if rc != -5 or out_cap is not None:
            break
        cap = size.value
    if rc:
        err = LeonDnaError(rc, (lib.leon_last_error(None) or b"").decode())
        err.size, err.piece_off = size.value, off
        raise err
    return out[:size.value].tobytes(), off


def host_anchor_dict_encode_pieces(kmers, k, piece_anchors=0, n_threads=0, out_cap=None):
    """leon_host_anchor_dict_encode_pieces (no GPU): kmers = flat uint64 array, kmer_words(k) words per anchor"""
    lib = load_library()
    kmers = np.ascontiguousarray(kmers, dtype=np.uint64).reshape(-1)
    n = len(kmers) // kmer_words(k) if 1 <= k <= 63 else len(kmers)
    return _dict_pieces_encode(lambda *a: lib.leon_host_anchor_dict_encode_pieces(*a), C.c_void_p(kmers.ctypes.data if len(kmers) else 0), n, k,
                               piece_anchors, out_cap, (n_threads,))


def anchor_dict_encode_pieces_device(d_kmers, n_anchors, k, piece_anchors=0, device_id=0, out_cap=None):
    """leon_anchor_dict_encode_pieces_device: d_kmers = a raw device pointer (integer) to n_anchors * kmer_words(k) words"""
    lib = load_library()
    return _dict_pieces_encode(lambda kp, *a: lib.leon_anchor_dict_encode_pieces_device(device_id, kp, *a), C.c_void_p(int(d_kmers)), n_anchors, k,
                               piece_anchors, out_cap, ())


def _dict_pieces_decode(call, payload, piece_off, n_anchors, k, piece_anchors, n_pieces, out):
    lib = load_library()
    buf = np.frombuffer(bytes(payload) + b"\0", dtype=np.uint8)
    off = np.ascontiguousarray(piece_off, dtype=np.uint64)
    if n_pieces is None:
        n_pieces = len(off) - 1
    if out is None:
        out = np.zeros(max(int(n_anchors) * kmer_words(k), 1), dtype=np.uint64)
    rc = call(C.c_void_p(buf.ctypes.data), C.c_void_p(off.ctypes.data), int(n_pieces), int(n_anchors), k, piece_anchors, C.c_void_p(out.ctypes.data))
    if rc:
        raise LeonDnaError(rc, (lib.leon_last_error(None) or b"").decode())
    return out[:int(n_anchors) * kmer_words(k)]


def host_anchor_dict_decode_pieces(payload, piece_off, n_anchors, k, piece_anchors=0, n_threads=0, n_pieces=None, out=None):
    """leon_host_anchor_dict_decode_pieces (no GPU): the anchors' k-mer words; `out` (a uint64 array) is written only when every piece decodes"""
    lib = load_library()
    return _dict_pieces_decode(lambda *a: lib.leon_host_anchor_dict_decode_pieces(*a, n_threads), payload, piece_off, n_anchors, k, piece_anchors, n_pieces, out)


def anchor_dict_decode_pieces_device(payload, piece_off, n_anchors, k, piece_anchors=0, device_id=0, n_pieces=None, out=None):
    """leon_anchor_dict_decode_pieces_device: host memory in and out, the pieces decoded on the device"""
    lib = load_library()
    return _dict_pieces_decode(lambda *a: lib.leon_anchor_dict_decode_pieces_device(device_id, *a), payload, piece_off, n_anchors, k, piece_anchors, n_pieces, out)


def _join_blocks(blocks):
    """[(id, payload, n_reads)] -> (payload bytes array, offsets, n_reads array)"""
    pay = np.frombuffer(b"".join(b[1] for b in blocks) + b"\0", dtype=np.uint8)
    off = np.zeros(len(blocks) + 1, dtype=np.uint64)
    if blocks:
        off[1:] = np.cumsum([len(b[1]) for b in blocks])
    nr = np.array([b[2] for b in blocks] or [0], dtype=np.uint32)
    return pay, off, nr


def host_header_decode_blocks(blocks, first_header, n_threads=0):
    """HeaderDecoder on host threads (no GPU): blocks = [(id, payload, n_reads)] -> list of header bytes"""
    lib = load_library()
    if not blocks:
        return []
    pay, off, nr = _join_blocks(blocks)
    total = int(nr[:len(blocks)].sum())
    out_off = np.zeros(total + 1, dtype=np.uint64)
    need = C.c_uint64()
    cap = max(64, 64 * total)
    for _ in range(2):
        out = np.zeros(cap, dtype=np.uint8)
        rc = lib.leon_host_header_decode_blocks(_ptr(pay, _u8p), _ptr(off, _u64p), _ptr(nr, _u32p), len(blocks), first_header,
                                                len(first_header), _ptr(out, _u8p), cap, _ptr(out_off, _u64p), C.byref(need), n_threads)
        if rc != -5:
            break
        cap = need.value
    if rc:
        raise LeonDnaError(rc, (lib.leon_last_error(None) or b"").decode())
    raw = out.tobytes()
    return [raw[int(out_off[i]):int(out_off[i + 1])] for i in range(total)]


def host_qual_encode_blocks(quals, offsets, reads_per_block, zlib_level=-1, n_threads=0, first_block_id=0):
    """lossless quality stream: [(id, zlib payload, n_reads)] per read block (host-only)"""
    lib = load_library()
    blocks = []
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)

    def cb(user, block_id, payload, size, n_reads):
        blocks.append((block_id, C.string_at(payload, size), n_reads))
        return 0
    rc = lib.leon_host_qual_encode_blocks(bytes(quals), _ptr(offsets, _u64p), len(offsets) - 1, reads_per_block, zlib_level, n_threads,
                                          SINK(cb), None, first_block_id)
    if rc:
        raise LeonDnaError(rc, (lib.leon_last_error(None) or b"").decode())
    return blocks


def qual_deflate_blocks_device(d_quals_ptr, offsets, reads_per_block, device_id=0, first_block_id=0):
    """the lossless quality blocks written by the device (RLE deflate + dynamic Huffman): [(id, zlib payload, n_reads)];
    d_quals_ptr = device pointer to the concatenated qualities, offsets on the host"""
    lib = load_library()
    blocks = []
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)

    def cb(user, block_id, payload, size, n_reads):
        blocks.append((block_id, C.string_at(payload, size), n_reads))
        return 0
    rc = lib.leon_qual_deflate_blocks_device(device_id, C.c_void_p(int(d_quals_ptr)), _ptr(offsets, _u64p), len(offsets) - 1, reads_per_block,
                                             SINK(cb), None, first_block_id)
    if rc:
        raise LeonDnaError(rc, (lib.leon_last_error(None) or b"").decode())
    return blocks


def host_qual_decode_blocks(blocks, block_n_bytes, n_threads=0):
    lib = load_library()
    if not blocks:
        return []
    pay, off, nr = _join_blocks(blocks)
    nb = np.ascontiguousarray(block_n_bytes, dtype=np.uint64)
    total, cap = int(nr[:len(blocks)].sum()), int(nb.sum())
    out = np.zeros(cap + 1, dtype=np.uint8)
    out_off = np.zeros(total + 1, dtype=np.uint64)
    rc = lib.leon_host_qual_decode_blocks(_ptr(pay, _u8p), _ptr(off, _u64p), _ptr(nr, _u32p), _ptr(nb, _u64p), len(blocks),
                                          _ptr(out, _u8p), cap, _ptr(out_off, _u64p), n_threads)
    if rc:
        raise LeonDnaError(rc, (lib.leon_last_error(None) or b"").decode())
    raw = out.tobytes()
    return [raw[int(out_off[i]):int(out_off[i + 1])] for i in range(total)]


def qual_inflate_blocks_device(payloads, payload_off, block_n_reads, block_n_bytes, d_quals, quals_cap, d_qual_off=0, d_len=0,
                               device_id=0, n_blocks=None):
    """leon_qual_inflate_blocks_device over raw pointers: payloads (bytes-like or a uint8 array, host), payload_off / block_n_reads /
    block_n_bytes (host arrays), d_quals / d_qual_off / d_len (device pointers as integers, 0 = NULL).  Returns the literal/length
    symbols the call decoded.  None for a host array passes NULL."""
    lib = load_library()
    keep = []

    def host(a, dtype):
        if a is None:
            return C.c_void_p(0)
        if isinstance(a, np.ndarray) and a.dtype == dtype:
            keep.append(a)                       # as it lies (the tests pass odd addresses)
        else:
            keep.append(np.ascontiguousarray(np.frombuffer(bytes(a), dtype=np.uint8) if dtype == np.uint8 else a, dtype=dtype))
        return C.c_void_p(keep[-1].ctypes.data)
    if n_blocks is None:
        n_blocks = len(block_n_reads)
    n_syms = C.c_uint64()
    rc = lib.leon_qual_inflate_blocks_device(device_id, host(payloads, np.uint8), host(payload_off, np.uint64), host(block_n_reads, np.uint32),
                                             host(block_n_bytes, np.uint64), int(n_blocks), C.c_void_p(int(d_len)), C.c_void_p(int(d_quals)),
                                             int(quals_cap), C.c_void_p(int(d_qual_off)), C.byref(n_syms))
    if rc:
        raise LeonDnaError(rc, (lib.leon_last_error(None) or b"").decode())
    return n_syms.value


def qual_inflate_blocks(blocks, block_n_bytes, device_id=0):
    """the convenience form: blocks = [(id, zlib payload, n_reads)] -> (the quality bytes without newlines, offsets[total reads + 1]),
    inflated on the device and brought back"""
    pay, off, nr = _join_blocks(blocks)
    nb = np.ascontiguousarray(block_n_bytes, dtype=np.uint64)
    total, cap = int(nr[:len(blocks)].sum()), int(nb.sum())
    d_q, d_o = device_alloc(cap + 64, device_id), device_alloc((total + 1) * 8, device_id)
    try:
        qual_inflate_blocks_device(pay, off, nr, nb, d_q, cap, d_o, 0, device_id, n_blocks=len(blocks))
        quals = device_download(d_q, cap, device_id) if cap else b""
        offsets = np.frombuffer(device_download(d_o, (total + 1) * 8, device_id), dtype=np.uint64) if blocks else np.zeros(1, np.uint64)
        return quals, offsets
    finally:
        device_free(d_q)
        device_free(d_o)


def _crc32_args(seg_off, n_seg):
    """seg_off (None = NULL) as a uint64 array, the count of segments and the host words the call fills"""
    off = None if seg_off is None else np.ascontiguousarray(seg_off, dtype=np.uint64)
    if n_seg is None:
        n_seg = 0 if off is None else max(len(off) - 1, 0)
    return off, int(n_seg), np.zeros(max(int(n_seg), 1), dtype=np.uint32)


def crc32_segments_device(d_bytes, n_bytes, seg_off, device_id=0, n_seg=None, null_crc=False):
    """leon_crc32_segments_device: zlib's CRC-32 of every segment [seg_off[s], seg_off[s + 1]) of the n_bytes at the device pointer
    d_bytes (an integer, 0 = NULL), as a uint32 array.  seg_off is a host array (None passes NULL, as null_crc does for the result)."""
    lib = load_library()
    off, n_seg, crc = _crc32_args(seg_off, n_seg)
    rc = lib.leon_crc32_segments_device(device_id, C.c_void_p(int(d_bytes)), int(n_bytes), C.c_void_p(0 if off is None else off.ctypes.data), n_seg,
                                        C.c_void_p(0 if null_crc else crc.ctypes.data))
    if rc:
        raise LeonDnaError(rc, (lib.leon_last_error(None) or b"").decode())
    return crc[:n_seg]


def host_crc32_segments(data, seg_off, n_threads=0, n_bytes=None, n_seg=None, null_crc=False):
    """leon_host_crc32_segments (no GPU): data is bytes-like or a uint8 array (None passes NULL), the rest as crc32_segments_device"""
    lib = load_library()
    buf = None if data is None else (data if isinstance(data, np.ndarray) and data.dtype == np.uint8 else np.frombuffer(bytes(data) + b"\0", dtype=np.uint8))
    if n_bytes is None:
        n_bytes = 0 if data is None else len(data)
    off, n_seg, crc = _crc32_args(seg_off, n_seg)
    rc = lib.leon_host_crc32_segments(C.c_void_p(0 if buf is None else buf.ctypes.data), int(n_bytes), C.c_void_p(0 if off is None else off.ctypes.data),
                                      n_seg, n_threads, C.c_void_p(0 if null_crc else crc.ctypes.data))
    if rc:
        raise LeonDnaError(rc, (lib.leon_last_error(None) or b"").decode())
    return crc[:n_seg]


BGZF_WHOLE, BGZF_PARTIAL, BGZF_TRUNCATED, BGZF_FOREIGN = 0, 1, 2, 3


def _host_bytes(data):
    """bytes-like or a uint8 array (used as it lies) as a uint8 array that is never empty; None stays None"""
    if data is None:
        return None
    if isinstance(data, np.ndarray) and data.dtype == np.uint8:
        return data
    return np.frombuffer(bytes(data) + b"\0", dtype=np.uint8)


def host_bgzf_members(data, last=False, off_cap=None, n_bytes=None):
    """leon_host_bgzf_members (no GPU) over data[:n_bytes]: a dict of rc, message, member_off (the members' first bytes and the end of
    the last whole one), n_text, consumed and stop (BGZF_*).  off_cap: the entries the table has room for (default: enough)."""
    lib = load_library()
    buf = _host_bytes(data)
    if n_bytes is None:
        n_bytes = 0 if data is None else len(data)
    if off_cap is None:
        off_cap = n_bytes // 20 + 2
    off = np.zeros(max(off_cap, 1), dtype=np.uint64)
    n, text, used, stop = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_uint32()
    rc = lib.leon_host_bgzf_members(C.c_void_p(0 if buf is None else buf.ctypes.data), int(n_bytes), int(last), C.c_void_p(off.ctypes.data if off_cap else 0),
                                    int(off_cap), C.byref(n), C.byref(text), C.byref(used), C.byref(stop))
    return {"rc": rc, "message": (lib.leon_last_error(None) or b"").decode() if rc else "", "member_off": off[:min(n.value + 1, off_cap)].copy(),
            "n_members": n.value, "n_text": text.value, "consumed": used.value, "stop": stop.value}


def host_bgzf_inflate(data, member_off, n_threads=0, text_cap=None, n_members=None, n_bytes=None):
    """leon_host_bgzf_inflate (no GPU): the members' text as bytes.  text_cap: the room given (default: 65 536 bytes per member)"""
    lib = load_library()
    buf = _host_bytes(data)
    off = None if member_off is None else np.ascontiguousarray(member_off, dtype=np.uint64)
    if n_members is None:
        n_members = 0 if off is None else max(len(off) - 1, 0)
    if n_bytes is None:
        n_bytes = 0 if data is None else len(data)
    if text_cap is None:
        text_cap = 65536 * n_members
    text = np.zeros(text_cap + 1, dtype=np.uint8)
    n_text = C.c_uint64()
    rc = lib.leon_host_bgzf_inflate(C.c_void_p(0 if buf is None else buf.ctypes.data), int(n_bytes), C.c_void_p(0 if off is None else off.ctypes.data),
                                    int(n_members), C.c_void_p(text.ctypes.data), int(text_cap), C.byref(n_text), n_threads)
    if rc:
        err = LeonDnaError(rc, (lib.leon_last_error(None) or b"").decode())
        err.n_text = n_text.value
        raise err
    return text[:n_text.value].tobytes()


def bgzf_inflate_device(data, member_off, d_text, text_cap, device_id=0, max_members_per_launch=0, n_members=None, n_bytes=None):
    """leon_bgzf_inflate_device: data and member_off on the host, d_text a device pointer (an integer, 0 = NULL) with room for text_cap
    bytes.  Returns (bytes of text, literal/length symbols decoded)."""
    lib = load_library()
    buf = _host_bytes(data)
    off = None if member_off is None else np.ascontiguousarray(member_off, dtype=np.uint64)
    if n_members is None:
        n_members = 0 if off is None else max(len(off) - 1, 0)
    if n_bytes is None:
        n_bytes = 0 if data is None else len(data)
    n_text, n_syms = C.c_uint64(), C.c_uint64()
    rc = lib.leon_bgzf_inflate_device(device_id, C.c_void_p(0 if buf is None else buf.ctypes.data), int(n_bytes), C.c_void_p(0 if off is None else off.ctypes.data),
                                      int(n_members), C.c_void_p(int(d_text)), int(text_cap), C.byref(n_text), int(max_members_per_launch), C.byref(n_syms))
    if rc:
        err = LeonDnaError(rc, (lib.leon_last_error(None) or b"").decode())
        err.n_text = n_text.value
        raise err
    return n_text.value, n_syms.value


def letters_count_device(d_bases, n_bytes, device_id=0):
    """leon_letters_count_device: (lower-case runs, bytes outside ACGTN) of the n_bytes at the device pointer d_bases (an integer)"""
    lib = load_library()
    n_runs, n_odd = C.c_uint64(), C.c_uint64()
    rc = lib.leon_letters_count_device(device_id, C.c_void_p(int(d_bases)), int(n_bytes), C.byref(n_runs), C.byref(n_odd))
    if rc:
        raise LeonDnaError(rc, (lib.leon_last_error(None) or b"").decode())
    return n_runs.value, n_odd.value


def letters_take_device(d_bases, n_bytes, n_runs, n_odd, device_id=0, slack=0, fill=0):
    """leon_letters_take_device: folds the buffer in place; (runs as an (n_runs, 2) uint64 array, odd_pos, odd_byte).  With `slack` the
    three host arrays are that many elements longer, filled with `fill`, and come back whole: what lies behind the tables is the
    caller's to inspect."""
    lib = load_library()
    runs = np.full(2 * (n_runs + slack) + 1, fill, dtype=np.uint64)
    pos = np.full(n_odd + slack + 1, fill, dtype=np.uint64)
    byte = np.full(n_odd + slack + 1, fill, dtype=np.uint8)
    rc = lib.leon_letters_take_device(device_id, C.c_void_p(int(d_bases)), int(n_bytes), C.c_void_p(runs.ctypes.data), int(n_runs), C.c_void_p(pos.ctypes.data),
                                      C.c_void_p(byte.ctypes.data), int(n_odd))
    if rc:
        err = LeonDnaError(rc, (lib.leon_last_error(None) or b"").decode())
        err.tables = (runs, pos, byte)
        raise err
    if slack:
        return runs, pos, byte
    return runs[:2 * n_runs].reshape(-1, 2), pos[:n_odd], byte[:n_odd]


def _letters_tables(runs, odd_pos, odd_byte, n_runs, n_odd):
    """the tables (None = NULL) as contiguous arrays, and the counts the call is given"""
    r = None if runs is None else np.ascontiguousarray(runs, dtype=np.uint64).reshape(-1)
    p = None if odd_pos is None else np.ascontiguousarray(odd_pos, dtype=np.uint64)
    b = None if odd_byte is None else np.ascontiguousarray(odd_byte, dtype=np.uint8)
    n_runs = (0 if r is None else len(r) // 2) if n_runs is None else int(n_runs)
    n_odd = (0 if p is None else len(p)) if n_odd is None else int(n_odd)
    at = lambda a: C.c_void_p(0 if a is None or not len(a) else a.ctypes.data)
    return (r, p, b), (at(r), n_runs, at(p), at(b), n_odd)


def letters_apply_device(d_bases, n_bytes, runs, odd_pos, odd_byte, device_id=0, n_runs=None, n_odd=None):
    """leon_letters_apply_device on the n_bytes at the device pointer d_bases (an integer, 0 = NULL); the tables are host arrays (None
    passes NULL; n_runs / n_odd override the counts)"""
    lib = load_library()
    keep, (r, nr, p, b, no) = _letters_tables(runs, odd_pos, odd_byte, n_runs, n_odd)
    rc = lib.leon_letters_apply_device(device_id, C.c_void_p(int(d_bases)), int(n_bytes), r, nr, p, b, no)
    if rc:
        raise LeonDnaError(rc, (lib.leon_last_error(None) or b"").decode())


def host_letters_apply(bases, runs, odd_pos, odd_byte, n_threads=0, n_bytes=None, n_runs=None, n_odd=None):
    """leon_host_letters_apply (no GPU) on a writable uint8 array (None passes NULL), in place; the rest as letters_apply_device"""
    lib = load_library()
    keep, (r, nr, p, b, no) = _letters_tables(runs, odd_pos, odd_byte, n_runs, n_odd)
    if n_bytes is None:
        n_bytes = 0 if bases is None else len(bases)
    rc = lib.leon_host_letters_apply(C.c_void_p(0 if bases is None or not len(bases) else bases.ctypes.data), int(n_bytes), r, nr, p, b, no, n_threads)
    if rc:
        raise LeonDnaError(rc, (lib.leon_last_error(None) or b"").decode())


def kmer_auto_cutoff(histogram):
    lib = load_library()
    h = np.ascontiguousarray(histogram, dtype=np.uint64)
    assert len(h) == 256
    out = C.c_uint32()
    rc = lib.leon_kmer_auto_cutoff(_ptr(h, _u64p), C.byref(out))
    if rc:
        raise LeonDnaError(rc, "leon_kmer_auto_cutoff failed")
    return out.value


def kmer_solid(bases, offsets, k, min_abundance, device_id=0, with_histogram=False, max_keys_per_pass=0):
    """solid canonical k-mers of the reads, counted on the device (host arrays in and out); flat uint64, kmer_words(k) each"""
    lib = load_library()
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    if not isinstance(bases, (bytes, bytearray)):
        bases = np.ascontiguousarray(bases, dtype=np.uint8).tobytes()
    w = kmer_words(k)
    hist = np.zeros(256, dtype=np.uint64)
    ns = C.c_uint64()
    cap = max(int(offsets[-1] - offsets[0]), 1)
    out = np.zeros(cap * w, dtype=np.uint64)
    rc = lib.leon_kmer_solid(device_id, bases, _ptr(offsets, _u64p), n, k, min_abundance, int(max_keys_per_pass),
                             _ptr(out, _u64p), cap, C.byref(ns), _ptr(hist, _u64p))
    if rc:
        raise LeonDnaError(rc, (lib.leon_last_error(None) or b"").decode())
    res = out[:ns.value * w].copy()
    return (res, hist) if with_histogram else res


def kmer_solid_device(d_bases_ptr, d_offsets_ptr, n_reads, k, min_abundance, device_id=0, max_keys_per_pass=0):
    """device arrays in, device array out: returns (device pointer, n_solid); free with device_free()"""
    lib = load_library()
    p, ns = C.c_void_p(), C.c_uint64()
    rc = lib.leon_kmer_solid_device(device_id, C.c_void_p(int(d_bases_ptr)), C.c_void_p(int(d_offsets_ptr)), int(n_reads), k,
                                    min_abundance, int(max_keys_per_pass), C.byref(p), C.byref(ns), None)
    if rc:
        raise LeonDnaError(rc, (lib.leon_last_error(None) or b"").decode())
    return p.value, ns.value


def device_free(ptr):
    if ptr:
        load_library().leon_device_free(C.c_void_p(int(ptr)))


def device_trim():
    """return the device memory the library parks between calls (the k-mer counter's ~22 GB of sort buffers after a large count) to the
    driver: for hosts that go on allocating through torch or their own hipMalloc with no context's leon_dna_reserve in between"""
    load_library().leon_device_trim()


def device_copy(d_dst, d_src, n_bytes, device_id=0):
    """device to device, n_bytes from d_src to d_dst (raw device pointers)"""
    rc = load_library().leon_device_copy(device_id, C.c_void_p(int(d_dst)), C.c_void_p(int(d_src)), int(n_bytes))
    if rc:
        raise LeonDnaError(rc, (load_library().leon_last_error(None) or b"").decode())


def device_upload_bytes(data, device_id=0):
    """a new device buffer holding `data` (bytes-like); the caller frees it with device_free"""
    lib = load_library()
    data = bytes(data)
    p = C.c_void_p()
    rc = lib.leon_device_alloc(device_id, len(data) + 64, C.byref(p))
    if rc == 0 and data:
        rc = lib.leon_device_upload(device_id, p, C.c_char_p(data), len(data))
    if rc:
        raise LeonDnaError(rc, (lib.leon_last_error(None) or b"").decode())
    return p.value


def device_count():
    """leon_device_count: the HIP devices the library sees; 0 when it sees none (or cannot ask)"""
    n = C.c_int(0)
    return n.value if load_library().leon_device_count(C.byref(n)) == 0 and n.value > 0 else 0


def host_pinned_alloc(n_bytes, device_id=0):
    """leon_host_pinned_alloc: page-locked host memory as an integer address; the caller frees it with host_pinned_free"""
    lib = load_library()
    p = C.c_void_p()
    rc = lib.leon_host_pinned_alloc(device_id, int(n_bytes), C.byref(p))
    if rc:
        raise LeonDnaError(rc, (lib.leon_last_error(None) or b"").decode())
    return p.value


def host_pinned_free(ptr):
    """leon_host_pinned_free (0 / None passes NULL, which is allowed)"""
    load_library().leon_host_pinned_free(C.c_void_p(int(ptr or 0)))


def device_download_to(host_ptr, d_ptr, n_bytes, device_id=0):
    """leon_device_download into the host memory at the integer address host_ptr (a pinned buffer: one direct copy)"""
    lib = load_library()
    rc = lib.leon_device_download(device_id, C.c_void_p(int(host_ptr)), C.c_void_p(int(d_ptr)), int(n_bytes))
    if rc:
        raise LeonDnaError(rc, (lib.leon_last_error(None) or b"").decode())


def device_alloc(n_bytes, device_id=0):
    """plain device memory (leon_device_alloc); the caller frees it with device_free"""
    lib = load_library()
    p = C.c_void_p()
    rc = lib.leon_device_alloc(device_id, int(n_bytes), C.byref(p))
    if rc:
        raise LeonDnaError(rc, (lib.leon_last_error(None) or b"").decode())
    return p.value


def device_download(d_ptr, n_bytes, device_id=0):
    """n_bytes from a raw device pointer, as bytes"""
    lib = load_library()
    out = np.zeros(max(int(n_bytes), 1), dtype=np.uint8)
    rc = lib.leon_device_download(device_id, C.c_void_p(out.ctypes.data), C.c_void_p(int(d_ptr)), int(n_bytes))
    if rc:
        raise LeonDnaError(rc, (lib.leon_last_error(None) or b"").decode())
    return out[:int(n_bytes)].tobytes()


def device_download_pieces(d_ptr, n_bytes, sink, device_id=0):
    """leon_device_download_pieces: sink(offset, address, size) -> 0 to go on, called with every pinned piece where it landed -- in no
    particular order and from several threads at once"""
    lib = load_library()
    raised = []

    def thunk(user, offset, address, size):
        try:
            return int(sink(int(offset), int(address or 0), int(size)) or 0)
        except Exception as e:                         # noqa: BLE001 -- nothing may cross the C boundary
            raised.append(e)
            return 1
    rc = lib.leon_device_download_pieces(device_id, C.c_void_p(int(d_ptr)), int(n_bytes), PIECE_SINK(thunk), None)
    if rc:
        err = LeonDnaError(rc, (lib.leon_last_error(None) or b"").decode())
        if raised:
            raise err from raised[0]
        raise err


BGZF_MEMBER_TEXT = 32768     # LEON_BGZF_MEMBER_TEXT
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def text_bgzf_device(d_text, n_text, last=1, device_id=0, sink=None):
    """leon_text_bgzf_device: the n_text bytes at the device pointer d_text (an integer, 0 = NULL) as BGZF.  Returns (bytes of this call's
    output, n_taken, n_members); the pieces are collected into one bytes object, every offset checked to arrive once.  sink (tests): called
    as sink(offset, size) before a piece is kept, non-zero stops the call."""
    lib = load_library()
    pieces, raised = [], []
    lock = threading.Lock()

    def thunk(user, offset, address, size):
        try:
            if sink is not None:
                rc = int(sink(int(offset), int(size)) or 0)
                if rc:
                    return rc
            data = C.string_at(address, size) if size else b""
            with lock:
                pieces.append((int(offset), data))
            return 0
        except Exception as e:                         # noqa: BLE001 -- nothing may cross the C boundary
            raised.append(e)
            return 1
    taken, out_bytes, members = C.c_uint64(), C.c_uint64(), C.c_uint64()
    rc = lib.leon_text_bgzf_device(device_id, C.c_void_p(int(d_text) if d_text else 0), int(n_text), int(last), PIECE_SINK(thunk), None,
                                   C.byref(taken), C.byref(out_bytes), C.byref(members))
    if rc:
        err = LeonDnaError(rc, (lib.leon_last_error(None) or b"").decode())
        if raised:
            raise err from raised[0]
        raise err
    pieces.sort()
    at = 0
    for off, data in pieces:
        if off != at:
            raise LeonDnaError(-5, "leon_text_bgzf_device: the pieces do not tile the output (offset %d, expected %d)" % (off, at))
        at += len(data)
    if at != out_bytes.value:
        raise LeonDnaError(-5, "leon_text_bgzf_device: %d bytes delivered, out_bytes = %d" % (at, out_bytes.value))
    return b"".join(d for _, d in pieces), taken.value, members.value


def bgzf_members_bound(n_text):
    """the most members leon_text_bgzf_records_device writes for n_text bytes (head included)"""
    return 3 * (int(n_text) // BGZF_MEMBER_TEXT) + 2


BGZF_F_MATCHES = 1           # LEON_BGZF_F_MATCHES


def text_bgzf_device_ex(d_text, n_head, n_body, d_rec_off, n_records, flags=0, **kw):
    """leon_text_bgzf_device_ex: text_bgzf_records_device's arguments and results, with the encoder chosen by flags (BGZF_F_MATCHES:
    k_deflate_lz_chunks; 0: the bytes of text_bgzf_records_device)."""
    return text_bgzf_records_device(d_text, n_head, n_body, d_rec_off, n_records, _flags=int(flags), **kw)


def text_bgzf_records_device(d_text, n_head, n_body, d_rec_off, n_records, last=1, device_id=0, sink=None, member_out=None, member_text=None,
                             members_cap=None, tables=True, null=(), _flags=None):
    """leon_text_bgzf_records_device: n_head + n_body bytes at the device pointer d_text as BGZF with members cut at the record starts
    d_rec_off[0 .. n_records] (a device pointer; 0 = NULL, with no records and no head: the fixed cuts).  Returns (bytes of this call's
    output, n_taken, n_members, member_out_off, member_text_off); the pieces are collected as text_bgzf_device collects them.
    tables: give the call member tables (of bgzf_members_bound entries, or members_cap); member_out / member_text: uint64 arrays of the
    caller's to use instead (either may be None: the pointer is NULL).  null (tests): names among 'sink', 'n_taken', 'out_bytes',
    'n_members' passed as NULL.  A failed call raises LeonDnaError; its n_members attribute holds what the call left there."""
    lib = load_library()
    pieces, raised = [], []
    lock = threading.Lock()

    def thunk(user, offset, address, size):
        try:
            if sink is not None:
                rc = int(sink(int(offset), int(size)) or 0)
                if rc:
                    return rc
            data = C.string_at(address, size) if size else b""
            with lock:
                pieces.append((int(offset), data))
            return 0
        except Exception as e:                         # noqa: BLE001 -- nothing may cross the C boundary
            raised.append(e)
            return 1
    if member_out is None and member_text is None and tables:
        cap = bgzf_members_bound(n_head + n_body) if members_cap is None else int(members_cap)
        member_out, member_text = np.zeros(max(cap, 1), dtype=np.uint64), np.zeros(max(cap, 1), dtype=np.uint64)
        members_cap = cap
    if members_cap is None:
        members_cap = 0 if member_out is None and member_text is None else min(len(a) for a in (member_out, member_text) if a is not None)
    for a in (member_out, member_text):
        assert a is None or (a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"])
    taken, out_bytes, members = C.c_uint64(), C.c_uint64(), C.c_uint64()
    vp = lambda a: C.c_void_p(0 if a is None else a.ctypes.data)
    name = "leon_text_bgzf_records_device" if _flags is None else "leon_text_bgzf_device_ex"             # (_flags: text_bgzf_device_ex's)
    rc = getattr(lib, name)(device_id, C.c_void_p(int(d_text) if d_text else 0), int(n_head), int(n_body),
                            C.c_void_p(int(d_rec_off) if d_rec_off else 0), int(n_records), int(last),
                            None if "sink" in null else PIECE_SINK(thunk), None,
                            None if "n_taken" in null else C.byref(taken), None if "out_bytes" in null else C.byref(out_bytes),
                            vp(member_out), vp(member_text), int(members_cap), None if "n_members" in null else C.byref(members),
                            *(() if _flags is None else (C.c_uint32(_flags),)))
    if rc:
        err = LeonDnaError(rc, (lib.leon_last_error(None) or b"").decode())
        err.n_members = members.value
        if raised:
            raise err from raised[0]
        raise err
    pieces.sort()
    at = 0
    for off, data in pieces:
        if off != at:
            raise LeonDnaError(-5, "%s: the pieces do not tile the output (offset %d, expected %d)" % (name, off, at))
        at += len(data)
    if at != out_bytes.value:
        raise LeonDnaError(-5, "%s: %d bytes delivered, out_bytes = %d" % (name, at, out_bytes.value))
    n = members.value
    return (b"".join(d for _, d in pieces), taken.value, n, None if member_out is None else member_out[:n].copy(),
            None if member_text is None else member_text[:n].copy())


def host_bgzf_record_cuts(rec_off, n_head=0, last=1, cap=None, n_records=None, tables=True):
    """leon_host_bgzf_record_cuts (no GPU): the members of n_head bytes of head and a body whose records start at rec_off (n_records + 1
    entries, or None: a head alone).  Returns (begin, len, n_taken): every member's offset in the call's text and its bytes.  cap: the
    entries the tables have room for (default: enough); tables=False: count only, returns (n_members, n_taken)."""
    lib = load_library()
    off = None if rec_off is None else np.ascontiguousarray(rec_off, dtype=np.uint64)
    if n_records is None:
        n_records = 0 if off is None else len(off) - 1
    n_body = 0 if off is None or not len(off) else int(off[min(n_records, len(off) - 1)])
    if cap is None:
        cap = bgzf_members_bound(n_head + n_body) if tables else 0
    begin, length = np.zeros(max(cap, 1), dtype=np.uint64), np.zeros(max(cap, 1), dtype=np.uint32)
    n, taken = C.c_uint64(), C.c_uint64()
    rc = lib.leon_host_bgzf_record_cuts(C.c_void_p(0 if off is None else off.ctypes.data), int(n_records), int(n_head), int(last),
                                        C.c_void_p(begin.ctypes.data if tables else 0), C.c_void_p(length.ctypes.data if tables else 0), int(cap),
                                        C.byref(n), C.byref(taken))
    if rc:
        err = LeonDnaError(rc, (lib.leon_last_error(None) or b"").decode())
        err.n_members = n.value
        raise err
    if not tables:
        return n.value, taken.value
    return begin[:n.value].copy(), length[:n.value].copy(), taken.value


def fastq_split_device(d_text, n_text, last, max_records, plus_kind, d_headers, d_header_off, d_bases, d_base_off, d_quals, bytes_cap, records_cap,
                       device_id=0):
    """leon_fastq_split_device over raw device pointers (integers).  Returns the result's fields as a dict; a LeonDnaError carries them
    as .result (LEON_E_OVERFLOW: what the call needs)"""
    lib = load_library()
    res = FastqSplitResult()
    rc = lib.leon_fastq_split_device(device_id, C.c_void_p(int(d_text)), int(n_text), int(last), int(max_records), int(plus_kind), C.c_void_p(int(d_headers)),
                                     C.c_void_p(int(d_header_off)), C.c_void_p(int(d_bases)), C.c_void_p(int(d_base_off)), C.c_void_p(int(d_quals)),
                                     int(bytes_cap), int(records_cap), C.byref(res))
    if rc:
        err = LeonDnaError(rc, (lib.leon_last_error(None) or b"").decode())
        err.result = res.as_dict()
        raise err
    return res.as_dict()


def host_fastq_split(text, last=1, max_records=1 << 62, plus_kind=-1, bytes_cap=None, records_cap=None):
    """leon_host_fastq_split (no GPU): text is bytes-like.  Returns (result dict, headers, header_off, bases, base_off, quals): the blobs as
    bytes, the offsets as uint64 arrays of n_records + 1 entries.  bytes_cap / records_cap default to what never overflows"""
    lib = load_library()
    buf = np.frombuffer(bytes(text) + b"\0", dtype=np.uint8)
    n_text = len(buf) - 1
    bytes_cap = n_text if bytes_cap is None else int(bytes_cap)
    records_cap = n_text // 4 + 2 if records_cap is None else int(records_cap)
    blobs = [np.zeros(bytes_cap + 1, dtype=np.uint8) for _ in range(3)]
    offs = [np.zeros(records_cap + 1, dtype=np.uint64) for _ in range(2)]
    res = FastqSplitResult()
    rc = lib.leon_host_fastq_split(C.c_void_p(buf.ctypes.data), n_text, int(last), int(max_records), int(plus_kind), C.c_void_p(blobs[0].ctypes.data),
                                   C.c_void_p(offs[0].ctypes.data), C.c_void_p(blobs[1].ctypes.data), C.c_void_p(offs[1].ctypes.data),
                                   C.c_void_p(blobs[2].ctypes.data), bytes_cap, records_cap, C.byref(res))
    if rc:
        err = LeonDnaError(rc, (lib.leon_last_error(None) or b"").decode())
        err.result = res.as_dict()
        raise err
    r = res.as_dict()
    n = r["n_records"]
    return (r, blobs[0][:r["header_bytes"]].tobytes(), offs[0][:n + 1].copy(), blobs[1][:r["base_bytes"]].tobytes(), offs[1][:n + 1].copy(),
            blobs[2][:r["base_bytes"]].tobytes())


def fasta_split_device(d_text, n_text, last, max_records, wrap, d_headers, d_header_off, d_bases, d_base_off, bytes_cap, records_cap, device_id=0):
    """leon_fasta_split_device over raw device pointers (integers); wrap: 0, the line width, or FASTA_ANY_WIDTH.  Returns the result's
    fields as a dict; a LeonDnaError carries them as .result (LEON_E_OVERFLOW: what the call needs)"""
    lib = load_library()
    res = FastaSplitResult()
    rc = lib.leon_fasta_split_device(device_id, C.c_void_p(int(d_text)), int(n_text), int(last), int(max_records), int(wrap), C.c_void_p(int(d_headers)),
                                     C.c_void_p(int(d_header_off)), C.c_void_p(int(d_bases)), C.c_void_p(int(d_base_off)), int(bytes_cap), int(records_cap),
                                     C.byref(res))
    if rc:
        err = LeonDnaError(rc, (lib.leon_last_error(None) or b"").decode())
        err.result = res.as_dict()
        raise err
    return res.as_dict()


def host_fasta_split(text, last=1, max_records=1 << 62, wrap=FASTA_ANY_WIDTH, bytes_cap=None, records_cap=None):
    """leon_host_fasta_split (no GPU): text is bytes-like.  Returns (result dict, headers, header_off, bases, base_off): the blobs as bytes,
    the offsets as uint64 arrays of n_records + 1 entries.  bytes_cap / records_cap default to what never overflows"""
    lib = load_library()
    buf = np.frombuffer(bytes(text) + b"\0", dtype=np.uint8)
    n_text = len(buf) - 1
    bytes_cap = n_text if bytes_cap is None else int(bytes_cap)
    records_cap = n_text // 2 + 2 if records_cap is None else int(records_cap)
    blobs = [np.zeros(bytes_cap + 1, dtype=np.uint8) for _ in range(2)]
    offs = [np.zeros(records_cap + 1, dtype=np.uint64) for _ in range(2)]
    res = FastaSplitResult()
    rc = lib.leon_host_fasta_split(C.c_void_p(buf.ctypes.data), n_text, int(last), int(max_records), int(wrap), C.c_void_p(blobs[0].ctypes.data),
                                   C.c_void_p(offs[0].ctypes.data), C.c_void_p(blobs[1].ctypes.data), C.c_void_p(offs[1].ctypes.data), bytes_cap, records_cap,
                                   C.byref(res))
    if rc:
        err = LeonDnaError(rc, (lib.leon_last_error(None) or b"").decode())
        err.result = res.as_dict()
        raise err
    r = res.as_dict()
    n = r["n_records"]
    return r, blobs[0][:r["header_bytes"]].tobytes(), offs[0][:n + 1].copy(), blobs[1][:r["base_bytes"]].tobytes(), offs[1][:n + 1].copy()


def records_format_device(d_bases, d_len, n_reads, n_bases, d_text, text_cap, lead=b"@", fastq=True, plus_kind=0, wrap=0, first_read_index=0,
                          d_hdr_text=None, d_hdr_off=None, hdr_bytes=0, d_quals=None, d_rec_off=None, device_id=0, struct_size=None):
    """leon_records_format_device over raw device pointers: the reads' FASTA / FASTQ text into d_text.  Returns the text's size;
    a LeonDnaError carries .text_size (the bytes needed) when the capacity was too small"""
    lib = load_library()
    lay = RecordLayout()
    lay.struct_size = C.sizeof(RecordLayout) if struct_size is None else struct_size
    lay.lead, lay.fastq, lay.plus_kind, lay.wrap = lead[0], 1 if fastq else 0, plus_kind, wrap
    lay.first_read_index, lay.hdr_bytes = int(first_read_index), int(hdr_bytes)
    size = C.c_uint64()
    vp = lambda p: C.c_void_p(int(p)) if p else None
    rc = lib.leon_records_format_device(device_id, C.byref(lay), vp(d_bases), vp(d_len), int(n_reads), int(n_bases), vp(d_hdr_text), vp(d_hdr_off),
                                        vp(d_quals), vp(d_text), int(text_cap), vp(d_rec_off), C.byref(size))
    if rc:
        err = LeonDnaError(rc, (lib.leon_last_error(None) or b"").decode())
        err.text_size = int(size.value)
        raise err
    return int(size.value)


def _bam_layout(fastq, first_read_index, hdr_bytes, struct_size):
    lay = RecordLayout()
    lay.struct_size = C.sizeof(RecordLayout) if struct_size is None else struct_size
    lay.lead, lay.fastq = (b"@" if fastq else b">")[0], 1 if fastq else 0
    lay.first_read_index, lay.hdr_bytes = int(first_read_index), int(hdr_bytes)
    return lay


def records_bam_device(d_bases, d_len, n_reads, n_bases, d_out, out_cap, fastq=True, first_read_index=0, d_hdr_text=None, d_hdr_off=None,
                       hdr_bytes=0, d_quals=None, d_rec_off=None, device_id=0, struct_size=None):
    """leon_records_bam_device over raw device pointers: the reads as unaligned BAM records into d_out.  Returns the records' size;
    a LeonDnaError carries .out_size (the bytes needed) when the capacity was too small"""
    lib = load_library()
    lay = _bam_layout(fastq, first_read_index, hdr_bytes, struct_size)
    size = C.c_uint64()
    vp = lambda p: C.c_void_p(int(p)) if p else None
    rc = lib.leon_records_bam_device(device_id, C.byref(lay), vp(d_bases), vp(d_len), int(n_reads), int(n_bases), vp(d_hdr_text), vp(d_hdr_off),
                                     vp(d_quals), vp(d_out), int(out_cap), vp(d_rec_off), C.byref(size))
    if rc:
        err = LeonDnaError(rc, (lib.leon_last_error(None) or b"").decode())
        err.out_size = int(size.value)
        raise err
    return int(size.value)


def host_records_bam(bases, lens, n_bases=None, fastq=True, first_read_index=0, hdr_text=None, hdr_off=None, hdr_bytes=None, quals=None, out_cap=None,
                     n_threads=1, struct_size=None):
    """leon_host_records_bam (no GPU): bases / hdr_text / quals bytes-like (hdr_text, quals may be None), lens the reads' lengths, hdr_off
    n_reads + 1 offsets whose first entry is hdr_text's first byte.  out_cap None: sized by a first call.  Returns (records as bytes,
    rec_off as a uint64 array of n_reads + 1 entries); a LeonDnaError carries .out_size"""
    lib = load_library()
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    n = len(lens)
    lens_buf = np.concatenate([lens, np.zeros(1, dtype=np.uint32)])
    b = np.frombuffer(bytes(bases) + b"\0", dtype=np.uint8)
    h = None if hdr_text is None else np.frombuffer(bytes(hdr_text) + b"\0", dtype=np.uint8)
    ho = None if hdr_off is None else np.ascontiguousarray(hdr_off, dtype=np.uint64)
    q = None if quals is None else np.frombuffer(bytes(quals) + b"\0", dtype=np.uint8)
    if hdr_bytes is None:
        hdr_bytes = 0 if h is None else len(h) - 1
    lay = _bam_layout(fastq, first_read_index, hdr_bytes, struct_size)
    n_bases = len(b) - 1 if n_bases is None else int(n_bases)
    vp = lambda a: C.c_void_p(0 if a is None else a.ctypes.data)
    size = C.c_uint64()

    def call(out, cap, rec):
        rc = lib.leon_host_records_bam(C.byref(lay), vp(b), vp(lens_buf), n, n_bases, vp(h), vp(ho), vp(q), vp(out), int(cap), vp(rec), C.byref(size),
                                       int(n_threads))
        if rc:
            err = LeonDnaError(rc, (lib.leon_last_error(None) or b"").decode())
            err.out_size = int(size.value)
            raise err
    if out_cap is None:
        try:
            call(None, 0, None)
            out_cap = 0
        except LeonDnaError as e:
            if e.code != -5:
                raise
            out_cap = e.out_size
    out = np.full(int(out_cap) + 1, 0xA5, dtype=np.uint8)
    rec = np.zeros(n + 1, dtype=np.uint64)
    call(out, out_cap, rec)
    assert out[size.value:].tobytes() == b"\xa5" * (len(out) - size.value), "leon_host_records_bam wrote past the size it reports"
    return out[:size.value].tobytes(), rec


def bam_header():
    """leon_bam_header: the bytes a BAM file's uncompressed content begins with"""
    lib = load_library()
    size = C.c_uint64()
    out = np.zeros(256, dtype=np.uint8)
    rc = lib.leon_bam_header(C.c_void_p(out.ctypes.data), len(out), C.byref(size))
    if rc:
        raise LeonDnaError(rc, (lib.leon_last_error(None) or b"").decode())
    return out[:size.value].tobytes()


class DnaEncodeContext:
    """One ordered read stream on one GPU (wraps leon_dna_ctx)."""

    def __init__(self, kmer_size=31, reads_per_block=50000, bloom_tai=0, bloom_n_hash=7, bloom_block_nbits=12,
                 device_id=0, resolve_window=0, keep_trace=False, random_values=None, dict_on_device=False, dict_pieces=False,
                 dict_piece_anchors=0):
        self.lib = load_library()
        cfg = _Cfg()
        cfg.struct_size = C.sizeof(_Cfg)
        cfg.kmer_size, cfg.reads_per_block = kmer_size, reads_per_block
        cfg.bloom_n_hash, cfg.bloom_block_nbits, cfg.device_id = bloom_n_hash, bloom_block_nbits, device_id
        cfg.bloom_tai, cfg.resolve_window = int(bloom_tai), int(resolve_window)
        cfg.flags = (LEON_F_KEEP_TRACE if keep_trace else 0) | (LEON_F_DICT_ON_DEVICE if dict_on_device else 0) | \
            (LEON_F_DICT_PIECES if dict_pieces else 0)
        cfg.dict_piece_anchors = dict_piece_anchors
        self._rv = None
        if random_values is not None:
            self._rv = np.ascontiguousarray(random_values, dtype=np.uint64)
            assert len(self._rv) == 256
            cfg.random_values = _ptr(self._rv, _u64p)
        h = C.c_void_p()
        rc = self.lib.leon_dna_ctx_create(C.byref(cfg), C.byref(h))
        if rc:
            raise LeonDnaError(rc, (self.lib.leon_last_error(None) or b"").decode())
        self.h = h
        self.kmer_size, self.reads_per_block = kmer_size, reads_per_block
        self.bloom_tai, self.bloom_n_hash, self.bloom_block_nbits = int(bloom_tai), bloom_n_hash, bloom_block_nbits
        self.next_read = 0
        self._hdr_next = 0
        self._xch_error = None               # what a Python exchange / gather callback raised inside the last call (nothing may cross the C boundary)

    def _chk(self, rc):
        cause, self._xch_error = getattr(self, "_xch_error", None), None
        if rc:
            err = LeonDnaError(rc, (self.lib.leon_last_error(self.h) or b"").decode())
            if cause is not None:            # the callback's own exception is the cause, not lost behind "the callback returned non-zero"
                raise err from cause
            raise err

    def close(self):
        if getattr(self, "h", None):
            self.lib.leon_dna_ctx_destroy(self.h)
            self.h = None

    __del__ = close

    # ---- bloom ----
    @property
    def bloom_nbytes(self):
        n = C.c_uint64()
        self._chk(self.lib.leon_dna_bloom_nbytes(self.h, C.byref(n)))
        return n.value

    def bloom_upload(self, bits):
        bits = np.ascontiguousarray(bits, dtype=np.uint8)
        self._chk(self.lib.leon_dna_bloom_upload(self.h, _ptr(bits, _u8p), len(bits)))

    def bloom_download(self):
        out = np.zeros(self.bloom_nbytes, dtype=np.uint8)
        self._chk(self.lib.leon_dna_bloom_download(self.h, _ptr(out, _u8p), len(out)))
        return out

    def bloom_clear(self):
        self._chk(self.lib.leon_dna_bloom_clear(self.h))

    def bloom_insert(self, kmers):
        """kmers: flat uint64 array, kmer_words(k) words per k-mer"""
        kmers = np.ascontiguousarray(kmers, dtype=np.uint64).reshape(-1)
        self._chk(self.lib.leon_dna_bloom_insert(self.h, _ptr(kmers, _u64p), len(kmers) // kmer_words(self.kmer_size)))

    def bloom_insert_device(self, dev_ptr, n):
        self._chk(self.lib.leon_dna_bloom_insert_device(self.h, C.c_void_p(int(dev_ptr)), int(n)))

    def bloom_device_ptr(self):
        p, n = C.c_void_p(), C.c_uint64()
        self._chk(self.lib.leon_dna_bloom_device_ptr(self.h, C.byref(p), C.byref(n)))
        return p.value, n.value

    def bloom_upload_device(self, dev_ptr, n):
        self._chk(self.lib.leon_dna_bloom_upload_device(self.h, C.c_void_p(int(dev_ptr)), int(n)))

    def bloom_download_device(self, dev_ptr, n):
        self._chk(self.lib.leon_dna_bloom_download_device(self.h, C.c_void_p(int(dev_ptr)), int(n)))

    def bloom_contains4(self, kmers, right):
        kmers = np.ascontiguousarray(kmers, dtype=np.uint64).reshape(-1)
        n = len(kmers) // kmer_words(self.kmer_size)
        out = np.zeros(n, dtype=np.uint8)
        self._chk(self.lib.leon_dna_bloom_contains4(self.h, _ptr(kmers, _u64p), n, int(right), _ptr(out, _u8p)))
        return out

    def bloom_contains(self, kmers):
        kmers = np.ascontiguousarray(kmers, dtype=np.uint64).reshape(-1)
        n = len(kmers) // kmer_words(self.kmer_size)
        out = np.zeros(n, dtype=np.uint8)
        self._chk(self.lib.leon_dna_bloom_contains(self.h, _ptr(kmers, _u64p), n, _ptr(out, _u8p)))
        return out

    # ---- encode ----
    def _collect_sink(self, blocks):
        def cb(user, block_id, payload, size, n_reads):
            blocks.append((block_id, C.string_at(payload, size), n_reads))
            return 0
        return SINK(cb)

    def encode_batch(self, bases, offsets, sink=None):
        """bases: bytes / uint8 array, offsets: uint64[n+1].  Returns [(block_id, payload, n_reads)]."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        if isinstance(bases, (bytes, bytearray)):
            keep = (C.c_char * len(bases)).from_buffer_copy(bases) if isinstance(bases, bytes) else (C.c_char * len(bases)).from_buffer(bases)
            ptr = C.cast(keep, C.c_void_p)
        else:                                                   # a uint8 array is handed over in place (no copy)
            keep = np.ascontiguousarray(bases, dtype=np.uint8)
            ptr = C.c_void_p(keep.ctypes.data)
        blocks = []
        cb = sink if sink is not None else self._collect_sink(blocks)
        self._chk(self.lib.leon_dna_encode_batch(self.h, ptr, _ptr(offsets, _u64p), n, self.next_read, cb, None))
        self.next_read += n
        return blocks

    def encode_batch_device(self, d_bases_ptr, d_offsets_ptr, n_reads, sink=None):
        blocks = []
        cb = sink if sink is not None else self._collect_sink(blocks)
        self._chk(self.lib.leon_dna_encode_batch_device(self.h, C.c_void_p(int(d_bases_ptr)), C.c_void_p(int(d_offsets_ptr)),
                                                        int(n_reads), self.next_read, cb, None))
        self.next_read += int(n_reads)
        return blocks

    def header_encode_batch(self, headers, first_header=None, sink=None):
        """HeaderEncoder over a batch of header texts (list of bytes, file order) -> [(block_id, payload, n_reads)]"""
        blob = b"".join(headers)
        off = np.zeros(len(headers) + 1, dtype=np.uint64)
        if headers:
            off[1:] = np.cumsum([len(h) for h in headers])
        if first_header is None:
            first_header = headers[0] if headers else b""
        blocks = []
        cb = sink or self._collect_sink(blocks)
        self._chk(self.lib.leon_header_encode_batch(self.h, blob, _ptr(off, _u64p), len(headers), self._hdr_next, first_header,
                                                    len(first_header), cb, None))
        self._hdr_next += len(headers)
        return blocks

    def header_decode_blocks(self, blocks, first_header, n_threads=0):
        """HeaderDecoder with the symbols decoded on the device and the text rebuilt on host threads:
        blocks = [(id, payload, n_reads)] -> list of header bytes (same results as host_header_decode_blocks)"""
        if not blocks:
            return []
        pay, off, nr = _join_blocks(blocks)
        total = int(nr[:len(blocks)].sum())
        out_off = np.zeros(total + 1, dtype=np.uint64)
        need = C.c_uint64()
        cap = max(64, 64 * total)
        for _ in range(2):
            out = np.zeros(cap, dtype=np.uint8)
            rc = self.lib.leon_header_decode_blocks(self.h, _ptr(pay, _u8p), _ptr(off, _u64p), _ptr(nr, _u32p), len(blocks), first_header,
                                                    len(first_header), _ptr(out, _u8p), cap, _ptr(out_off, _u64p), C.byref(need), n_threads)
            if rc != -5:
                break
            cap = need.value
        self._chk(rc)
        raw = out.tobytes()
        return [raw[int(out_off[i]):int(out_off[i + 1])] for i in range(total)]

    def header_symbol_set(self, blocks):
        """the device half of header_decode_blocks alone: the symbols of ALL of `blocks` in one device call.  Returns an object whose
        .text(first_block, n_blocks, first_header) gives those blocks' headers (host threads) and .close() frees the set"""
        ctx = self
        pay, off, nr = _join_blocks(blocks)
        h = C.c_void_p()
        self._chk(self.lib.leon_header_decode_symbols(self.h, _ptr(pay, _u8p), _ptr(off, _u64p), _ptr(nr, _u32p), len(blocks), C.byref(h)))

        class Set:
            def text(self, first_block, n_blocks, first_header, n_threads=0, n_reads=None):
                """n_reads: the reads of each of the blocks, where the caller's table says otherwise than the set was decoded with"""
                counts = np.ascontiguousarray(nr[first_block:first_block + n_blocks] if n_reads is None else n_reads, dtype=np.uint32)
                total = int(counts.sum())
                out_off = np.zeros(total + 1, dtype=np.uint64)
                need = C.c_uint64()
                cap = max(64, 64 * total)
                for _ in range(2):
                    out = np.zeros(cap, dtype=np.uint8)
                    rc = ctx.lib.leon_header_text_from_symbols(h, first_block, n_blocks, _ptr(counts, _u32p), first_header, len(first_header),
                                                               _ptr(out, _u8p), cap, _ptr(out_off, _u64p), C.byref(need), n_threads)
                    if rc != -5:
                        break
                    cap = need.value
                if rc:
                    raise LeonDnaError(rc, (ctx.lib.leon_last_error(None) or b"").decode())
                raw = out.tobytes()
                return [raw[int(out_off[i]):int(out_off[i + 1])] for i in range(total)]

            def close(self):
                ctx.lib.leon_header_symbols_free(h)
        return Set()

    def header_decode_blocks_device(self, blocks, first_header, n_threads=0):
        """HeaderDecoder with the symbols AND the text on the device (k_hdr_text): blocks = [(id, payload, n_reads)] ->
        (list of header bytes, number of blocks the kernel declined and the host decoder took on n_threads threads)"""
        if not blocks:
            return [], 0
        pay, off, nr = _join_blocks(blocks)
        total = int(nr[:len(blocks)].sum())
        out_off = np.zeros(total + 1, dtype=np.uint64)
        need, on_host = C.c_uint64(), C.c_uint64()
        cap = max(64, 64 * total)
        for _ in range(2):
            out = np.zeros(cap, dtype=np.uint8)
            rc = self.lib.leon_header_decode_blocks_device(self.h, _ptr(pay, _u8p), _ptr(off, _u64p), _ptr(nr, _u32p), len(blocks), first_header,
                                                           len(first_header), _ptr(out, _u8p), cap, _ptr(out_off, _u64p), C.byref(need), n_threads,
                                                           C.byref(on_host))
            if rc != -5:
                break
            cap = need.value
        self._chk(rc)
        raw = out.tobytes()
        return [raw[int(out_off[i]):int(out_off[i + 1])] for i in range(total)], int(on_host.value)

    def header_text_set(self, blocks, first_header, text_bytes=None):
        """both device halves of header_decode_blocks_device over ALL of `blocks` in one call; the text stays in device memory.
        text_bytes: every block's text size where known (a container's block table), else the kernel sizes them first.  Returns an object
        whose .fetch(first_block, n_blocks) gives those blocks' headers, .device_ptr(first_block, n_blocks) -> (d_text, d_off, size), and
        .close() frees the set (before the context is closed)"""
        ctx = self
        pay, off, nr = _join_blocks(blocks)
        tb = None if text_bytes is None else np.ascontiguousarray(list(text_bytes) or [0], dtype=np.uint64)
        if tb is not None and len(text_bytes) != len(blocks):
            raise ValueError("text_bytes: one entry per block")
        h = C.c_void_p()
        self._chk(self.lib.leon_header_decode_text(self.h, _ptr(pay, _u8p), _ptr(off, _u64p), _ptr(nr, _u32p), None if tb is None else _ptr(tb, _u64p),
                                                   len(blocks), first_header, len(first_header), C.byref(h)))

        class Set:
            def fetch(self, first_block, n_blocks):
                total = int(nr[first_block:first_block + n_blocks].sum()) if first_block + n_blocks <= len(blocks) else 0
                out_off = np.zeros(total + 1, dtype=np.uint64)
                need = C.c_uint64()
                cap = max(64, 64 * total)
                for _ in range(2):
                    out = np.zeros(cap, dtype=np.uint8)
                    rc = ctx.lib.leon_header_text_fetch(h, first_block, n_blocks, _ptr(out, _u8p), cap, _ptr(out_off, _u64p), C.byref(need))
                    if rc != -5:
                        break
                    cap = need.value
                if rc:
                    raise LeonDnaError(rc, (ctx.lib.leon_last_error(None) or b"").decode())
                raw = out.tobytes()
                return [raw[int(out_off[i]):int(out_off[i + 1])] for i in range(total)]

            def device_ptr(self, first_block, n_blocks):
                d_text, d_off, size = C.c_void_p(), C.c_void_p(), C.c_uint64()
                rc = ctx.lib.leon_header_text_device_ptr(h, first_block, n_blocks, C.byref(d_text), C.byref(d_off), C.byref(size))
                if rc:
                    raise LeonDnaError(rc, (ctx.lib.leon_last_error(None) or b"").decode())
                return d_text.value, d_off.value, int(size.value)

            def close(self):
                ctx.lib.leon_header_text_free(h)
        return Set()

    def qual_smooth_batch(self, bases, offsets, quals):
        """DnaEncoder::smoothQuals (lossy qualities) over a batch: returns the smoothed quality bytes (same offsets)"""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        q = np.frombuffer(bytes(quals), dtype=np.uint8).copy()
        if len(offsets) > 1:
            self._chk(self.lib.leon_qual_smooth_batch(self.h, bytes(bases), _ptr(offsets, _u64p), len(offsets) - 1, _ptr(q, _u8p)))
        return q.tobytes()

    def qual_smooth_batch_device(self, d_bases, d_offsets, n_reads, d_quals):
        """leon_qual_smooth_batch_device: bases, offsets (uint64[n_reads + 1]) and qualities in device memory (raw pointers,
        device_alloc / device_upload_bytes); read i's qualities lie at d_quals + offsets[i] - offsets[0] and are rewritten in place"""
        self._chk(self.lib.leon_qual_smooth_batch_device(self.h, C.c_void_p(int(d_bases or 0)), C.c_void_p(int(d_offsets or 0)),
                                                         int(n_reads), C.c_void_p(int(d_quals or 0))))

    def finish(self, copy=True):
        """(dictionary stream, number of anchors); copy=False returns its size instead of a bytes copy (the C caller
        gets a pointer into the context and writes from there: a 100 M-read file's stream is 110 MB)"""
        p, sz, na = _u8p(), C.c_uint64(), C.c_uint64()
        self._chk(self.lib.leon_dna_finish(self.h, C.byref(p), C.byref(sz), C.byref(na)))
        return (C.string_at(p, sz.value) if copy else sz.value), na.value

    def dict_pieces(self):
        """leon_dna_dict_pieces, after finish() on a context created with dict_pieces=True: (piece_off uint64[n_pieces + 1], piece_anchors)"""
        p, n, pa = _u64p(), C.c_uint64(), C.c_uint32()
        self._chk(self.lib.leon_dna_dict_pieces(self.h, C.byref(p), C.byref(n), C.byref(pa)))
        return np.ctypeslib.as_array(p, shape=(n.value + 1,)).astype(np.uint64, copy=True), pa.value

    def decode_blocks(self, anchors, blocks, block_n_bases):
        """DnaDecoder over read blocks: blocks = [(block_id, payload, n_reads)] as the encoder's sink delivered them,
        anchors = the dictionary (anchor_dict_decode), block_n_bases = bases per block.  Returns the list of reads (bytes)."""
        out, lens = self.decode_blocks_raw(anchors, blocks, block_n_bases)
        ends = np.cumsum(lens, dtype=np.uint64)
        raw = out.tobytes()
        return [raw[int(e) - int(l):int(e)] for e, l in zip(ends, lens)]

    def decode_blocks_raw(self, anchors, blocks, block_n_bases):
        """same, returning (bases back to back as a uint8 array, read lengths as a uint32 array)"""
        blocks = sorted(blocks)
        nb = len(blocks)
        anchors = np.ascontiguousarray(anchors, dtype=np.uint64)
        W = kmer_words(self.kmer_size)
        pay = np.frombuffer(b"".join(b[1] for b in blocks) + b"\0", dtype=np.uint8)
        off = np.zeros(nb + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(b[1]) for b in blocks], dtype=np.uint64)
        nreads = np.array([b[2] for b in blocks], dtype=np.uint32)
        nbases = np.ascontiguousarray(block_n_bases, dtype=np.uint64)
        total, n_total = int(nbases.sum()), int(nreads.sum())
        out = np.zeros(total + 1, dtype=np.uint8)
        lens = np.zeros(n_total + 1, dtype=np.uint32)
        self._chk(self.lib.leon_dna_decode_blocks(self.h, _ptr(anchors, _u64p), len(anchors) // W, _ptr(pay, _u8p), _ptr(off, _u64p),
                                                  _ptr(nreads, _u32p), _ptr(nbases, _u64p), nb, _ptr(out, _u8p), total,
                                                  _ptr(lens, _u32p)))
        return out[:total], lens[:n_total]

    def decode_blocks_device(self, anchors, blocks, block_n_bases, d_bases, d_len, host_lens=True):
        """decode_blocks_raw with the bases and lengths left in the caller's device buffers (raw pointers, device_alloc): returns the
        host copy of the lengths (or None)"""
        blocks = sorted(blocks)
        nb = len(blocks)
        anchors = np.ascontiguousarray(anchors, dtype=np.uint64)
        W = kmer_words(self.kmer_size)
        pay = np.frombuffer(b"".join(b[1] for b in blocks) + b"\0", dtype=np.uint8)
        off = np.zeros(nb + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(b[1]) for b in blocks], dtype=np.uint64)
        nreads = np.array([b[2] for b in blocks], dtype=np.uint32)
        nbases = np.ascontiguousarray(block_n_bases, dtype=np.uint64)
        total, n_total = int(nbases.sum()), int(nreads.sum())
        lens = np.zeros(n_total + 1, dtype=np.uint32) if host_lens else None
        self._chk(self.lib.leon_dna_decode_blocks_device(self.h, _ptr(anchors, _u64p), len(anchors) // W, _ptr(pay, _u8p), _ptr(off, _u64p),
                                                         _ptr(nreads, _u32p), _ptr(nbases, _u64p), nb, C.c_void_p(int(d_bases)), total,
                                                         C.c_void_p(int(d_len)), _ptr(lens, _u32p) if host_lens else None))
        return lens[:n_total] if host_lens else None

    def reserve(self, max_reads, max_bases):
        self._chk(self.lib.leon_dna_reserve(self.h, int(max_reads), int(max_bases)))

    def set_shard(self, rank, world):
        self._chk(self.lib.leon_dna_set_shard(self.h, rank, world))

    def set_exchange(self, mode, fn=None):
        """how the walk is divided among the ranks of set_shard: XCH_OFF (by block range), XCH_BY_ANCHOR with `fn(d_send, send_counts) ->
        (d_recv, recv_total)` doing the all-to-all of the 64-bit words in device memory, XCH_EMULATE (this context plays every rank's slice)"""
        if fn is None:
            self._xch_cb = C.cast(None, EXCHANGE)
        else:
            def thunk(user, d_send, counts, world, d_recv, recv_total):
                try:
                    ptr, total = fn(int(d_send or 0), [int(counts[i]) for i in range(world)])
                    d_recv[0] = C.c_void_p(ptr)
                    recv_total[0] = int(total)
                    return 0
                except Exception as e:                 # noqa: BLE001 -- nothing may cross the C boundary
                    self._xch_error = e
                    return 1
            self._xch_cb = EXCHANGE(thunk)
        self._chk(self.lib.leon_dna_set_exchange(self.h, mode, self._xch_cb, None))

    def set_gather(self, fn=None):
        """the window look-ups of the anchor resolution divided among the ranks too: `fn(d_buf, part_bytes, world)` all-gathers the
        device buffer in place (part r at d_buf + r * part_bytes, this rank's part filled on entry)"""
        if fn is None:
            self._gather_cb = C.cast(None, GATHER)
        else:
            def thunk(user, d_buf, part_bytes, world):
                try:
                    fn(int(d_buf or 0), int(part_bytes), int(world))
                    return 0
                except Exception as e:                 # noqa: BLE001 -- nothing may cross the C boundary
                    self._xch_error = e
                    return 1
            self._gather_cb = GATHER(thunk)
        self._chk(self.lib.leon_dna_set_gather(self.h, self._gather_cb, None))

    def reset_stream(self):
        self._hdr_next = 0
        self._chk(self.lib.leon_dna_reset_stream(self.h))
        self.next_read = 0

    def stats(self):
        s = Stats()
        self._chk(self.lib.leon_dna_get_stats(self.h, C.byref(s)))
        return s.as_dict()

    # ---- traces ----
    def trace_anchors(self, n_reads):
        pos = np.zeros(n_reads, dtype=np.int32)
        addr = np.zeros(n_reads, dtype=np.uint32)
        flags = np.zeros(n_reads, dtype=np.uint8)
        self._chk(self.lib.leon_dna_trace_anchors(self.h, _ptr(pos, _i32p), _ptr(addr, _u32p), _ptr(flags, _u8p), n_reads))
        return pos, addr, flags

    def trace_events(self, n_bases):
        ev = np.zeros(n_bases, dtype=np.uint8)
        self._chk(self.lib.leon_dna_trace_events(self.h, _ptr(ev, _u8p), n_bases))
        return ev

    def anchor_kmers(self, n):
        w = kmer_words(self.kmer_size)
        out = np.zeros(max(n, 1) * w, dtype=np.uint64)
        self._chk(self.lib.leon_dna_anchor_kmers(self.h, _ptr(out, _u64p), n))
        return out[:n * w]

    def rc_encode_streams(self, syms, begin):
        """syms: uint8[2*n] (model, value) pairs; begin: uint64[n_streams+1].  Returns list of payload bytes."""
        syms = np.ascontiguousarray(syms, dtype=np.uint8)
        begin = np.ascontiguousarray(begin, dtype=np.uint64)
        ns = len(begin) - 1
        cap = 3 * (len(syms) // 2) + 64 * (ns + 1)
        out = np.zeros(cap, dtype=np.uint8)
        sizes = np.zeros(max(ns, 1), dtype=np.uint64)
        self._chk(self.lib.leon_rc_encode_streams(self.h, _ptr(syms, _u8p), _ptr(begin, _u64p), ns, _ptr(out, _u8p), cap,
                                                  _ptr(sizes, _u64p)))
        res, w = [], 0
        for i in range(ns):
            res.append(out[w:w + int(sizes[i])].tobytes())
            w += int(sizes[i])
        return res
