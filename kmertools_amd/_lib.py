"""ctypes binding of libkmertools_hip.so (the C ABI declared in include/kmertools_hip.h).

There is no CPU fallback: if the HIP library is missing or no gfx950 device is usable,
the calls raise.  Nothing here imports the parity oracle.
"""
import ctypes as C
import os
import pathlib
import subprocess

_HERE = pathlib.Path(__file__).resolve().parent
LIB_PATH = pathlib.Path(os.environ.get("KT_LIB", _HERE / "libkmertools_hip.so"))  # KT_LIB: A/B builds

KT_OK = 0
KT_ERR_ARG, KT_ERR_HIP, KT_ERR_NOMEM, KT_ERR_FULL, KT_ERR_NODEVICE, KT_ERR_BADNT, KT_ERR_IO = 1, 2, 3, 4, 5, 6, 7
KT_MEM_HOST, KT_MEM_DEVICE = 0, 1
KT_F64, KT_F32, KT_U32 = 0, 1, 2
KT_EMPTY_KEY = 0xFFFFFFFFFFFFFFFF
KT_SKETCH_MAX_S = 16384
KT_CARD_MIN_P, KT_CARD_MAX_P = 4, 16
KT_PREFILTER_MIN_LOG2, KT_PREFILTER_MAX_LOG2 = 10, 34
KT_SET_INTERSECT, KT_SET_SUBTRACT, KT_SET_UNION, KT_SET_XOR = 0, 1, 2, 3
KT_SETCNT_FIRST, KT_SETCNT_MIN, KT_SETCNT_MAX, KT_SETCNT_SUM = 0, 1, 2, 3
KT_GRAPH_CENSUS = 32
KT_HET_ALL, KT_HET_MIDDLE, KT_HET_CENSUS = 0, 1, 8
KT_TIP_KEEP, KT_TIP_TIP, KT_TIP_ISOLATED, KT_TIP_TALLY = 0, 1, 2, 4
KT_CLIP_ISOLATED, KT_CLIP_STATS = 1, 8
KT_BUBBLE_POP, KT_BUBBLE_TALLY, KT_SIMPLIFY_STATS = 4, 4, 12
KT_THREAD_TALLY = 6
KT_NO_COMPONENT, KT_COMPONENT_FIELDS, KT_COMPONENT_TALLY, KT_READ_COMPONENT_TALLY = 0xFFFFFFFF, 5, 6, 4

# every symbol include/kmertools_hip.h declares: name -> (restype, argtypes)
_vp, _u64, _u32, _i = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
SYMBOLS = {
    "kt_version": (_i, []),
    "kt_last_error": (C.c_char_p, []),
    "kt_device_count": (_i, [C.POINTER(_i)]),
    "kt_ctx_create": (_i, [_i, _vp, _i, C.POINTER(_vp)]),
    "kt_ctx_destroy": (_i, [_vp]),
    "kt_device_memory": (_i, [_vp, C.POINTER(_u64), C.POINTER(_u64)]),
    "kt_device_alloc_placed": (_i, [_vp, _u64, _i, _i, _vp, _vp, C.POINTER(_vp), C.POINTER(C.c_double), C.POINTER(_i),
                               C.POINTER(_i)]),
    "kt_device_free": (_i, [_vp, _vp]),
    "kt_host_register": (_i, [_vp, _vp, C.c_size_t]),
    "kt_host_unregister": (_i, [_vp, _vp]),
    "kt_ctx_sync": (_i, [_vp]),
    "kt_ctx_set_cu_limit": (_i, [_vp, _u32]),
    "kt_ctx_cu_limit": (_i, [_vp, C.POINTER(_u32), C.POINTER(_u32)]),
    "kt_bins": (_i, [_i, _i, C.POINTER(_u64)]),
    "kt_pos_map": (_i, [_i, _vp, _vp, C.POINTER(_u32)]),
    "kt_rev_comp": (_u64, [_u64, _i]),
    "kt_numeric_to_kmer": (_i, [_u64, _i, C.c_char_p]),
    "kt_kmer_to_numeric": (_i, [C.c_char_p, _u64, C.POINTER(_u64), C.POINTER(_u64)]),
    "kt_cgr_coords": (_i, [_i, C.c_double, _vp]),
    "kt_kmers": (_i, [_vp, _vp, _vp, _u64, _i, _vp, _vp, _vp, _i]),
    "kt_oligo_batch": (_i, [_vp, _vp, _vp, _u64, _i, _i, _i, _i, _i, _vp, _i]),
    "kt_oligo_tuning": (_i, [_vp, _i]),
    "kt_oligo_launch_info": (_i, [_vp, C.POINTER(_u32), C.POINTER(_i), C.POINTER(C.c_double)]),
    "kt_selftest_quotient": (_i, [_vp, _u32, _u32, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64)]),
    "kt_ctr_create": (_i, [_vp, _i, _u64, C.POINTER(_vp)]),
    "kt_ctr_destroy": (_i, [_vp]),
    "kt_ctr_clear": (_i, [_vp]),
    "kt_ctr_add_reads": (_i, [_vp, _vp, _vp, _u64, _i]),
    "kt_ctr_add_reads_part": (_i, [_vp, _vp, _vp, _u64, _i, _u32, _u32]),
    "kt_ctr_add_pairs": (_i, [_vp, _vp, _vp, _u64, _i]),
    "kt_ctr_size": (_i, [_vp, C.POINTER(_u64)]),
    "kt_ctr_capacity": (_i, [_vp, C.POINTER(_u64)]),
    "kt_ctr_export": (_i, [_vp, _vp, _vp, _u64, C.POINTER(_u64), _i]),
    "kt_ctr_export_target": (_i, [_vp, _vp, _vp, _u64]),
    "kt_ctr_export_stage": (_i, [_vp, C.POINTER(_u64)]),
    "kt_ctr_export_fetch": (_i, [_vp, _u64, _u64, _vp, _vp]),
    "kt_ctr_export_stage_range": (_i, [_vp, _u32, _u32, C.POINTER(_u64)]),
    "kt_table_file_info": (_i, [C.c_char_p, C.POINTER(_i), C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64)]),
    "kt_table_file_check": (_i, [C.c_char_p]),
    "kt_ctr_save": (_i, [_vp, C.c_char_p, _u32, _u32, _i, C.POINTER(_u64)]),
    "kt_ctr_add_file": (_i, [_vp, C.c_char_p, C.POINTER(_u64)]),
    "kt_ctr_spectrum": (_i, [_vp, _vp, _u32, _vp, _i]),
    "kt_ctr_compare": (_i, [_vp, _vp, _vp, _u32, _u32, _vp, _i]),
    "kt_ctr_setop": (_i, [_vp, _vp, _i, _i, _u32, _u32, _u32, _u32, _vp, _vp, _u64, C.POINTER(_u64), _i, _i]),
    "kt_ctr_graph": (_i, [_vp, _u32, _u32, _vp, _vp, _vp, _u64, C.POINTER(_u64), _vp, _i, _i]),
    "kt_ctr_hetmers": (_i, [_vp, _u32, _u32, _i, _vp, _vp, _vp, _vp, _u64, C.POINTER(_u64), _vp, _u32, _u32, _vp, _i, _i]),
    "kt_ctr_unitigs": (_i, [_vp, _u32, _u32, _vp, _u64, _vp, _vp, _vp, _u64, C.POINTER(_u64), C.POINTER(_u64), _i]),
    "kt_ctr_unitigs_linked": (_i, [_vp, _u32, _u32, _vp, _u64, _vp, _vp, _vp, _u64, C.POINTER(_u64), C.POINTER(_u64), _vp, _vp, _u64,
                                   C.POINTER(_u64), _i]),
    "kt_ctr_unitig_tips": (_i, [_vp, _u32, _u32, _u32, _vp, _u64, C.POINTER(_u64), _vp, _i]),
    "kt_ctr_clip_tips": (_i, [_vp, _u32, _u32, _u32, _u32, _u32, _vp]),
    "kt_ctr_unitig_bubbles": (_i, [_vp, _u32, _u32, _u32, _vp, _u64, C.POINTER(_u64), _vp, _i]),
    "kt_ctr_simplify": (_i, [_vp, _u32, _u32, _u32, _u32, _u32, _u32, _vp]),
    "kt_ctr_erase": (_i, [_vp, _vp, _u64, C.POINTER(_u64), _i]),
    "kt_cgr_points": (_i, [_vp, _vp, _vp, _u64, C.c_double, _vp, _vp, _i]),
    "kt_minimisers": (_i, [_vp, _vp, _vp, _u64, _u64, _i, _vp, _vp, _vp, _vp, _u64, C.POINTER(_u64), _i]),
    "kt_cov_batch": (_i, [_vp, _vp, _vp, _u64, _u64, _u64, _i, _i, _vp, _i]),
    "kt_cov_batch_part": (_i, [_vp, _vp, _vp, _u64, _u64, _u64, _vp, _i, _u32, _u32]),
    "kt_ctr_lookup": (_i, [_vp, _vp, _u64, _vp, _i]),
    "kt_ctr_read_solidity": (_i, [_vp, _vp, _vp, _u64, _u32, _u32, _vp, _vp, _vp, _i, _u32, _u32]),
    "kt_ctr_profile": (_i, [_vp, _vp, _vp, _u64, _vp, _i, _u32, _u32]),
    "kt_profile_stats": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _i]),
    "kt_ctr_index_sequences": (_i, [_vp, _vp, _vp, _u64, C.POINTER(_u64), _i]),
    "kt_ctr_thread_hits": (_i, [_vp, _vp, _vp, _u64, _vp, _i]),
    "kt_thread_runs": (_i, [_vp, _vp, _vp, _u64, _vp, _u64, _i, _vp, _vp, _vp, _vp, _vp, _u64, C.POINTER(_u64), _vp, _vp, _vp, _i]),
    "kt_unitig_components": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _i, _vp, _vp, _u64, C.POINTER(_u64), _vp, _i]),
    "kt_thread_read_components": (_i, [_vp, _vp, _vp, _vp, _u64, _vp, _u64, _u64, _vp, _vp, _vp, _vp, _vp, _i]),
    "kt_ctr_correct_support": (_i, [_vp, _vp, _vp, _u64, _vp, _u32, _u32, _vp, _i, _u32, _u32]),
    "kt_correct_apply": (_i, [_vp, _vp, _vp, _u64, _vp, _u32, _u32, _vp, _vp, _vp, _i]),
    "kt_sketch_batch": (_i, [_vp, _vp, _vp, _u64, _i, _u32, _u64, _vp, _vp, _vp, _i]),
    "kt_sketch_merge": (_i, [_vp, _vp, _vp, _u64, _u32, _vp, _u64, _vp, _vp, _i]),
    "kt_sketch_pairs": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _u64, _u32, _vp, _vp, _i]),
    "kt_mash_distance": (C.c_double, [_u32, _u32, _i]),
    "kt_scaled_max_hash": (_u64, [_u64]),
    "kt_containment_ani": (C.c_double, [_u64, _u64, _i]),
    "kt_scaled_batch": (_i, [_vp, _vp, _vp, _u64, _i, _u64, _u64, _vp, _vp, _u64, _vp, _vp, C.POINTER(_u64), _i]),
    "kt_scaled_merge": (_i, [_vp, _vp, _vp, _vp, _u64, _vp, _u64, _vp, _vp, _u64, _vp, C.POINTER(_u64), _i]),
    "kt_ctr_scaled": (_i, [_vp, _u32, _u32, _u64, _u64, _vp, _vp, _u64, C.POINTER(_u64), _vp, _i]),
    "kt_scaled_pairs": (_i, [_vp, _vp, _vp, _u64, _vp, _vp, _u64, _vp, _i]),
    "kt_card_add_reads": (_i, [_vp, _vp, _vp, _u64, _i, _i, _u64, _vp, _vp, _i]),
    "kt_card_merge": (_i, [_vp, _vp, _i]),
    "kt_card_estimate": (_i, [_vp, _i, C.POINTER(C.c_double), C.POINTER(_u64)]),
    "kt_card_rel_error": (C.c_double, [_i]),
    "kt_prefilter_create": (_i, [_vp, _i, _i, _i, _u64, C.POINTER(_vp)]),
    "kt_prefilter_destroy": (_i, [_vp]),
    "kt_prefilter_clear": (_i, [_vp]),
    "kt_prefilter_add_reads": (_i, [_vp, _vp, _vp, _u64, _i]),
    "kt_prefilter_stats": (_i, [_vp, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64)]),
    "kt_prefilter_query": (_i, [_vp, _vp, _u64, _vp, _i]),
    "kt_ctr_add_reads_filtered": (_i, [_vp, _vp, _vp, _vp, _u64, _i, _u32, _u32]),
    "kt_ctr_route": (_i, [_vp, _vp, _vp, _u64, _i, _i, _vp, _vp, _i]),
    "kt_owner_of": (_u32, [_u64, _u32]),
    "kt_rccl_unique_id": (_i, [_vp]),
    "kt_sharded_create_rccl": (_i, [_vp, _i, _u64, _u64, _i, _i, _vp, C.POINTER(_vp)]),
    "kt_sharded_create_host": (_i, [_vp, _i, _u64, _u64, _i, _i, _vp, _vp, C.POINTER(_vp)]),
    "kt_sharded_destroy": (_i, [_vp]),
    "kt_sharded_clear": (_i, [_vp]),
    "kt_sharded_add_reads": (_i, [_vp, _vp, _vp, _u64, _i]),
    "kt_sharded_finalize": (_i, [_vp]),
    "kt_sharded_table": (_i, [_vp, C.POINTER(_vp)]),
    "kt_sharded_exchanged_bytes": (_i, [_vp, C.POINTER(_u64)]),
    "kt_sharded_comm_info": (_i, [_vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "kt_sharded_create_local": (_i, [_vp, _i, _u64, _u64, _i, _i, C.POINTER(_vp)]),
    "kt_sharded_connect_rccl": (_i, [_vp, _vp]),
    "kt_sharded_connect_host": (_i, [_vp, _vp, _vp]),
    "kt_sharded_owner_of": (_i, [_vp, _u64, C.POINTER(_u32)]),
    "kt_sharded_route_stats": (_i, [_vp, C.POINTER(_u32), _vp, _vp]),
    "kt_shard_minimiser": (_i, [_i, C.POINTER(_u32), C.POINTER(_u32)]),
    "kt_shard_owner_of": (_u32, [_u64, _i, _u32]),
    "kt_synth_reads": (_i, [_vp, _u64, _u64, _u64, _u32, _i, _u64, _vp, _vp]),
}


ALLTOALL_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64)  # kt_alltoall_fn
PROBE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p)                              # kt_probe_fn


class KmertoolsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libkmertools_hip error %d: %s" % (code, msg))
        self.code = code


_lib = None


def build(force=False):
    """Compile libkmertools_hip.so for gfx950 (hipcc cross-compiles without a GPU)."""
    srcdir = _HERE / "csrc"
    if force:
        subprocess.check_call(["make", "-C", str(srcdir), "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", str(srcdir), "-j4"], stdout=subprocess.DEVNULL)
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise ImportError(
                "%s is missing - build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C kmertools_amd/csrc`; there is no CPU fallback" % LIB_PATH)
        # torch bundles its own libamdhip64; importing it first makes this library resolve to
        # the same HIP runtime instance, so torch's streams/pointers are valid here (two
        # runtimes in one process cannot both see the GPU).  Without torch, /opt/rocm's is used.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(str(LIB_PATH))
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)  # AttributeError if the ABI lost a symbol
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def last_error():
    s = lib().kt_last_error()
    return s.decode("utf-8", "replace") if s else ""


def check(rc):
    if rc != KT_OK:
        raise KmertoolsError(rc, last_error())
    return rc
