"""ctypes binding of libkzgx.so (the C ABI in include/kzg_gpu.h).

Host-side plumbing for tests and bench.py: numpy arrays in, numpy arrays out.
There is no fallback: if libkzgx.so is missing or no gfx950 device is visible,
every entry point raises.  Scalars are (n, 4) uint64 arrays (little-endian
limbs, canonical mod r); points are (n, 2 * W64) uint64 arrays (x || y,
canonical), W64 = 4 (BN254) or 6 (BLS12-381), infinity = all zeros.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get("KZGX_LIB", os.path.join(PKG_DIR, "libkzgx.so"))
CURVES = {"BN254": 0, "BLS12381": 1}
BASE_LIMBS = {"BN254": 4, "BLS12381": 6}

# exported C symbols (must match include/kzg_gpu.h)
EXPORTS = [
    "kzgx_strerror", "kzgx_base_limbs", "kzgx_init_device", "kzgx_create", "kzgx_destroy", "kzgx_sync", "kzgx_curve",
    "kzgx_srs_size", "kzgx_stream", "kzgx_prof_enable", "kzgx_prof_read", "kzgx_prof_clear", "kzgx_set_window_bits", "kzgx_set_segment",
    "kzgx_set_fixed_base", "kzgx_fixed_base_info", "kzgx_fixed_base_bytes", "kzgx_set_fixed_base_budget",
    "kzgx_set_fixed_base_layout", "kzgx_fixed_base_layout", "kzgx_set_default_table", "kzgx_default_table_info",
    "kzgx_set_fixed_joint", "kzgx_fixed_joint_info", "kzgx_fixed_window_info", "kzgx_set_fixed_joint_ranges",
    "kzgx_set_fixed_accum_reserve", "kzgx_fixed_accum_reserve_info",
    "kzgx_microbench_mad_u64", "kzgx_microbench_mad_u64_clock", "kzgx_clock_probe", "kzgx_set_fixed_points_per_thread", "kzgx_set_small_batch", "kzgx_microbench_mixed_add", "kzgx_load_srs_g1", "kzgx_gen_srs_g1", "kzgx_get_srs_g1", "kzgx_msm_g1",
    "kzgx_msm_g1_batch", "kzgx_msm_g1_batch_device", "kzgx_quotient_single_batch_device",
    "kzgx_prove_single_batch", "kzgx_prove_single_batch_device", "kzgx_prove_range", "kzgx_poly_eval",
    "kzgx_poly_interpolate", "kzgx_poly_vanishing", "kzgx_g1_validate", "kzgx_g1_sum", "kzgx_g1_sum_device", "kzgx_g1_sum_packed_device",
    "kzgx_gen_srs_g2", "kzgx_load_srs_g2", "kzgx_get_srs_g2", "kzgx_srs_g2_size", "kzgx_g2_validate",
    "kzgx_msm_g2", "kzgx_pairing", "kzgx_verify_proof", "kzgx_verify_single_batch",
    "kzgx_verify_single_batch_device", "kzgx_set_verify_wave_max", "kzgx_msm_g1_sharded",
    "kzgx_quotient_single_batch", "kzgx_shared_tables", "kzgx_release_cached_memory",
    "kzgx_partial_record_words", "kzgx_msm_g1_partial_device", "kzgx_g1_sum_partials_device",
    "kzgx_msm_g1_points", "kzgx_msm_g1_points_device", "kzgx_verify_aggregate", "kzgx_verify_aggregate_device",
    "kzgx_g1_check_batch", "kzgx_g1_check_batch_device", "kzgx_g2_check_batch", "kzgx_srs_check",
    "kzgx_verify_aggregate_checked", "kzgx_verify_aggregate_checked_device",
    "kzgx_ntt_max_log2", "kzgx_domain_root", "kzgx_ntt", "kzgx_ntt_device", "kzgx_commit_evals_batch",
    "kzgx_commit_evals_batch_device", "kzgx_prove_evals_batch", "kzgx_prove_evals_batch_device",
    "kzgx_g1_ntt", "kzgx_g1_ntt_device", "kzgx_prove_all_prepare", "kzgx_prove_all_batch",
    "kzgx_prove_all_batch_device",
    "kzgx_coset_points", "kzgx_prove_cosets_prepare", "kzgx_prove_cosets_batch", "kzgx_prove_cosets_batch_device",
    "kzgx_verify_cells_aggregate", "kzgx_verify_cells_aggregate_device", "kzgx_verify_cells_aggregate_checked",
    "kzgx_verify_cells_aggregate_checked_device",
    "kzgx_verify_cells_each", "kzgx_verify_cells_each_device", "kzgx_verify_cells_each_checked",
    "kzgx_verify_cells_each_checked_device", "kzgx_set_verify_cells_chunk",
    "kzgx_recover_cells", "kzgx_recover_cells_device", "kzgx_recover_cells_and_proofs",
    "kzgx_recover_cells_and_proofs_device",
    "kzgx_point_bytes", "kzgx_g1_decompress_batch", "kzgx_g1_decompress_batch_device", "kzgx_g1_compress_batch",
    "kzgx_g1_compress_batch_device", "kzgx_g2_decompress_batch", "kzgx_g2_compress_batch",
    "kzgx_verify_cells_aggregate_bytes", "kzgx_verify_cells_aggregate_bytes_device",
    "kzgx_sha256", "kzgx_blob_challenge", "kzgx_blob_challenges", "kzgx_blob_challenges_device",
    "kzgx_evals_at_batch", "kzgx_evals_at_batch_device", "kzgx_prove_blobs_batch", "kzgx_prove_blobs_batch_device",
    "kzgx_verify_blobs_batch", "kzgx_verify_blobs_batch_device", "kzgx_verify_blobs_each",
    "kzgx_verify_blobs_each_device",
    "kzgx_srs_update", "kzgx_srs_verify_structure", "kzgx_srs_verify_update",
    "kzgx_prove_multi_batch", "kzgx_prove_multi_batch_device", "kzgx_verify_multi_batch",
    "kzgx_verify_multi_batch_device", "kzgx_verify_multi_batch_checked", "kzgx_verify_multi_batch_checked_device",
    "kzgx_set_multi_chunk",
    "kzgx_shplonk_commit", "kzgx_shplonk_commit_device", "kzgx_shplonk_open", "kzgx_shplonk_open_device",
    "kzgx_shplonk_verify", "kzgx_shplonk_verify_device", "kzgx_shplonk_verify_checked",
    "kzgx_shplonk_verify_checked_device", "kzgx_set_shplonk_chunk",
]


def _header_define(name: str) -> int:
    """an integer #define of include/kzg_gpu.h (the one place such constants live)"""
    import re
    with open(os.path.join(os.path.dirname(PKG_DIR), "include", "kzg_gpu.h")) as f:
        return int(re.search(r"^#define %s (-?\d+)\b" % name, f.read(), re.M).group(1))


# evaluation form: flag bits, the largest transform, and the largest one a
# workgroup runs out of LDS (above it the transform takes two passes)
NTT_INVERSE = _header_define("KZGX_NTT_INVERSE")
NTT_BITREV = _header_define("KZGX_NTT_BITREV")
NTT_MAX_LOG2 = _header_define("KZGX_NTT_MAX_LOG2")
NTT_TILE_LOG2 = _header_define("KZGX_NTT_TILE_LOG2")
# G1 NTT and all-domain openings: the input-is-evaluations flag, and the points
# per internal chunk of transforms
PROVE_ALL_EVALS = _header_define("KZGX_PROVE_ALL_EVALS")
G1_NTT_CHUNK_POINTS = _header_define("KZGX_G1_NTT_CHUNK_POINTS")
# coset openings: the cosets are those of the size-2n domain
PROVE_COSETS_EXTENDED = _header_define("KZGX_PROVE_COSETS_EXTENDED")
# cell recovery: the most cells per blob (log2), and the scalars per internal chunk of blobs
RECOVER_MAX_LOG2_CELLS = _header_define("KZGX_RECOVER_MAX_LOG2_CELLS")
RECOVER_CHUNK_SCALARS = _header_define("KZGX_RECOVER_CHUNK_SCALARS")
# compressed points: the ZCash / IETF BLS12-381 encoding, and SEC1 (0x02 | parity, then x)
ENC_ZCASH = _header_define("KZGX_ENC_ZCASH")
ENC_SEC1 = _header_define("KZGX_ENC_SEC1")
# blob proofs: elements are 32-byte big-endian (checked < r), and the scalars per internal chunk of blobs
BLOB_BYTES = _header_define("KZGX_BLOB_BYTES")
BLOB_CHUNK_SCALARS = _header_define("KZGX_BLOB_CHUNK_SCALARS")
# setup ceremony: the structure test also requires G1[0], G2[0] to be the curve's generators
SRS_STRUCT_GENERATORS = _header_define("KZGX_SRS_STRUCT_GENERATORS")
# batch openings: weights are one gamma per group, the scalars per internal chunk of folded
# polynomials, and the coefficients per workgroup of the sliced evaluation
MULTI_WEIGHT_POWERS = _header_define("KZGX_MULTI_WEIGHT_POWERS")
MULTI_CHUNK_SCALARS = _header_define("KZGX_MULTI_CHUNK_SCALARS")
MULTI_EVAL_SLICE = _header_define("KZGX_MULTI_EVAL_SLICE")
# Shplonk openings: weights are one gamma (w_k = gamma^k), the most points per set and in T, the scalars per
# internal chunk of folded polynomials, and the coefficients per workgroup of the fused quotient
SHPLONK_WEIGHT_POWERS = _header_define("KZGX_SHPLONK_WEIGHT_POWERS")
SHPLONK_SET_MAX = _header_define("KZGX_SHPLONK_SET_MAX")
SHPLONK_POINTS_MAX = _header_define("KZGX_SHPLONK_POINTS_MAX")
SHPLONK_CHUNK_SCALARS = _header_define("KZGX_SHPLONK_CHUNK_SCALARS")
SHPLONK_TILE = _header_define("KZGX_SHPLONK_TILE")

_lib = None
u64p = ctypes.POINTER(ctypes.c_uint64)
intp = ctypes.POINTER(ctypes.c_int)
u32p = ctypes.POINTER(ctypes.c_uint32)
u8p = ctypes.POINTER(ctypes.c_uint8)
vp = ctypes.c_void_p
sz = ctypes.c_size_t


class KzgxError(RuntimeError):
    def __init__(self, status: int, where: str):
        self.status = status
        super().__init__("%s: %s (%d)" % (where, lib().kzgx_strerror(status).decode(), status))


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libkzgx.so not built (run __graft_entry__.build())")
        # One HIP runtime per process: PyTorch ships its own libamdhip64 with
        # the same soname as /opt/rocm's.  Loaded first, torch's copy is the
        # one libkzgx.so binds to; loaded second (after libkzgx pulled in
        # /opt/rocm's), torch finds no devices.  Device pointers from torch
        # tensors are then valid in both.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(LIB_PATH)
        sig = {
            "kzgx_strerror": (ctypes.c_char_p, [ctypes.c_int]),
            "kzgx_base_limbs": (ctypes.c_int, [ctypes.c_int]),
            "kzgx_init_device": (ctypes.c_int, [ctypes.c_int, ctypes.c_int]),
            "kzgx_create": (ctypes.c_int, [ctypes.POINTER(vp), ctypes.c_int, ctypes.c_int]),
            "kzgx_destroy": (None, [vp]),
            "kzgx_sync": (ctypes.c_int, [vp]),
            "kzgx_curve": (ctypes.c_int, [vp]),
            "kzgx_srs_size": (sz, [vp]),
            "kzgx_stream": (vp, [vp]),
            "kzgx_prof_enable": (ctypes.c_int, [vp, ctypes.c_int]),
            "kzgx_prof_read": (ctypes.c_int, [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_double), intp]),
            "kzgx_prof_clear": (ctypes.c_int, [vp]),
            "kzgx_set_window_bits": (ctypes.c_int, [vp, ctypes.c_int]),
            "kzgx_set_segment": (ctypes.c_int, [vp, ctypes.c_uint]),
            "kzgx_set_fixed_base": (ctypes.c_int, [vp, ctypes.c_int, sz]),
            "kzgx_fixed_base_info": (ctypes.c_int, [vp, intp, ctypes.POINTER(sz), ctypes.POINTER(sz)]),
            "kzgx_fixed_base_bytes": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, sz, ctypes.POINTER(sz)]),
            "kzgx_set_fixed_base_budget": (ctypes.c_int, [vp, sz, sz, intp]),
            "kzgx_set_fixed_base_layout": (ctypes.c_int, [vp, ctypes.c_int]),
            "kzgx_set_fixed_joint": (ctypes.c_int, [vp, ctypes.c_int]),
            "kzgx_fixed_joint_info": (ctypes.c_int, [vp, intp, ctypes.POINTER(sz), ctypes.POINTER(sz)]),
            "kzgx_fixed_window_info": (ctypes.c_int, [vp, intp, ctypes.POINTER(sz)]),
            "kzgx_set_fixed_joint_ranges": (ctypes.c_int, [vp, ctypes.c_uint]),
            "kzgx_set_fixed_accum_reserve": (ctypes.c_int, [vp, ctypes.c_int]),
            "kzgx_fixed_accum_reserve_info": (ctypes.c_int, [vp, intp, intp, ctypes.POINTER(sz), intp]),
            "kzgx_set_default_table": (ctypes.c_int, [vp, ctypes.c_int, sz]),
            "kzgx_default_table_info": (ctypes.c_int, [vp, intp, ctypes.POINTER(sz), ctypes.POINTER(sz)]),
            "kzgx_fixed_base_layout": (ctypes.c_int, [vp, intp]),
            "kzgx_microbench_mad_u64": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_double)]),
            "kzgx_microbench_mad_u64_clock": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_double),
                                                             ctypes.POINTER(ctypes.c_double)]),
            "kzgx_clock_probe": (ctypes.c_int, [vp, vp, ctypes.c_uint, vp]),
            "kzgx_set_fixed_points_per_thread": (ctypes.c_int, [vp, ctypes.c_uint]),
            "kzgx_set_small_batch": (ctypes.c_int, [vp, ctypes.c_uint]),
            "kzgx_microbench_mixed_add": (ctypes.c_int, [vp, ctypes.POINTER(ctypes.c_double)]),
            "kzgx_load_srs_g1": (ctypes.c_int, [vp, u64p, sz]),
            "kzgx_gen_srs_g1": (ctypes.c_int, [vp, u64p, sz, sz]),
            "kzgx_get_srs_g1": (ctypes.c_int, [vp, u64p, sz]),
            "kzgx_msm_g1": (ctypes.c_int, [vp, u64p, sz, u64p, intp]),
            "kzgx_msm_g1_batch": (ctypes.c_int, [vp, u64p, sz, sz, u64p, intp]),
            "kzgx_msm_g1_batch_device": (ctypes.c_int, [vp, vp, sz, sz, sz, vp, vp, vp]),
            "kzgx_quotient_single_batch_device": (ctypes.c_int, [vp, vp, sz, sz, vp, sz, vp, sz, vp, vp]),
            "kzgx_prove_single_batch": (ctypes.c_int, [vp, u64p, sz, sz, u64p, sz, u64p, intp, u64p]),
            "kzgx_prove_single_batch_device": (ctypes.c_int, [vp, vp, sz, sz, vp, sz, vp, vp, vp, vp]),
            "kzgx_prove_range": (ctypes.c_int, [vp, u64p, sz, u64p, sz, u64p, intp]),
            "kzgx_poly_eval": (ctypes.c_int, [vp, u64p, sz, u64p, sz, u64p]),
            "kzgx_poly_interpolate": (ctypes.c_int, [vp, u64p, u64p, sz, u64p]),
            "kzgx_poly_vanishing": (ctypes.c_int, [vp, u64p, sz, u64p]),
            "kzgx_g1_validate": (ctypes.c_int, [vp, u64p, intp]),
            "kzgx_g1_sum": (ctypes.c_int, [vp, u64p, intp, sz, u64p, intp]),
            "kzgx_g1_sum_device": (ctypes.c_int, [vp, vp, vp, sz, vp, vp, vp]),
            "kzgx_g1_sum_packed_device": (ctypes.c_int, [vp, vp, sz, vp, vp]),
            "kzgx_gen_srs_g2": (ctypes.c_int, [vp, u64p, sz, sz]),
            "kzgx_load_srs_g2": (ctypes.c_int, [vp, u64p, sz]),
            "kzgx_get_srs_g2": (ctypes.c_int, [vp, u64p, sz]),
            "kzgx_srs_g2_size": (sz, [vp]),
            "kzgx_g2_validate": (ctypes.c_int, [vp, u64p, sz, intp]),
            "kzgx_msm_g2": (ctypes.c_int, [vp, u64p, sz, u64p, intp]),
            "kzgx_pairing": (ctypes.c_int, [vp, u64p, intp, u64p, intp, sz, u64p]),
            "kzgx_verify_proof": (ctypes.c_int, [vp, u64p, ctypes.c_int, u64p, ctypes.c_int, u64p, u64p, sz, intp]),
            "kzgx_verify_single_batch": (ctypes.c_int, [vp, u64p, intp, u64p, intp, u64p, u64p, sz, intp]),
            "kzgx_verify_single_batch_device": (ctypes.c_int, [vp, vp, vp, vp, vp, vp, vp, sz, vp, vp]),
            "kzgx_set_verify_wave_max": (ctypes.c_int, [vp, sz]),
            "kzgx_quotient_single_batch": (ctypes.c_int, [vp, u64p, sz, sz, u64p, sz, u64p, u64p]),
            "kzgx_msm_g1_sharded": (ctypes.c_int, [ctypes.POINTER(vp), ctypes.POINTER(sz), sz, u64p, sz, u64p, intp]),
            "kzgx_shared_tables": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(sz), ctypes.POINTER(sz)]),
            "kzgx_release_cached_memory": (ctypes.c_int, [ctypes.c_int]),
            "kzgx_partial_record_words": (ctypes.c_int, [ctypes.c_int]),
            "kzgx_msm_g1_partial_device": (ctypes.c_int, [vp, vp, sz, vp, vp]),
            "kzgx_g1_sum_partials_device": (ctypes.c_int, [vp, vp, sz, vp, vp]),
            "kzgx_msm_g1_points": (ctypes.c_int, [vp, u64p, intp, u64p, sz, u64p, intp]),
            "kzgx_msm_g1_points_device": (ctypes.c_int, [vp, vp, vp, vp, sz, vp, vp, vp]),
            "kzgx_verify_aggregate": (ctypes.c_int, [vp, u64p, intp, u64p, intp, u64p, u64p, u64p, sz, intp]),
            "kzgx_verify_aggregate_device": (ctypes.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, sz, vp, vp]),
            "kzgx_g1_check_batch": (ctypes.c_int, [vp, u64p, intp, sz, ctypes.c_int, intp]),
            "kzgx_g1_check_batch_device": (ctypes.c_int, [vp, vp, vp, sz, ctypes.c_int, vp, vp, vp]),
            "kzgx_g2_check_batch": (ctypes.c_int, [vp, u64p, intp, sz, ctypes.c_int, intp]),
            "kzgx_srs_check": (ctypes.c_int, [vp, ctypes.c_int, intp, intp]),
            "kzgx_verify_aggregate_checked": (ctypes.c_int, [vp, u64p, intp, u64p, intp, u64p, u64p, u64p, sz,
                                                             ctypes.c_int, intp]),
            "kzgx_verify_aggregate_checked_device": (ctypes.c_int, [vp, vp, vp, vp, vp, vp, vp, vp, sz, ctypes.c_int,
                                                                    vp, vp]),
            "kzgx_ntt_max_log2": (ctypes.c_int, [ctypes.c_int]),
            "kzgx_domain_root": (ctypes.c_int, [ctypes.c_int, ctypes.c_uint, u64p]),
            "kzgx_ntt": (ctypes.c_int, [vp, u64p, ctypes.c_uint, sz, ctypes.c_int, u64p]),
            "kzgx_ntt_device": (ctypes.c_int, [vp, vp, sz, vp, sz, ctypes.c_uint, sz, ctypes.c_int, vp]),
            "kzgx_commit_evals_batch": (ctypes.c_int, [vp, u64p, ctypes.c_uint, sz, ctypes.c_int, u64p, intp]),
            "kzgx_commit_evals_batch_device": (ctypes.c_int, [vp, vp, ctypes.c_uint, sz, sz, ctypes.c_int, vp, vp,
                                                              vp]),
            "kzgx_prove_evals_batch": (ctypes.c_int, [vp, u64p, ctypes.c_uint, sz, u64p, sz, ctypes.c_int, u64p,
                                                      intp, u64p]),
            "kzgx_prove_evals_batch_device": (ctypes.c_int, [vp, vp, ctypes.c_uint, sz, vp, sz, ctypes.c_int, vp, vp,
                                                             vp, vp]),
            "kzgx_g1_ntt": (ctypes.c_int, [vp, u64p, intp, ctypes.c_uint, sz, ctypes.c_int, u64p, intp]),
            "kzgx_g1_ntt_device": (ctypes.c_int, [vp, vp, vp, vp, vp, ctypes.c_uint, sz, ctypes.c_int, vp]),
            "kzgx_prove_all_prepare": (ctypes.c_int, [vp, ctypes.c_uint]),
            "kzgx_prove_all_batch": (ctypes.c_int, [vp, u64p, ctypes.c_uint, sz, ctypes.c_int, u64p, intp, u64p]),
            "kzgx_prove_all_batch_device": (ctypes.c_int, [vp, vp, ctypes.c_uint, sz, sz, ctypes.c_int, vp, vp, vp,
                                                           vp]),
            "kzgx_coset_points": (ctypes.c_int, [ctypes.c_int, ctypes.c_uint, ctypes.c_uint, ctypes.c_int, sz, u64p]),
            "kzgx_prove_cosets_prepare": (ctypes.c_int, [vp, ctypes.c_uint, ctypes.c_uint]),
            "kzgx_prove_cosets_batch": (ctypes.c_int, [vp, u64p, ctypes.c_uint, ctypes.c_uint, sz, ctypes.c_int, u64p,
                                                       intp, u64p]),
            "kzgx_prove_cosets_batch_device": (ctypes.c_int, [vp, vp, ctypes.c_uint, ctypes.c_uint, sz, sz,
                                                              ctypes.c_int, vp, vp, vp, vp]),
            "kzgx_verify_cells_aggregate": (ctypes.c_int, [vp, u64p, intp, sz, u32p, u32p, u64p, intp, u64p, u64p, sz,
                                                           ctypes.c_uint, ctypes.c_uint, ctypes.c_int, intp]),
            "kzgx_verify_cells_aggregate_device": (ctypes.c_int, [vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, sz,
                                                                  ctypes.c_uint, ctypes.c_uint, ctypes.c_int, vp, vp]),
            "kzgx_verify_cells_aggregate_checked": (ctypes.c_int, [vp, u64p, intp, sz, u32p, u32p, u64p, intp, u64p,
                                                                   u64p, sz, ctypes.c_uint, ctypes.c_uint,
                                                                   ctypes.c_int, ctypes.c_int, intp]),
            "kzgx_verify_cells_aggregate_checked_device": (ctypes.c_int, [vp, vp, vp, sz, vp, vp, vp, vp, vp, vp, sz,
                                                                          ctypes.c_uint, ctypes.c_uint, ctypes.c_int,
                                                                          ctypes.c_int, vp, vp]),
            "kzgx_verify_cells_each": (ctypes.c_int, [vp, u64p, intp, sz, u32p, u32p, u64p, intp, u64p, sz,
                                                      ctypes.c_uint, ctypes.c_uint, ctypes.c_int, intp]),
            "kzgx_verify_cells_each_device": (ctypes.c_int, [vp, vp, vp, sz, vp, vp, vp, vp, vp, sz, ctypes.c_uint,
                                                             ctypes.c_uint, ctypes.c_int, vp, vp]),
            "kzgx_verify_cells_each_checked": (ctypes.c_int, [vp, u64p, intp, sz, u32p, u32p, u64p, intp, u64p, sz,
                                                              ctypes.c_uint, ctypes.c_uint, ctypes.c_int,
                                                              ctypes.c_int, intp]),
            "kzgx_verify_cells_each_checked_device": (ctypes.c_int, [vp, vp, vp, sz, vp, vp, vp, vp, vp, sz,
                                                                     ctypes.c_uint, ctypes.c_uint, ctypes.c_int,
                                                                     ctypes.c_int, vp, vp]),
            "kzgx_set_verify_cells_chunk": (ctypes.c_int, [vp, sz]),
            "kzgx_recover_cells": (ctypes.c_int, [vp, u32p, u32p, u64p, sz, sz, ctypes.c_uint, ctypes.c_uint,
                                                  ctypes.c_int, u64p, u64p, intp]),
            "kzgx_recover_cells_device": (ctypes.c_int, [vp, vp, vp, vp, sz, sz, ctypes.c_uint, ctypes.c_uint,
                                                         ctypes.c_int, vp, vp, vp, vp]),
            "kzgx_recover_cells_and_proofs": (ctypes.c_int, [vp, u32p, u32p, u64p, sz, sz, ctypes.c_uint,
                                                             ctypes.c_uint, ctypes.c_int, u64p, u64p, u64p, intp,
                                                             intp]),
            "kzgx_recover_cells_and_proofs_device": (ctypes.c_int, [vp, vp, vp, vp, sz, sz, ctypes.c_uint,
                                                                    ctypes.c_uint, ctypes.c_int, vp, vp, vp, vp, vp,
                                                                    vp]),
            "kzgx_point_bytes": (sz, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
            "kzgx_g1_decompress_batch": (ctypes.c_int, [vp, u8p, sz, ctypes.c_int, ctypes.c_int, u64p, intp, intp]),
            "kzgx_g1_decompress_batch_device": (ctypes.c_int, [vp, vp, sz, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp,
                                                               vp]),
            "kzgx_g1_compress_batch": (ctypes.c_int, [vp, u64p, intp, sz, ctypes.c_int, u8p]),
            "kzgx_g1_compress_batch_device": (ctypes.c_int, [vp, vp, vp, sz, ctypes.c_int, vp, vp]),
            "kzgx_g2_decompress_batch": (ctypes.c_int, [vp, u8p, sz, ctypes.c_int, u64p, intp, intp]),
            "kzgx_g2_compress_batch": (ctypes.c_int, [vp, u64p, intp, sz, u8p]),
            "kzgx_verify_cells_aggregate_bytes": (ctypes.c_int, [vp, u8p, sz, u32p, u32p, u8p, u64p, u64p, sz,
                                                                 ctypes.c_uint, ctypes.c_uint, ctypes.c_int,
                                                                 ctypes.c_int, ctypes.c_int, intp]),
            "kzgx_verify_cells_aggregate_bytes_device": (ctypes.c_int, [vp, vp, sz, vp, vp, vp, vp, vp, sz,
                                                                        ctypes.c_uint, ctypes.c_uint, ctypes.c_int,
                                                                        ctypes.c_int, ctypes.c_int, vp, vp]),
            "kzgx_sha256": (ctypes.c_int, [u8p, sz, u8p]),
            "kzgx_blob_challenge": (ctypes.c_int, [ctypes.c_int, vp, ctypes.c_uint, ctypes.c_int, u8p, u64p, intp]),
            "kzgx_blob_challenges": (ctypes.c_int, [vp, vp, ctypes.c_uint, sz, ctypes.c_int, u8p, u64p, intp]),
            "kzgx_blob_challenges_device": (ctypes.c_int, [vp, vp, ctypes.c_uint, sz, ctypes.c_int, vp, vp, vp, vp]),
            "kzgx_evals_at_batch": (ctypes.c_int, [vp, vp, ctypes.c_uint, sz, u64p, sz, ctypes.c_int, u64p]),
            "kzgx_evals_at_batch_device": (ctypes.c_int, [vp, vp, ctypes.c_uint, sz, vp, sz, ctypes.c_int, vp, vp]),
            "kzgx_prove_blobs_batch": (ctypes.c_int, [vp, vp, ctypes.c_uint, sz, ctypes.c_int, u8p, u8p, u64p, u64p]),
            "kzgx_prove_blobs_batch_device": (ctypes.c_int, [vp, vp, ctypes.c_uint, sz, ctypes.c_int, vp, vp, vp, vp,
                                                             vp, vp]),
            "kzgx_verify_blobs_batch": (ctypes.c_int, [vp, vp, ctypes.c_uint, sz, ctypes.c_int, u8p, u8p, u64p,
                                                       ctypes.c_int, intp]),
            "kzgx_verify_blobs_batch_device": (ctypes.c_int, [vp, vp, ctypes.c_uint, sz, ctypes.c_int, vp, vp, vp,
                                                              ctypes.c_int, vp, vp]),
            "kzgx_verify_blobs_each": (ctypes.c_int, [vp, vp, ctypes.c_uint, sz, ctypes.c_int, u8p, u8p, ctypes.c_int,
                                                      intp]),
            "kzgx_verify_blobs_each_device": (ctypes.c_int, [vp, vp, ctypes.c_uint, sz, ctypes.c_int, vp, vp,
                                                             ctypes.c_int, vp, vp]),
            "kzgx_srs_update": (ctypes.c_int, [vp, u64p, sz, sz, u64p]),
            "kzgx_srs_verify_structure": (ctypes.c_int, [vp, u64p, u64p, ctypes.c_int, intp, intp]),
            "kzgx_srs_verify_update": (ctypes.c_int, [vp, u64p, u64p, u64p, intp]),
            "kzgx_prove_multi_batch": (ctypes.c_int, [vp, u64p, sz, sz, sz, u32p, u32p, sz, u64p, u64p, sz,
                                                      ctypes.c_int, u64p, intp, u64p, u64p]),
            "kzgx_prove_multi_batch_device": (ctypes.c_int, [vp, vp, sz, sz, sz, vp, vp, sz, vp, vp, sz, ctypes.c_int,
                                                             vp, vp, vp, vp, vp, vp]),
            "kzgx_verify_multi_batch": (ctypes.c_int, [vp, u64p, intp, sz, u32p, u32p, sz, u64p, u64p, u64p, u64p,
                                                       intp, u64p, sz, ctypes.c_int, intp]),
            "kzgx_verify_multi_batch_device": (ctypes.c_int, [vp, vp, vp, sz, vp, vp, sz, vp, vp, vp, vp, vp, vp, sz,
                                                              ctypes.c_int, vp, vp]),
            "kzgx_verify_multi_batch_checked": (ctypes.c_int, [vp, u64p, intp, sz, u32p, u32p, sz, u64p, u64p, u64p,
                                                               u64p, intp, u64p, sz, ctypes.c_int, ctypes.c_int,
                                                               intp]),
            "kzgx_verify_multi_batch_checked_device": (ctypes.c_int, [vp, vp, vp, sz, vp, vp, sz, vp, vp, vp, vp, vp,
                                                                      vp, sz, ctypes.c_int, ctypes.c_int, vp, vp]),
            "kzgx_set_multi_chunk": (ctypes.c_int, [vp, sz]),
            "kzgx_shplonk_commit": (ctypes.c_int, [vp, u64p, sz, sz, sz, u64p, sz, u32p, u32p, sz, u32p, u32p, sz,
                                                   u64p, sz, sz, ctypes.c_int, u64p, intp, u64p, u64p]),
            "kzgx_shplonk_commit_device": (ctypes.c_int, [vp, vp, sz, sz, sz, vp, sz, vp, vp, sz, vp, vp, sz, vp, sz,
                                                          sz, ctypes.c_int, vp, vp, vp, vp, vp, vp]),
            "kzgx_shplonk_open": (ctypes.c_int, [vp, u64p, sz, sz, sz, u64p, sz, u32p, u32p, sz, u32p, u32p, sz, u64p,
                                                 sz, ctypes.c_int, u64p, u64p, u64p, intp, u64p]),
            "kzgx_shplonk_open_device": (ctypes.c_int, [vp, vp, sz, sz, sz, vp, sz, vp, vp, sz, vp, vp, sz, vp, sz,
                                                        ctypes.c_int, vp, vp, vp, vp, vp, vp, vp]),
            "kzgx_shplonk_verify": (ctypes.c_int, [vp, u64p, intp, sz, u32p, u64p, sz, u32p, u32p, sz, u32p, sz, u64p,
                                                   sz, u64p, sz, u64p, u64p, intp, ctypes.c_int, intp]),
            "kzgx_shplonk_verify_device": (ctypes.c_int, [vp, vp, vp, sz, vp, vp, sz, vp, vp, sz, vp, sz, vp, sz, vp,
                                                          sz, vp, vp, vp, ctypes.c_int, vp, vp]),
            "kzgx_shplonk_verify_checked": (ctypes.c_int, [vp, u64p, intp, sz, u32p, u64p, sz, u32p, u32p, sz, u32p,
                                                           sz, u64p, sz, u64p, sz, u64p, u64p, intp, ctypes.c_int,
                                                           ctypes.c_int, intp]),
            "kzgx_shplonk_verify_checked_device": (ctypes.c_int, [vp, vp, vp, sz, vp, vp, sz, vp, vp, sz, vp, sz, vp,
                                                                  sz, vp, sz, vp, vp, vp, ctypes.c_int, ctypes.c_int,
                                                                  vp, vp]),
            "kzgx_set_shplonk_chunk": (ctypes.c_int, [vp, sz]),
        }
        for name, (res, args) in sig.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _p(a):
    return None if a is None else a.ctypes.data_as(u64p)


def _chk(rc, where):
    if rc != 0:
        raise KzgxError(rc, where)


def as_scalars(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)


def msm_g1_sharded(ctxs, starts, scalars):
    """kzgx_msm_g1_sharded: one commitment over contexts holding contiguous SRS
    slices (context k's slice starts at point starts[k]); -> (xy, is_inf)"""
    sc = as_scalars(scalars)
    n = sc.shape[0]
    hs = (vp * len(ctxs))(*[c.h for c in ctxs])
    st = (sz * len(ctxs))(*starts)
    out = np.zeros(2 * ctxs[0].w64, dtype=np.uint64)
    oi = ctypes.c_int(0)
    _chk(lib().kzgx_msm_g1_sharded(hs, st, len(ctxs), _p(sc) if n else None, n, _p(out), ctypes.byref(oi)),
         "kzgx_msm_g1_sharded")
    return out, bool(oi.value)


def init_device(curve: str, device: int):
    """kzgx_init_device: HIP, every code object and the generator tables, once
    per (curve, device)."""
    _chk(lib().kzgx_init_device(CURVES[curve], device), "kzgx_init_device")


def shared_tables(device: int = 0):
    """kzgx_shared_tables: (count, bytes) of the default tables shared on a device"""
    c, b = sz(0), sz(0)
    _chk(lib().kzgx_shared_tables(device, ctypes.byref(c), ctypes.byref(b)), "kzgx_shared_tables")
    return c.value, b.value


def release_cached_memory(device: int = 0):
    """kzgx_release_cached_memory: hand the device's cached table block back"""
    _chk(lib().kzgx_release_cached_memory(device), "kzgx_release_cached_memory")


def fixed_base_bytes(curve: str, c: int, n_points: int) -> int:
    """device bytes of a fixed-base table (host arithmetic, no device)"""
    b = sz(0)
    _chk(lib().kzgx_fixed_base_bytes(CURVES[curve], c, n_points, ctypes.byref(b)), "kzgx_fixed_base_bytes")
    return b.value


def ntt_max_log2(curve: str) -> int:
    """kzgx_ntt_max_log2: the largest log2 n of the curve's NTT (host arithmetic, no device)"""
    return lib().kzgx_ntt_max_log2(CURVES[curve])


def point_bytes(curve: str, group: int, encoding: int) -> int:
    """kzgx_point_bytes: the record length of a compressed point, 0 if the combination is not offered
    (host arithmetic, no device)"""
    return int(lib().kzgx_point_bytes(CURVES[curve], group, encoding))


def domain_root(curve: str, log2n: int) -> int:
    """kzgx_domain_root: the generator of the size-2^log2n domain as an integer (no device)"""
    w = np.zeros(4, dtype=np.uint64)
    _chk(lib().kzgx_domain_root(CURVES[curve], log2n, _p(w)), "kzgx_domain_root")
    return sum(int(w[i]) << (64 * i) for i in range(4))


def _ntt_flags(inverse: bool = False, bitrev: bool = False) -> int:
    return (NTT_INVERSE if inverse else 0) | (NTT_BITREV if bitrev else 0)


def _cosets_flags(extended: bool = False, evals: bool = False, bitrev: bool = False) -> int:
    return (PROVE_COSETS_EXTENDED if extended else 0) | (PROVE_ALL_EVALS if evals else 0) | _ntt_flags(bitrev=bitrev)


def coset_points(curve: str, log2n: int, log2l: int, index: int, extended: bool = False,
                 bitrev: bool = False) -> np.ndarray:
    """kzgx_coset_points: the (2^log2l, 4) points whose values sit in chunk `index` of prove_cosets' y,
    in y's order (host arithmetic, no device)"""
    xs = np.zeros((1 << log2l, 4), dtype=np.uint64)
    _chk(lib().kzgx_coset_points(CURVES[curve], log2n, log2l, _cosets_flags(extended, bitrev=bitrev), index, _p(xs)),
         "kzgx_coset_points")
    return xs


def _blob_flags(bytes_mode: bool = False, bitrev: bool = False) -> int:
    return (BLOB_BYTES if bytes_mode else 0) | _ntt_flags(bitrev=bitrev)


def _blob_array(blobs, log2n: int):
    """blobs as one contiguous array: bytes / bytearray / a uint8 array are 32-byte big-endian elements
    (KZGX_BLOB_BYTES), anything else (.., 4) uint64 limbs -> (array, bytes_mode, count)"""
    if isinstance(blobs, (bytes, bytearray)):
        blobs = np.frombuffer(bytes(blobs), dtype=np.uint8)
    a = np.asarray(blobs)
    per = 32 << log2n
    if a.dtype == np.uint8:
        a = np.ascontiguousarray(a).reshape(-1)
        assert a.shape[0] % per == 0
        return a, True, a.shape[0] // per
    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 4)
    assert a.shape[0] % (1 << log2n) == 0
    return a, False, a.shape[0] >> log2n


def _records48(data) -> np.ndarray:
    b = np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else \
        np.ascontiguousarray(data, dtype=np.uint8)
    b = np.ascontiguousarray(b).reshape(-1)
    assert b.shape[0] % 48 == 0
    return b


def sha256(data) -> bytes:
    """kzgx_sha256: the SHA-256 digest (host arithmetic, no device)"""
    m = np.frombuffer(bytes(data), dtype=np.uint8)
    out = np.zeros(32, dtype=np.uint8)
    _chk(lib().kzgx_sha256(m.ctypes.data_as(u8p) if m.shape[0] else None, m.shape[0], out.ctypes.data_as(u8p)),
         "kzgx_sha256")
    return out.tobytes()


def blob_challenge(curve: str, blob, record, flags: int | None = None):
    """kzgx_blob_challenge: one blob (bytes: 32-byte big-endian elements; else (n, 4) uint64 limbs) and its 48-byte
    commitment record -> (z as an integer, ok); host arithmetic, no device.  flags: None = from the blob's type."""
    a = np.asarray(np.frombuffer(bytes(blob), dtype=np.uint8) if isinstance(blob, (bytes, bytearray)) else blob)
    nel = a.size // 32 if a.dtype == np.uint8 else a.size // 4
    log2n = _log2_exact(nel)
    a, bm, cnt = _blob_array(a, log2n)
    assert cnt == 1
    rec = _records48(record)
    assert rec.shape[0] == 48
    z = np.zeros(4, dtype=np.uint64)
    ok = ctypes.c_int(0)
    _chk(lib().kzgx_blob_challenge(CURVES[curve], a.ctypes.data, log2n, _blob_flags(bm) if flags is None else flags,
                                   rec.ctypes.data_as(u8p), _p(z), ctypes.byref(ok)), "kzgx_blob_challenge")
    return sum(int(z[i]) << (64 * i) for i in range(4)), bool(ok.value)


def _log2_exact(n: int) -> int:
    if n < 1 or n & (n - 1):
        raise ValueError("size %d is not a power of two" % n)
    return n.bit_length() - 1


class Context:
    """One device context (SRS + stream + workspaces), kzgx_ctx*."""

    def __init__(self, curve: str = "BN254", device: int = 0):
        self.curve = curve
        self.w64 = BASE_LIMBS[curve]
        h = vp()
        _chk(lib().kzgx_create(ctypes.byref(h), CURVES[curve], device), "kzgx_create")
        self.h = h
        self.device = device

    def set_default_table(self, c: int, n_points: int = 4097):
        """kzgx_set_default_table: c = -1 the budget-chosen window, 0 off"""
        _chk(lib().kzgx_set_default_table(self.h, c, n_points if c else 0), "kzgx_set_default_table")

    def default_table_info(self):
        c, n, b = ctypes.c_int(0), ctypes.c_size_t(0), ctypes.c_size_t(0)
        _chk(lib().kzgx_default_table_info(self.h, ctypes.byref(c), ctypes.byref(n), ctypes.byref(b)),
             "kzgx_default_table_info")
        return c.value, n.value, b.value

    def debug_ws_read(self, name: str, nbytes: int) -> np.ndarray:
        """bytes of one workspace buffer of the context stream (test hook:
        kzgx_debug_ws_read, declared outside kzg_gpu.h)"""
        L = lib()
        fn = L.kzgx_debug_ws_read
        fn.restype = ctypes.c_int
        fn.argtypes = [vp, ctypes.c_char_p, vp, sz]
        a = np.zeros(nbytes, dtype=np.uint8)
        _chk(fn(self.h, name.encode(), a.ctypes.data, nbytes), "kzgx_debug_ws_read")
        return a

    def close(self):
        if getattr(self, "h", None):
            lib().kzgx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self) -> int:
        return lib().kzgx_stream(self.h)

    def sync(self):
        _chk(lib().kzgx_sync(self.h), "kzgx_sync")

    def prof_enable(self, on: bool = True):
        _chk(lib().kzgx_prof_enable(self.h, 1 if on else 0), "kzgx_prof_enable")

    def prof_read(self, name: str):
        ms = ctypes.c_double(0)
        cnt = ctypes.c_int(0)
        _chk(lib().kzgx_prof_read(self.h, name.encode(), ctypes.byref(ms), ctypes.byref(cnt)), "kzgx_prof_read")
        return ms.value, cnt.value

    def set_window_bits(self, c: int):
        _chk(lib().kzgx_set_window_bits(self.h, c), "kzgx_set_window_bits")

    def set_small_batch(self, max_batch: int):
        """table-less batches of <= max_batch MSMs use the window-10 table (0 = never)"""
        _chk(lib().kzgx_set_small_batch(self.h, max_batch), "kzgx_set_small_batch")

    def set_segment(self, k: int):
        _chk(lib().kzgx_set_segment(self.h, k), "kzgx_set_segment")

    def set_fixed_base(self, c: int, n_points: int = 0):
        """Precompute the signed-digit multiples table for the first n_points
        SRS points (c = 0: off).  Built now if an SRS is installed."""
        _chk(lib().kzgx_set_fixed_base(self.h, c, n_points), "kzgx_set_fixed_base")

    def set_fixed_base_layout(self, layout: int):
        """-1 automatic, 0 window-major, 1 point-major (next table build)"""
        _chk(lib().kzgx_set_fixed_base_layout(self.h, layout), "kzgx_set_fixed_base_layout")

    def fixed_base_point_major(self) -> bool:
        pm = ctypes.c_int(0)
        _chk(lib().kzgx_fixed_base_layout(self.h, ctypes.byref(pm)), "kzgx_fixed_base_layout")
        return bool(pm.value)

    def fixed_base_info(self):
        c = ctypes.c_int(0)
        n = sz(0)
        b = sz(0)
        _chk(lib().kzgx_fixed_base_info(self.h, ctypes.byref(c), ctypes.byref(n), ctypes.byref(b)),
             "kzgx_fixed_base_info")
        return c.value, n.value, b.value

    def set_fixed_joint(self, g: int):
        """the block table beside the fixed-base table: -1 automatic, 0 off,
        2..25 that block size at any size and batch (rebuilds a set table)"""
        _chk(lib().kzgx_set_fixed_joint(self.h, g), "kzgx_set_fixed_joint")

    def set_fixed_joint_ranges(self, ranges: int):
        """block ranges per MSM of the block table's accumulation (0 = automatic)"""
        _chk(lib().kzgx_set_fixed_joint_ranges(self.h, ranges), "kzgx_set_fixed_joint_ranges")

    def set_fixed_accum_reserve(self, r: int):
        """wave slots per CU that the block table's accumulation leaves free for the other
        stream's tail passes (-1 = the curve's default, 0 = none; clamped to what the device allows)"""
        _chk(lib().kzgx_set_fixed_accum_reserve(self.h, r), "kzgx_set_fixed_accum_reserve")

    def fixed_accum_reserve_info(self):
        """(request, reserve in effect, dynamic LDS bytes per accumulation workgroup that hold it)"""
        req = ctypes.c_int(0)
        r = ctypes.c_int(0)
        b = sz(0)
        _chk(lib().kzgx_fixed_accum_reserve_info(self.h, ctypes.byref(req), ctypes.byref(r), ctypes.byref(b), None),
             "kzgx_fixed_accum_reserve_info")
        return req.value, r.value, b.value

    def fixed_accum_variant(self):
        """the accumulation kernel the next block-table call launches: bit 0 = tests for entries at
        infinity, bit 1 = the endomorphism split's"""
        v = ctypes.c_int(0)
        _chk(lib().kzgx_fixed_accum_reserve_info(self.h, None, None, None, ctypes.byref(v)),
             "kzgx_fixed_accum_reserve_info")
        return v.value

    def fixed_joint_info(self):
        """(block size g, blocks, device bytes) of the built block table, g = 0: none"""
        g = ctypes.c_int(0)
        n = sz(0)
        b = sz(0)
        _chk(lib().kzgx_fixed_joint_info(self.h, ctypes.byref(g), ctypes.byref(n), ctypes.byref(b)),
             "kzgx_fixed_joint_info")
        return g.value, n.value, b.value

    def fixed_window_info(self):
        """(window bits, device bytes) of the built window table itself"""
        c = ctypes.c_int(0)
        b = sz(0)
        _chk(lib().kzgx_fixed_window_info(self.h, ctypes.byref(c), ctypes.byref(b)), "kzgx_fixed_window_info")
        return c.value, b.value

    def set_fixed_base_budget(self, budget_bytes: int, n_points: int) -> int:
        """widest table window whose table fits budget_bytes and free device
        memory (0: none built, Pippenger); returns the window built"""
        c = ctypes.c_int(0)
        _chk(lib().kzgx_set_fixed_base_budget(self.h, int(budget_bytes), n_points, ctypes.byref(c)),
             "kzgx_set_fixed_base_budget")
        return c.value

    def microbench_mad_u64(self) -> float:
        """v_mad_u64_u32 lane operations / s (hardware issue ceiling)"""
        r = ctypes.c_double(0)
        _chk(lib().kzgx_microbench_mad_u64(self.h, ctypes.byref(r)), "kzgx_microbench_mad_u64")
        return r.value

    def microbench_mad_u64_clock(self):
        """(v_mad_u64_u32 lane operations / s, core GHz the ceiling ran at)"""
        r = ctypes.c_double(0)
        g = ctypes.c_double(0)
        _chk(lib().kzgx_microbench_mad_u64_clock(self.h, ctypes.byref(r), ctypes.byref(g)),
             "kzgx_microbench_mad_u64_clock")
        return r.value, g.value

    def clock_probe(self, d_out: int, spin_us: int, stream: int = 0):
        """enqueue the core-clock probe on stream; d_out: device address of 3 uint64"""
        _chk(lib().kzgx_clock_probe(self.h, ctypes.c_void_p(stream or None), spin_us, ctypes.c_void_p(d_out)),
             "kzgx_clock_probe")

    def set_fixed_points_per_thread(self, p: int):
        _chk(lib().kzgx_set_fixed_points_per_thread(self.h, p), "kzgx_set_fixed_points_per_thread")

    def microbench_mixed_add(self) -> float:
        """mixed additions / s of the accumulation loop at full occupancy"""
        r = ctypes.c_double(0)
        _chk(lib().kzgx_microbench_mixed_add(self.h, ctypes.byref(r)), "kzgx_microbench_mixed_add")
        return r.value

    def prof_clear(self):
        _chk(lib().kzgx_prof_clear(self.h), "kzgx_prof_clear")

    # ---- SRS ----
    @property
    def srs_size(self) -> int:
        return lib().kzgx_srs_size(self.h)

    def load_srs(self, xy: np.ndarray):
        xy = np.ascontiguousarray(xy, dtype=np.uint64).reshape(-1, 2 * self.w64)
        _chk(lib().kzgx_load_srs_g1(self.h, _p(xy), xy.shape[0]), "kzgx_load_srs_g1")

    def gen_srs(self, tau: int, n: int, start: int = 0):
        t = np.array([(tau >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)
        _chk(lib().kzgx_gen_srs_g1(self.h, _p(t), start, n), "kzgx_gen_srs_g1")

    def get_srs(self, n: int | None = None) -> np.ndarray:
        n = self.srs_size if n is None else n
        out = np.zeros((n, 2 * self.w64), dtype=np.uint64)
        _chk(lib().kzgx_get_srs_g1(self.h, _p(out), n), "kzgx_get_srs_g1")
        return out

    # ---- MSM ----
    def msm_batch(self, scalars: np.ndarray, n: int, batch: int):
        sc = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1)
        assert sc.size >= n * batch * 4
        out = np.zeros((batch, 2 * self.w64), dtype=np.uint64)
        inf = np.zeros(batch, dtype=np.int32)
        _chk(lib().kzgx_msm_g1_batch(self.h, _p(sc) if n else None, n, batch, _p(out),
                                     inf.ctypes.data_as(intp)), "kzgx_msm_g1_batch")
        return out, inf.astype(bool)

    def msm(self, scalars: np.ndarray):
        sc = as_scalars(scalars)
        out, inf = self.msm_batch(sc, sc.shape[0], 1)
        return out[0], bool(inf[0])

    def quotient_single_batch(self, coeffs, zs, shared: bool = True):
        """q_j = (P_j - P_j(z_j)) / (X - z_j) and y_j = P_j(z_j) (host buffers);
        coeffs: n x 4 (shared) or batch x n x 4 words -> (q: batch x (n-1) x 4, y: batch x 4)"""
        c = np.ascontiguousarray(coeffs, dtype=np.uint64)
        z = as_scalars(zs)
        batch = z.shape[0]
        n = c.shape[-2] if c.ndim == 3 else c.reshape(-1, 4).shape[0]
        stride = 0 if shared else n
        q = np.zeros((batch, max(n - 1, 0), 4), dtype=np.uint64)
        y = np.zeros((batch, 4), dtype=np.uint64)
        _chk(lib().kzgx_quotient_single_batch(self.h, _p(c) if n else None, n, stride, _p(z), batch,
                                              _p(q) if n > 1 else None, _p(y)), "kzgx_quotient_single_batch")
        return q, y

    def msm_batch_device(self, d_scalars: int, n: int, batch: int, stride: int, d_out: int, d_inf: int,
                         stream: int | None = None):
        _chk(lib().kzgx_msm_g1_batch_device(self.h, d_scalars, n, batch, stride, d_out, d_inf, stream),
             "kzgx_msm_g1_batch_device")

    # ---- proofs ----
    def prove_single_batch(self, coeffs: np.ndarray, zs: np.ndarray, shared: bool = True):
        """coeffs: (n, 4) shared polynomial (shared=True) or (batch, n, 4)."""
        zs = as_scalars(zs)
        batch = zs.shape[0]
        c = np.ascontiguousarray(coeffs, dtype=np.uint64)
        n = c.shape[-2] if c.ndim >= 2 else 0
        stride = 0 if shared else n
        out = np.zeros((batch, 2 * self.w64), dtype=np.uint64)
        inf = np.zeros(batch, dtype=np.int32)
        y = np.zeros((batch, 4), dtype=np.uint64)
        _chk(lib().kzgx_prove_single_batch(self.h, _p(c) if n else None, n, stride, _p(zs), batch, _p(out),
                                           inf.ctypes.data_as(intp), _p(y)), "kzgx_prove_single_batch")
        return out, inf.astype(bool), y

    def prove_single_batch_device(self, d_coeffs, n, stride, d_z, batch, d_out, d_inf, d_y=None, stream=None):
        _chk(lib().kzgx_prove_single_batch_device(self.h, d_coeffs, n, stride, d_z, batch, d_out, d_inf, d_y,
                                                  stream), "kzgx_prove_single_batch_device")

    def quotient_single_device(self, d_coeffs, n, stride, d_z, batch, d_q, q_stride, d_y=None, stream=None):
        _chk(lib().kzgx_quotient_single_batch_device(self.h, d_coeffs, n, stride, d_z, batch, d_q, q_stride, d_y,
                                                     stream), "kzgx_quotient_single_batch_device")

    def prove_range(self, coeffs: np.ndarray, xs: np.ndarray):
        """multi-point opening: MSM of (P - I) / Z for the points xs"""
        c = as_scalars(coeffs) if len(coeffs) else np.zeros((0, 4), dtype=np.uint64)
        x = as_scalars(xs)
        out = np.zeros(2 * self.w64, dtype=np.uint64)
        inf = ctypes.c_int(0)
        _chk(lib().kzgx_prove_range(self.h, _p(c) if c.shape[0] else None, c.shape[0], _p(x), x.shape[0], _p(out),
                                    ctypes.byref(inf)), "kzgx_prove_range")
        return out, bool(inf.value)

    # ---- poly ----
    def poly_eval(self, coeffs: np.ndarray, xs: np.ndarray) -> np.ndarray:
        c = as_scalars(coeffs) if len(coeffs) else np.zeros((0, 4), dtype=np.uint64)
        x = as_scalars(xs)
        y = np.zeros_like(x)
        _chk(lib().kzgx_poly_eval(self.h, _p(c) if c.shape[0] else None, c.shape[0], _p(x), x.shape[0], _p(y)),
             "kzgx_poly_eval")
        return y

    def interpolate(self, xs: np.ndarray, ys: np.ndarray) -> np.ndarray:
        x = as_scalars(xs)
        y = as_scalars(ys)
        out = np.zeros_like(x)
        _chk(lib().kzgx_poly_interpolate(self.h, _p(x), _p(y), x.shape[0], _p(out)), "kzgx_poly_interpolate")
        return out

    def vanishing(self, xs: np.ndarray) -> np.ndarray:
        x = as_scalars(xs)
        out = np.zeros((x.shape[0] + 1, 4), dtype=np.uint64)
        _chk(lib().kzgx_poly_vanishing(self.h, _p(x) if x.shape[0] else None, x.shape[0], _p(out)),
             "kzgx_poly_vanishing")
        return out

    def g1_validate(self, xy: np.ndarray) -> bool:
        xy = np.ascontiguousarray(xy, dtype=np.uint64).reshape(2 * self.w64)
        ok = ctypes.c_int(0)
        _chk(lib().kzgx_g1_validate(self.h, _p(xy), ctypes.byref(ok)), "kzgx_g1_validate")
        return bool(ok.value)

    def g1_sum(self, pts: np.ndarray, inf=None):
        pts = np.ascontiguousarray(pts, dtype=np.uint64).reshape(-1, 2 * self.w64)
        f = None if inf is None else np.ascontiguousarray(inf, dtype=np.int32)
        out = np.zeros(2 * self.w64, dtype=np.uint64)
        oi = ctypes.c_int(0)
        _chk(lib().kzgx_g1_sum(self.h, _p(pts), None if f is None else f.ctypes.data_as(intp), pts.shape[0],
                               _p(out), ctypes.byref(oi)), "kzgx_g1_sum")
        return out, bool(oi.value)

    def g1_sum_device(self, d_xy: int, d_inf: int | None, count: int, d_out: int, d_out_inf: int,
                      stream: int | None = None):
        """Fold of count device-resident canonical points (uint32 infinity flags) on stream."""
        _chk(lib().kzgx_g1_sum_device(self.h, d_xy, d_inf, count, d_out, d_out_inf, stream), "kzgx_g1_sum_device")

    def g1_sum_packed_device(self, d_rec: int, count: int, d_out: int, stream: int | None = None):
        """Fold of count packed records (2 W64 uint64 x || y, then a uint64 infinity word) into one
        record at d_out, on stream (the sharded commitment's exchange format)."""
        _chk(lib().kzgx_g1_sum_packed_device(self.h, d_rec, count, d_out, stream), "kzgx_g1_sum_packed_device")

    @property
    def partial_record_words(self) -> int:
        """uint64 words of one projective partial record (kzgx_partial_record_words)"""
        return lib().kzgx_partial_record_words(CURVES[self.curve])

    def msm_partial_device(self, d_scalars: int, n: int, d_rec: int, stream: int | None = None):
        """kzgx_msm_g1_partial_device: sum_i s_i SRS_i as one XYZZ record at d_rec (no inversion)."""
        _chk(lib().kzgx_msm_g1_partial_device(self.h, d_scalars, n, d_rec, stream), "kzgx_msm_g1_partial_device")

    def g1_sum_partials_device(self, d_rec: int, count: int, d_out: int, stream: int | None = None):
        """kzgx_g1_sum_partials_device: count XYZZ records -> one packed affine record at d_out."""
        _chk(lib().kzgx_g1_sum_partials_device(self.h, d_rec, count, d_out, stream), "kzgx_g1_sum_partials_device")

    def init_device(self):
        """kzgx_init_device for this context's curve and device (ADVICE r05:
        the module-level init_device(curve, device) takes them explicitly)."""
        init_device(self.curve, self.device)

    # ---- verify half: G2 setup, polyeval_G2, pairing ----
    # G2 points: (n, 4 * W64) uint64 = x.re || x.im || y.re || y.im; Fp12: (12 * W64,)
    @property
    def srs2_size(self) -> int:
        return lib().kzgx_srs_g2_size(self.h)

    def gen_srs_g2(self, tau: int, n: int, start: int = 0):
        t = np.array([(tau >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)
        _chk(lib().kzgx_gen_srs_g2(self.h, _p(t), start, n), "kzgx_gen_srs_g2")

    def load_srs_g2(self, xy: np.ndarray):
        xy = np.ascontiguousarray(xy, dtype=np.uint64).reshape(-1, 4 * self.w64)
        _chk(lib().kzgx_load_srs_g2(self.h, _p(xy), xy.shape[0]), "kzgx_load_srs_g2")

    def get_srs_g2(self, n: int | None = None) -> np.ndarray:
        n = self.srs2_size if n is None else n
        out = np.zeros((n, 4 * self.w64), dtype=np.uint64)
        _chk(lib().kzgx_get_srs_g2(self.h, _p(out), n), "kzgx_get_srs_g2")
        return out

    def g2_validate(self, xy: np.ndarray) -> np.ndarray:
        xy = np.ascontiguousarray(xy, dtype=np.uint64).reshape(-1, 4 * self.w64)
        ok = np.zeros(xy.shape[0], dtype=np.int32)
        _chk(lib().kzgx_g2_validate(self.h, _p(xy), xy.shape[0], ok.ctypes.data_as(intp)), "kzgx_g2_validate")
        return ok.astype(bool)

    def msm_g2(self, scalars: np.ndarray):
        sc = as_scalars(scalars) if len(scalars) else np.zeros((0, 4), dtype=np.uint64)
        out = np.zeros(4 * self.w64, dtype=np.uint64)
        inf = ctypes.c_int(0)
        _chk(lib().kzgx_msm_g2(self.h, _p(sc) if sc.shape[0] else None, sc.shape[0], _p(out), ctypes.byref(inf)),
             "kzgx_msm_g2")
        return out, bool(inf.value)

    def pairing(self, g1: np.ndarray, g2: np.ndarray, g1_inf=None, g2_inf=None) -> np.ndarray:
        a = np.ascontiguousarray(g1, dtype=np.uint64).reshape(-1, 2 * self.w64)
        b = np.ascontiguousarray(g2, dtype=np.uint64).reshape(-1, 4 * self.w64)
        assert a.shape[0] == b.shape[0]
        fa = None if g1_inf is None else np.ascontiguousarray(g1_inf, dtype=np.int32)
        fb = None if g2_inf is None else np.ascontiguousarray(g2_inf, dtype=np.int32)
        out = np.zeros((a.shape[0], 12 * self.w64), dtype=np.uint64)
        _chk(lib().kzgx_pairing(self.h, _p(a), None if fa is None else fa.ctypes.data_as(intp), _p(b),
                                None if fb is None else fb.ctypes.data_as(intp), a.shape[0], _p(out)),
             "kzgx_pairing")
        return out

    def verify_proof(self, commit, commit_inf: bool, proof, proof_inf: bool, xs, ys) -> bool:
        c = np.ascontiguousarray(commit, dtype=np.uint64).reshape(2 * self.w64)
        p = np.ascontiguousarray(proof, dtype=np.uint64).reshape(2 * self.w64)
        x = as_scalars(xs) if len(xs) else np.zeros((0, 4), dtype=np.uint64)
        y = as_scalars(ys) if len(ys) else np.zeros((0, 4), dtype=np.uint64)
        ok = ctypes.c_int(0)
        _chk(lib().kzgx_verify_proof(self.h, _p(c), int(commit_inf), _p(p), int(proof_inf),
                                     _p(x) if x.shape[0] else None, _p(y) if y.shape[0] else None, x.shape[0],
                                     ctypes.byref(ok)), "kzgx_verify_proof")
        return bool(ok.value)

    def verify_single_batch(self, commits, proofs, zs, ys, commit_inf=None, proof_inf=None) -> np.ndarray:
        c = np.ascontiguousarray(commits, dtype=np.uint64).reshape(-1, 2 * self.w64)
        p = np.ascontiguousarray(proofs, dtype=np.uint64).reshape(-1, 2 * self.w64)
        z, y = as_scalars(zs), as_scalars(ys)
        n = c.shape[0]
        assert p.shape[0] == n and z.shape[0] == n and y.shape[0] == n
        fc = None if commit_inf is None else np.ascontiguousarray(commit_inf, dtype=np.int32)
        fp = None if proof_inf is None else np.ascontiguousarray(proof_inf, dtype=np.int32)
        ok = np.zeros(n, dtype=np.int32)
        _chk(lib().kzgx_verify_single_batch(self.h, _p(c), None if fc is None else fc.ctypes.data_as(intp), _p(p),
                                            None if fp is None else fp.ctypes.data_as(intp), _p(z), _p(y), n,
                                            ok.ctypes.data_as(intp)), "kzgx_verify_single_batch")
        return ok.astype(bool)

    def set_verify_wave_max(self, max_count: int) -> None:
        """batches of <= max_count openings run a wave per opening (0: a lane each)"""
        _chk(lib().kzgx_set_verify_wave_max(self.h, max_count), "kzgx_set_verify_wave_max")

    def verify_single_batch_device(self, d_commits, d_commit_inf, d_proofs, d_proof_inf, d_z, d_y, count, d_ok,
                                   stream=None):
        _chk(lib().kzgx_verify_single_batch_device(self.h, d_commits, d_commit_inf, d_proofs, d_proof_inf, d_z, d_y,
                                                   count, d_ok, stream), "kzgx_verify_single_batch_device")

    # ---- variable-base MSM over caller points, aggregated verification ----
    def msm_points(self, points, scalars, inf=None):
        """sum_k scalars[k] * points[k] over caller-supplied canonical affine points (no SRS needed)."""
        pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 2 * self.w64)
        n = pts.shape[0]
        sc = as_scalars(scalars) if n else np.zeros((0, 4), dtype=np.uint64)
        assert sc.shape[0] == n
        f = None if inf is None else np.ascontiguousarray(inf, dtype=np.int32)
        out = np.zeros(2 * self.w64, dtype=np.uint64)
        oi = ctypes.c_int(0)
        _chk(lib().kzgx_msm_g1_points(self.h, _p(pts) if n else None, None if f is None else f.ctypes.data_as(intp),
                                      _p(sc) if n else None, n, _p(out), ctypes.byref(oi)), "kzgx_msm_g1_points")
        return out, bool(oi.value)

    def msm_points_device(self, d_points, d_inf, d_scalars, n, d_out, d_out_inf, stream=None):
        """kzgx_msm_g1_points_device: device pointers (uint32 infinity flags or None), enqueued on stream."""
        _chk(lib().kzgx_msm_g1_points_device(self.h, d_points, d_inf, d_scalars, n, d_out, d_out_inf, stream),
             "kzgx_msm_g1_points_device")

    def verify_aggregate(self, commits, proofs, zs, ys, challenges=None, commit_inf=None, proof_inf=None) -> bool:
        """One pairing check of e(sum r_k proof_k, [tau]G2) == e(sum r_k (C_k - [y_k]G + [z_k] proof_k), G2);
        challenges None = the library draws 128-bit values (r_0 = 1)."""
        c = np.ascontiguousarray(commits, dtype=np.uint64).reshape(-1, 2 * self.w64)
        p = np.ascontiguousarray(proofs, dtype=np.uint64).reshape(-1, 2 * self.w64)
        n = c.shape[0]
        z = as_scalars(zs) if n else np.zeros((0, 4), dtype=np.uint64)
        y = as_scalars(ys) if n else np.zeros((0, 4), dtype=np.uint64)
        r = None if challenges is None else (as_scalars(challenges) if n else np.zeros((0, 4), dtype=np.uint64))
        assert p.shape[0] == n and z.shape[0] == n and y.shape[0] == n and (r is None or r.shape[0] == n)
        fc = None if commit_inf is None else np.ascontiguousarray(commit_inf, dtype=np.int32)
        fp = None if proof_inf is None else np.ascontiguousarray(proof_inf, dtype=np.int32)
        ok = ctypes.c_int(0)
        _chk(lib().kzgx_verify_aggregate(self.h, _p(c) if n else None, None if fc is None else fc.ctypes.data_as(intp),
                                         _p(p) if n else None, None if fp is None else fp.ctypes.data_as(intp),
                                         _p(z) if n else None, _p(y) if n else None,
                                         None if r is None or not n else _p(r), n, ctypes.byref(ok)),
             "kzgx_verify_aggregate")
        return bool(ok.value)

    def verify_aggregate_device(self, d_commits, d_commit_inf, d_proofs, d_proof_inf, d_z, d_y, d_challenges, count,
                                d_ok, stream=None):
        """kzgx_verify_aggregate_device: device pointers, d_ok one uint32, enqueued on stream."""
        _chk(lib().kzgx_verify_aggregate_device(self.h, d_commits, d_commit_inf, d_proofs, d_proof_inf, d_z, d_y,
                                                d_challenges, count, d_ok, stream), "kzgx_verify_aggregate_device")

    # ---- batched point validation, prime-order subgroup checks ----
    def _check_batch(self, fn, name, width, pts, inf, subgroup) -> np.ndarray:
        xy = np.ascontiguousarray(pts, dtype=np.uint64).reshape(-1, width)
        n = xy.shape[0]
        f = None if inf is None else np.ascontiguousarray(inf, dtype=np.int32)
        assert f is None or f.shape[0] == n
        ok = np.zeros(n, dtype=np.int32)
        _chk(fn(self.h, _p(xy) if n else None, None if f is None else f.ctypes.data_as(intp), n, int(bool(subgroup)),
                ok.ctypes.data_as(intp)), name)
        return ok.astype(bool)

    def g1_check(self, pts, inf=None, subgroup: bool = False) -> np.ndarray:
        """kzgx_g1_check_batch: per point, canonical + on the curve (+ in the order-r subgroup);
        infinite entries (flag or all-zero) pass."""
        return self._check_batch(lib().kzgx_g1_check_batch, "kzgx_g1_check_batch", 2 * self.w64, pts, inf, subgroup)

    def g1_check_device(self, d_xy, d_inf, count, subgroup, d_ok, d_all_ok, stream=None):
        """kzgx_g1_check_batch_device: device pointers (d_ok count x uint32, d_all_ok one uint32,
        either may be None), enqueued on stream."""
        _chk(lib().kzgx_g1_check_batch_device(self.h, d_xy, d_inf, count, int(bool(subgroup)), d_ok, d_all_ok, stream),
             "kzgx_g1_check_batch_device")

    def g2_check(self, pts, inf=None, subgroup: bool = False) -> np.ndarray:
        """kzgx_g2_check_batch: the same for G2 points on the twist."""
        return self._check_batch(lib().kzgx_g2_check_batch, "kzgx_g2_check_batch", 4 * self.w64, pts, inf, subgroup)

    def srs_check(self, subgroup: bool = True):
        """kzgx_srs_check: (g1_ok, g2_ok) over every installed SRS point, on the device."""
        a, b = ctypes.c_int(0), ctypes.c_int(0)
        _chk(lib().kzgx_srs_check(self.h, int(bool(subgroup)), ctypes.byref(a), ctypes.byref(b)), "kzgx_srs_check")
        return bool(a.value), bool(b.value)

    # ---- setup ceremony ----
    def srs_update(self, s: int, g1_start: int = 0, g2_start: int = 0, witness: bool = True):
        """kzgx_srs_update: G1[i] <- [s^(g1_start+i)] G1[i], G2[j] <- [s^(g2_start+j)] G2[j] on the device,
        then the install path of a loaded setup; -> the witness [s]G2gen (4 * W64 words), or None."""
        t = np.array([(s >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)
        w = np.zeros(4 * self.w64, dtype=np.uint64) if witness else None
        _chk(lib().kzgx_srs_update(self.h, _p(t), g1_start, g2_start, _p(w)), "kzgx_srs_update")
        return w

    def srs_verify_structure(self, rho: int | None = None, sigma: int | None = None, generators: bool = False):
        """kzgx_srs_verify_structure: (g1_ok, g2_ok), the installed points are consecutive powers of one
        tau; rho / sigma None = drawn by the library, explicit = exactly the documented equations."""
        ch = [None if v is None else np.array([(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)],
                                              dtype=np.uint64) for v in (rho, sigma)]
        a, b = ctypes.c_int(0), ctypes.c_int(0)
        _chk(lib().kzgx_srs_verify_structure(self.h, _p(ch[0]), _p(ch[1]), SRS_STRUCT_GENERATORS if generators else 0,
                                             ctypes.byref(a), ctypes.byref(b)), "kzgx_srs_verify_structure")
        return bool(a.value), bool(b.value)

    def srs_verify_update(self, prev_tau_g1, new_tau_g1, witness_g2) -> bool:
        """kzgx_srs_verify_update: e(new, G2gen) == e(prev, W), W and new finite (all-zero = infinity)."""
        p = np.ascontiguousarray(prev_tau_g1, dtype=np.uint64).reshape(2 * self.w64)
        q = np.ascontiguousarray(new_tau_g1, dtype=np.uint64).reshape(2 * self.w64)
        w = np.ascontiguousarray(witness_g2, dtype=np.uint64).reshape(4 * self.w64)
        ok = ctypes.c_int(0)
        _chk(lib().kzgx_srs_verify_update(self.h, _p(p), _p(q), _p(w), ctypes.byref(ok)), "kzgx_srs_verify_update")
        return bool(ok.value)

    def verify_aggregate_checked(self, commits, proofs, zs, ys, challenges=None, commit_inf=None, proof_inf=None,
                                 subgroup: bool = True) -> bool:
        """verify_aggregate behind the G1 check of every commit and proof (False if one fails)."""
        c = np.ascontiguousarray(commits, dtype=np.uint64).reshape(-1, 2 * self.w64)
        p = np.ascontiguousarray(proofs, dtype=np.uint64).reshape(-1, 2 * self.w64)
        n = c.shape[0]
        z = as_scalars(zs) if n else np.zeros((0, 4), dtype=np.uint64)
        y = as_scalars(ys) if n else np.zeros((0, 4), dtype=np.uint64)
        r = None if challenges is None else (as_scalars(challenges) if n else np.zeros((0, 4), dtype=np.uint64))
        assert p.shape[0] == n and z.shape[0] == n and y.shape[0] == n and (r is None or r.shape[0] == n)
        fc = None if commit_inf is None else np.ascontiguousarray(commit_inf, dtype=np.int32)
        fp = None if proof_inf is None else np.ascontiguousarray(proof_inf, dtype=np.int32)
        ok = ctypes.c_int(0)
        _chk(lib().kzgx_verify_aggregate_checked(
            self.h, _p(c) if n else None, None if fc is None else fc.ctypes.data_as(intp), _p(p) if n else None,
            None if fp is None else fp.ctypes.data_as(intp), _p(z) if n else None, _p(y) if n else None,
            None if r is None or not n else _p(r), n, int(bool(subgroup)), ctypes.byref(ok)),
            "kzgx_verify_aggregate_checked")
        return bool(ok.value)

    def verify_aggregate_checked_device(self, d_commits, d_commit_inf, d_proofs, d_proof_inf, d_z, d_y, d_challenges,
                                        count, subgroup, d_ok, stream=None):
        """kzgx_verify_aggregate_checked_device: device pointers, d_ok one uint32, enqueued on stream."""
        _chk(lib().kzgx_verify_aggregate_checked_device(self.h, d_commits, d_commit_inf, d_proofs, d_proof_inf, d_z,
                                                        d_y, d_challenges, count, int(bool(subgroup)), d_ok, stream),
             "kzgx_verify_aggregate_checked_device")

    # ---- batch openings: many polynomials at shared points, one proof each ----
    def prove_multi(self, polys, poly_index, group_start, zs, weights, powers: bool = False, n: int | None = None,
                    want_y: bool = True):
        """kzgx_prove_multi_batch.  polys: (n_polys, stride, 4), the first n coefficients of a row used (n = stride
        by default); claim k names polys[poly_index[k]], group g holds the claims group_start[g] .. group_start[g+1]
        and opens at zs[g]; weights: one scalar per claim, or one gamma per group with powers.  Returns the
        n_groups proofs, their infinity flags, the count values y_k (None without want_y) and the n_groups Y_g."""
        c = np.ascontiguousarray(polys, dtype=np.uint64)
        assert c.ndim == 3 and c.shape[2] == 4
        n_polys, stride = c.shape[0], c.shape[1]
        n = stride if n is None else n
        pi = np.ascontiguousarray(poly_index, dtype=np.uint32).reshape(-1)
        gs = np.ascontiguousarray(group_start, dtype=np.uint32).reshape(-1)
        count, n_groups = pi.shape[0], gs.shape[0] - 1
        z = as_scalars(zs) if n_groups else np.zeros((0, 4), dtype=np.uint64)
        w = np.ascontiguousarray(weights, dtype=np.uint64).reshape(-1, 4)
        assert z.shape[0] == n_groups and w.shape[0] == (n_groups if powers else count)
        out = np.zeros((n_groups, 2 * self.w64), dtype=np.uint64)
        inf = np.zeros(n_groups, dtype=np.int32)
        y = np.zeros((count, 4), dtype=np.uint64) if want_y else None
        Y = np.zeros((n_groups, 4), dtype=np.uint64)
        _chk(lib().kzgx_prove_multi_batch(self.h, _p(c), n, stride, n_polys, pi.ctypes.data_as(u32p),
                                          gs.ctypes.data_as(u32p), n_groups, _p(z), _p(w), count,
                                          MULTI_WEIGHT_POWERS if powers else 0, _p(out), inf.ctypes.data_as(intp),
                                          _p(y), _p(Y)), "kzgx_prove_multi_batch")
        return out, inf.astype(bool), y, Y

    def prove_multi_device(self, d_coeffs, n, stride, n_polys, d_poly_index, d_group_start, n_groups, d_zs, d_weights,
                           count, d_out, d_inf, d_y=None, d_Y=None, d_ok=None, powers=False, stream=None):
        """kzgx_prove_multi_batch_device: device pointers (indices uint32), d_ok one uint32 or None, enqueued on
        stream."""
        _chk(lib().kzgx_prove_multi_batch_device(self.h, d_coeffs, n, stride, n_polys, d_poly_index, d_group_start,
                                                 n_groups, d_zs, d_weights, count,
                                                 MULTI_WEIGHT_POWERS if powers else 0, d_out, d_inf, d_y, d_Y, d_ok,
                                                 stream), "kzgx_prove_multi_batch_device")

    def verify_multi(self, commits, commit_index, group_start, zs, ys, weights, proofs, challenges=None,
                     powers: bool = False, commit_inf=None, proof_inf=None, checked: bool = False,
                     subgroup: int = 0) -> bool:
        """kzgx_verify_multi_batch(_checked): one pairing check of the n_groups proofs against the count claimed
        values ys of the commitments commits[commit_index[k]]; challenges: one scalar per group, None = the
        library draws 128-bit values (r_0 = 1); checked: the G1 check of every commitment and proof in front."""
        c = np.ascontiguousarray(commits, dtype=np.uint64).reshape(-1, 2 * self.w64)
        p = np.ascontiguousarray(proofs, dtype=np.uint64).reshape(-1, 2 * self.w64)
        ci = np.ascontiguousarray(commit_index, dtype=np.uint32).reshape(-1)
        gs = np.ascontiguousarray(group_start, dtype=np.uint32).reshape(-1)
        count, n_groups, n_commits = ci.shape[0], gs.shape[0] - 1, c.shape[0]
        z = as_scalars(zs) if n_groups else np.zeros((0, 4), dtype=np.uint64)
        y = as_scalars(ys) if count else np.zeros((0, 4), dtype=np.uint64)
        w = np.ascontiguousarray(weights, dtype=np.uint64).reshape(-1, 4)
        r = None if challenges is None else np.ascontiguousarray(challenges, dtype=np.uint64).reshape(-1, 4)
        assert p.shape[0] == n_groups and z.shape[0] == n_groups and y.shape[0] == count
        assert w.shape[0] == (n_groups if powers else count) and (r is None or r.shape[0] == n_groups)
        fc = None if commit_inf is None else np.ascontiguousarray(commit_inf, dtype=np.int32)
        fp = None if proof_inf is None else np.ascontiguousarray(proof_inf, dtype=np.int32)
        ok = ctypes.c_int(0)
        args = [self.h, _p(c), None if fc is None else fc.ctypes.data_as(intp), n_commits, ci.ctypes.data_as(u32p),
                gs.ctypes.data_as(u32p), n_groups, _p(z), _p(y), _p(w), _p(p),
                None if fp is None else fp.ctypes.data_as(intp), _p(r), count, MULTI_WEIGHT_POWERS if powers else 0]
        if checked:
            _chk(lib().kzgx_verify_multi_batch_checked(*args, int(bool(subgroup)), ctypes.byref(ok)),
                 "kzgx_verify_multi_batch_checked")
        else:
            _chk(lib().kzgx_verify_multi_batch(*args, ctypes.byref(ok)), "kzgx_verify_multi_batch")
        return bool(ok.value)

    def verify_multi_device(self, d_commits, d_commit_inf, n_commits, d_commit_index, d_group_start, n_groups, d_zs,
                            d_ys, d_weights, d_proofs, d_proof_inf, d_challenges, count, d_ok, powers=False,
                            checked=False, subgroup=0, stream=None):
        """kzgx_verify_multi_batch(_checked)_device: device pointers, d_ok one uint32, enqueued on stream."""
        args = [self.h, d_commits, d_commit_inf, n_commits, d_commit_index, d_group_start, n_groups, d_zs, d_ys,
                d_weights, d_proofs, d_proof_inf, d_challenges, count, MULTI_WEIGHT_POWERS if powers else 0]
        if checked:
            _chk(lib().kzgx_verify_multi_batch_checked_device(*args, int(bool(subgroup)), d_ok, stream),
                 "kzgx_verify_multi_batch_checked_device")
        else:
            _chk(lib().kzgx_verify_multi_batch_device(*args, d_ok, stream), "kzgx_verify_multi_batch_device")

    def set_multi_chunk(self, scalars: int) -> None:
        """test knob: scalars of folded polynomials per internal chunk of prove_multi (0 = the default)"""
        _chk(lib().kzgx_set_multi_chunk(self.h, scalars), "kzgx_set_multi_chunk")

    # ---- Shplonk openings: many polynomials at different point sets, one two-point proof ----
    @staticmethod
    def _shplonk_table(points, sets):
        """sets: a list of (point indices, claim indices) pairs -> points, set_point_start, set_points,
        claim_start, claim index array (uint32)"""
        t = as_scalars(points)
        sps, sp, cs, ix = [0], [], [0], []
        for pts, claims in sets:
            sp += [int(v) for v in pts]
            ix += [int(v) for v in claims]
            sps.append(len(sp))
            cs.append(len(ix))
        u32 = lambda v: np.ascontiguousarray(np.array(v, dtype=np.uint32).reshape(-1))  # noqa: E731
        return t, u32(sps), u32(sp), u32(cs), u32(ix)

    def shplonk_commit(self, polys, points, sets, weights, powers: bool = False, n: int | None = None,
                       want_y: bool = True):
        """kzgx_shplonk_commit.  polys: (n_polys, stride, 4), the first n coefficients of a row used; points: T;
        sets: a list of (indices into T, polynomial indices of the set's claims); weights: one scalar per claim,
        or one gamma with powers (w_k = gamma^k).  Returns W, its infinity flag, h ((n, 4)) and the values
        ((n_values, 4), claim by claim in the set's point order; None without want_y)."""
        c = np.ascontiguousarray(polys, dtype=np.uint64)
        assert c.ndim == 3 and c.shape[2] == 4
        n_polys, stride = c.shape[0], c.shape[1]
        n = stride if n is None else n
        t, sps, sp, cs, pi = self._shplonk_table(points, sets)
        w = np.ascontiguousarray(weights, dtype=np.uint64).reshape(-1, 4)
        count = pi.shape[0]
        assert w.shape[0] == (1 if powers else count)
        n_values = sum(len(p) * len(k) for p, k in sets)
        out = np.zeros(2 * self.w64, dtype=np.uint64)
        inf = ctypes.c_int(0)
        h = np.zeros((n, 4), dtype=np.uint64)
        y = np.zeros((n_values, 4), dtype=np.uint64) if want_y else None
        _chk(lib().kzgx_shplonk_commit(self.h, _p(c), n, stride, n_polys, _p(t), t.shape[0],
                                       sps.ctypes.data_as(u32p), sp.ctypes.data_as(u32p), sp.shape[0],
                                       cs.ctypes.data_as(u32p), pi.ctypes.data_as(u32p), len(sets), _p(w), count,
                                       n_values, SHPLONK_WEIGHT_POWERS if powers else 0, _p(out), ctypes.byref(inf),
                                       _p(h), _p(y)), "kzgx_shplonk_commit")
        return out, bool(inf.value), h, y

    def shplonk_commit_device(self, d_coeffs, n, stride, n_polys, d_points, n_points, d_set_point_start, d_set_points,
                              n_set_points, d_claim_start, d_poly_index, n_sets, d_weights, count, n_values, d_out,
                              d_inf, d_h, d_y=None, d_ok=None, powers=False, stream=None):
        """kzgx_shplonk_commit_device: device pointers (indices uint32), d_ok one uint32 or None, enqueued on
        stream."""
        _chk(lib().kzgx_shplonk_commit_device(self.h, d_coeffs, n, stride, n_polys, d_points, n_points,
                                              d_set_point_start, d_set_points, n_set_points, d_claim_start,
                                              d_poly_index, n_sets, d_weights, count, n_values,
                                              SHPLONK_WEIGHT_POWERS if powers else 0, d_out, d_inf, d_h, d_y, d_ok,
                                              stream), "kzgx_shplonk_commit_device")

    def shplonk_open(self, polys, points, sets, weights, h, z, powers: bool = False, n: int | None = None):
        """kzgx_shplonk_open: the table of shplonk_commit, its h and the challenge z.  Returns W', its infinity
        flag and G(z)."""
        c = np.ascontiguousarray(polys, dtype=np.uint64)
        assert c.ndim == 3 and c.shape[2] == 4
        n_polys, stride = c.shape[0], c.shape[1]
        n = stride if n is None else n
        t, sps, sp, cs, pi = self._shplonk_table(points, sets)
        w = np.ascontiguousarray(weights, dtype=np.uint64).reshape(-1, 4)
        count = pi.shape[0]
        assert w.shape[0] == (1 if powers else count)
        hh = np.ascontiguousarray(h, dtype=np.uint64).reshape(-1, 4)
        assert hh.shape[0] == n
        zz = as_scalars(z).reshape(-1, 4)
        out = np.zeros(2 * self.w64, dtype=np.uint64)
        inf = ctypes.c_int(0)
        gz = np.zeros(4, dtype=np.uint64)
        _chk(lib().kzgx_shplonk_open(self.h, _p(c), n, stride, n_polys, _p(t), t.shape[0], sps.ctypes.data_as(u32p),
                                     sp.ctypes.data_as(u32p), sp.shape[0], cs.ctypes.data_as(u32p),
                                     pi.ctypes.data_as(u32p), len(sets), _p(w), count,
                                     SHPLONK_WEIGHT_POWERS if powers else 0, _p(hh), _p(zz), _p(out),
                                     ctypes.byref(inf), _p(gz)), "kzgx_shplonk_open")
        return out, bool(inf.value), gz

    def shplonk_open_device(self, d_coeffs, n, stride, n_polys, d_points, n_points, d_set_point_start, d_set_points,
                            n_set_points, d_claim_start, d_poly_index, n_sets, d_weights, count, d_h, d_z, d_out,
                            d_inf, d_Gz=None, d_ok=None, powers=False, stream=None):
        """kzgx_shplonk_open_device: device pointers, d_ok one uint32 or None, enqueued on stream."""
        _chk(lib().kzgx_shplonk_open_device(self.h, d_coeffs, n, stride, n_polys, d_points, n_points,
                                            d_set_point_start, d_set_points, n_set_points, d_claim_start,
                                            d_poly_index, n_sets, d_weights, count,
                                            SHPLONK_WEIGHT_POWERS if powers else 0, d_h, d_z, d_out, d_inf, d_Gz, d_ok,
                                            stream), "kzgx_shplonk_open_device")

    def shplonk_verify(self, commits, points, sets, ys, weights, z, proof, powers: bool = False, commit_inf=None,
                       proof_inf=None, checked: bool = False, subgroup: int = 0) -> bool:
        """kzgx_shplonk_verify(_checked): sets as for shplonk_commit with commitment indices for the claims; ys: the
        n_values values in shplonk_commit's layout; proof: W then W' ((2, 2 * w64)); checked: the G1 check of
        every commitment, W and W' in front."""
        c = np.ascontiguousarray(commits, dtype=np.uint64).reshape(-1, 2 * self.w64)
        p = np.ascontiguousarray(proof, dtype=np.uint64).reshape(-1, 2 * self.w64)
        assert p.shape[0] == 2
        t, sps, sp, cs, ci = self._shplonk_table(points, sets)
        count, n_commits = ci.shape[0], c.shape[0]
        n_values = sum(len(a) * len(b) for a, b in sets)
        y = as_scalars(ys) if n_values else np.zeros((0, 4), dtype=np.uint64)
        w = np.ascontiguousarray(weights, dtype=np.uint64).reshape(-1, 4)
        assert y.shape[0] == n_values and w.shape[0] == (1 if powers else count)
        zz = as_scalars(z).reshape(-1, 4)
        fc = None if commit_inf is None else np.ascontiguousarray(commit_inf, dtype=np.int32)
        fp = None if proof_inf is None else np.ascontiguousarray(proof_inf, dtype=np.int32)
        ok = ctypes.c_int(0)
        args = [self.h, _p(c), None if fc is None else fc.ctypes.data_as(intp), n_commits, ci.ctypes.data_as(u32p),
                _p(t), t.shape[0], sps.ctypes.data_as(u32p), sp.ctypes.data_as(u32p), sp.shape[0],
                cs.ctypes.data_as(u32p), len(sets), _p(y), n_values, _p(w), count, _p(zz), _p(p),
                None if fp is None else fp.ctypes.data_as(intp), SHPLONK_WEIGHT_POWERS if powers else 0]
        if checked:
            _chk(lib().kzgx_shplonk_verify_checked(*args, int(bool(subgroup)), ctypes.byref(ok)),
                 "kzgx_shplonk_verify_checked")
        else:
            _chk(lib().kzgx_shplonk_verify(*args, ctypes.byref(ok)), "kzgx_shplonk_verify")
        return bool(ok.value)

    def shplonk_verify_device(self, d_commits, d_commit_inf, n_commits, d_commit_index, d_points, n_points,
                              d_set_point_start, d_set_points, n_set_points, d_claim_start, n_sets, d_ys, n_values,
                              d_weights, count, d_z, d_proof, d_proof_inf, d_ok, powers=False, checked=False,
                              subgroup=0, stream=None):
        """kzgx_shplonk_verify(_checked)_device: device pointers, d_ok one uint32, enqueued on stream."""
        args = [self.h, d_commits, d_commit_inf, n_commits, d_commit_index, d_points, n_points, d_set_point_start,
                d_set_points, n_set_points, d_claim_start, n_sets, d_ys, n_values, d_weights, count, d_z, d_proof,
                d_proof_inf, SHPLONK_WEIGHT_POWERS if powers else 0]
        if checked:
            _chk(lib().kzgx_shplonk_verify_checked_device(*args, int(bool(subgroup)), d_ok, stream),
                 "kzgx_shplonk_verify_checked_device")
        else:
            _chk(lib().kzgx_shplonk_verify_device(*args, d_ok, stream), "kzgx_shplonk_verify_device")

    def set_shplonk_chunk(self, scalars: int) -> None:
        """test knob: scalars of folded polynomials per internal chunk of shplonk_commit (0 = the default)"""
        _chk(lib().kzgx_set_shplonk_chunk(self.h, scalars), "kzgx_set_shplonk_chunk")

    # ---- evaluation form: Fr NTT, commits and openings from evaluations ----
    def ntt(self, a, inverse: bool = False, bitrev: bool = False) -> np.ndarray:
        """kzgx_ntt of one transform ((n, 4) input) or a batch ((batch, n, 4)); n a power of two.
        bitrev: the evaluation side (forward output, inverse input) is in bit-reversed order."""
        x = np.ascontiguousarray(a, dtype=np.uint64)
        if x.ndim == 2:
            x = x.reshape(1, -1, 4)
        batch, n = x.shape[0], x.shape[1]
        out = np.zeros_like(x)
        _chk(lib().kzgx_ntt(self.h, _p(x), _log2_exact(n), batch, _ntt_flags(inverse, bitrev), _p(out)), "kzgx_ntt")
        return out.reshape(np.shape(a))

    def ntt_device(self, d_in, in_stride, d_out, out_stride, log2n, batch, inverse=False, bitrev=False, stream=None):
        """kzgx_ntt_device: device pointers, strides in scalars, enqueued on stream (d_in == d_out allowed)."""
        _chk(lib().kzgx_ntt_device(self.h, d_in, in_stride, d_out, out_stride, log2n, batch,
                                   _ntt_flags(inverse, bitrev), stream), "kzgx_ntt_device")

    def commit_evals(self, evals, bitrev: bool = False):
        """kzgx_commit_evals_batch: evals (batch, n, 4) -> (xy, is_inf), the commits of the interpolants."""
        e = np.ascontiguousarray(evals, dtype=np.uint64)
        if e.ndim == 2:
            e = e.reshape(1, -1, 4)
        batch, n = e.shape[0], e.shape[1]
        out = np.zeros((batch, 2 * self.w64), dtype=np.uint64)
        inf = np.zeros(batch, dtype=np.int32)
        _chk(lib().kzgx_commit_evals_batch(self.h, _p(e), _log2_exact(n), batch, _ntt_flags(bitrev=bitrev), _p(out),
                                           inf.ctypes.data_as(intp)), "kzgx_commit_evals_batch")
        return out, inf.astype(bool)

    def commit_evals_device(self, d_evals, log2n, batch, stride, d_out, d_inf, bitrev=False, stream=None):
        _chk(lib().kzgx_commit_evals_batch_device(self.h, d_evals, log2n, batch, stride, _ntt_flags(bitrev=bitrev),
                                                  d_out, d_inf, stream), "kzgx_commit_evals_batch_device")

    def prove_evals(self, evals, zs, shared: bool = True, bitrev: bool = False):
        """kzgx_prove_evals_batch: evals (n, 4) shared (shared=True) or (batch, n, 4) -> (xy, is_inf, y)."""
        z = as_scalars(zs)
        batch = z.shape[0]
        e = np.ascontiguousarray(evals, dtype=np.uint64)
        n = e.shape[-2]
        out = np.zeros((batch, 2 * self.w64), dtype=np.uint64)
        inf = np.zeros(batch, dtype=np.int32)
        y = np.zeros((batch, 4), dtype=np.uint64)
        _chk(lib().kzgx_prove_evals_batch(self.h, _p(e), _log2_exact(n), 0 if shared else n, _p(z), batch,
                                          _ntt_flags(bitrev=bitrev), _p(out), inf.ctypes.data_as(intp), _p(y)),
             "kzgx_prove_evals_batch")
        return out, inf.astype(bool), y

    def prove_evals_device(self, d_evals, log2n, stride, d_z, batch, d_out, d_inf, d_y=None, bitrev=False,
                           stream=None):
        _chk(lib().kzgx_prove_evals_batch_device(self.h, d_evals, log2n, stride, d_z, batch,
                                                 _ntt_flags(bitrev=bitrev), d_out, d_inf, d_y, stream),
             "kzgx_prove_evals_batch_device")

    # ---- G1 NTT, all-domain openings ----
    def g1_ntt(self, points, inf=None, inverse: bool = False, bitrev: bool = False):
        """kzgx_g1_ntt of one transform ((n, 2 w64) points) or a batch ((batch, n, 2 w64)); inf: optional
        flags of the same leading shape -> (points, is_inf) in the input's shape."""
        x = np.ascontiguousarray(points, dtype=np.uint64)
        shape = x.shape
        if x.ndim == 2:
            x = x.reshape(1, -1, 2 * self.w64)
        batch, n = x.shape[0], x.shape[1]
        f = None if inf is None else np.ascontiguousarray(inf, dtype=np.int32).reshape(batch, n)
        out = np.zeros_like(x)
        oi = np.zeros((batch, n), dtype=np.int32)
        _chk(lib().kzgx_g1_ntt(self.h, _p(x), None if f is None else f.ctypes.data_as(intp), _log2_exact(n), batch,
                               _ntt_flags(inverse, bitrev), _p(out), oi.ctypes.data_as(intp)), "kzgx_g1_ntt")
        return out.reshape(shape), oi.astype(bool).reshape(shape[:-1])

    def g1_ntt_device(self, d_in, d_in_inf, d_out, d_out_inf, log2n, batch, inverse=False, bitrev=False, stream=None):
        """kzgx_g1_ntt_device: device pointers (uint32 flags, d_in_inf may be None), enqueued on stream."""
        _chk(lib().kzgx_g1_ntt_device(self.h, d_in, d_in_inf, d_out, d_out_inf, log2n, batch,
                                      _ntt_flags(inverse, bitrev), stream), "kzgx_g1_ntt_device")

    def prove_all_prepare(self, log2n: int):
        """kzgx_prove_all_prepare: build the all-domain setup of size 2^log2n now."""
        _chk(lib().kzgx_prove_all_prepare(self.h, log2n), "kzgx_prove_all_prepare")

    def prove_all(self, polys, evals: bool = False, bitrev: bool = False, want_y: bool = True):
        """kzgx_prove_all_batch: (n, 4) or (batch, n, 4) coefficients (evals: values on the domain)
        -> (xy (batch, n, 2 w64), is_inf (batch, n), y (batch, n, 4) or None); one polynomial
        drops the batch axis."""
        c = np.ascontiguousarray(polys, dtype=np.uint64)
        single = c.ndim == 2
        if single:
            c = c.reshape(1, -1, 4)
        batch, n = c.shape[0], c.shape[1]
        out = np.zeros((batch, n, 2 * self.w64), dtype=np.uint64)
        inf = np.zeros((batch, n), dtype=np.int32)
        y = np.zeros((batch, n, 4), dtype=np.uint64) if want_y else None
        flags = _ntt_flags(bitrev=bitrev) | (PROVE_ALL_EVALS if evals else 0)
        _chk(lib().kzgx_prove_all_batch(self.h, _p(c), _log2_exact(n), batch, flags, _p(out),
                                        inf.ctypes.data_as(intp), _p(y)), "kzgx_prove_all_batch")
        inf = inf.astype(bool)
        return (out[0], inf[0], None if y is None else y[0]) if single else (out, inf, y)

    def prove_all_device(self, d_in, log2n, batch, stride, d_out, d_inf, d_y=None, evals=False, bitrev=False,
                         stream=None):
        """kzgx_prove_all_batch_device: device pointers, stride in scalars, enqueued on stream."""
        flags = _ntt_flags(bitrev=bitrev) | (PROVE_ALL_EVALS if evals else 0)
        _chk(lib().kzgx_prove_all_batch_device(self.h, d_in, log2n, batch, stride, flags, d_out, d_inf, d_y, stream),
             "kzgx_prove_all_batch_device")

    # ---- coset (cell) openings ----
    def prove_cosets_prepare(self, log2n: int, log2l: int):
        """kzgx_prove_cosets_prepare: build the coset setup of (2^log2n coefficients, 2^log2l points) now."""
        _chk(lib().kzgx_prove_cosets_prepare(self.h, log2n, log2l), "kzgx_prove_cosets_prepare")

    def prove_cosets(self, polys, log2l: int, extended: bool = False, evals: bool = False, bitrev: bool = False,
                     want_y: bool = True):
        """kzgx_prove_cosets_batch: (n, 4) or (batch, n, 4) coefficients (evals: values on the size-n domain)
        -> (xy (batch, R, 2 w64), is_inf (batch, R), y (batch, R, l, 4) or None), R = n / l cosets of
        l = 2^log2l points, 2 n / l with extended; one polynomial drops the batch axis."""
        c = np.ascontiguousarray(polys, dtype=np.uint64)
        single = c.ndim == 2
        if single:
            c = c.reshape(1, -1, 4)
        batch, n = c.shape[0], c.shape[1]
        log2n = _log2_exact(n)
        R = max(1, (n << int(bool(extended))) >> log2l)
        out = np.zeros((batch, R, 2 * self.w64), dtype=np.uint64)
        inf = np.zeros((batch, R), dtype=np.int32)
        y = np.zeros((batch, R, 1 << log2l, 4), dtype=np.uint64) if want_y else None
        flags = _cosets_flags(extended, evals, bitrev)
        _chk(lib().kzgx_prove_cosets_batch(self.h, _p(c), log2n, log2l, batch, flags, _p(out),
                                           inf.ctypes.data_as(intp), _p(y)), "kzgx_prove_cosets_batch")
        inf = inf.astype(bool)
        return (out[0], inf[0], None if y is None else y[0]) if single else (out, inf, y)

    def prove_cosets_device(self, d_in, log2n, log2l, batch, stride, d_out, d_inf, d_y=None, extended=False,
                            evals=False, bitrev=False, stream=None):
        """kzgx_prove_cosets_batch_device: device pointers, stride in scalars, enqueued on stream."""
        _chk(lib().kzgx_prove_cosets_batch_device(self.h, d_in, log2n, log2l, batch, stride,
                                                  _cosets_flags(extended, evals, bitrev), d_out, d_inf, d_y, stream),
             "kzgx_prove_cosets_batch_device")

    # ---- aggregated cell verification ----
    def _cells_marshal(self, commits, commit_index, cell_index, proofs, ys, commit_inf, proof_inf):
        """the cell entries' arrays: (leading ABI arguments up to ys, count, log2l, the arrays kept alive)"""
        c = np.ascontiguousarray(commits, dtype=np.uint64).reshape(-1, 2 * self.w64)
        p = np.ascontiguousarray(proofs, dtype=np.uint64).reshape(-1, 2 * self.w64)
        y = np.ascontiguousarray(ys, dtype=np.uint64)
        assert y.ndim >= 2 and y.shape[-1] == 4
        log2l = _log2_exact(y.shape[-2])
        y = y.reshape(-1, y.shape[-2], 4)
        nc, n = c.shape[0], p.shape[0]
        ci = np.ascontiguousarray(commit_index, dtype=np.uint32).reshape(-1)
        ki = np.ascontiguousarray(cell_index, dtype=np.uint32).reshape(-1)
        assert y.shape[0] == n and ci.shape[0] == n and ki.shape[0] == n
        fc = None if commit_inf is None else np.ascontiguousarray(commit_inf, dtype=np.int32)
        fp = None if proof_inf is None else np.ascontiguousarray(proof_inf, dtype=np.int32)
        assert (fc is None or fc.shape[0] == nc) and (fp is None or fp.shape[0] == n)
        head = (self.h, _p(c) if nc else None, None if fc is None else fc.ctypes.data_as(intp), nc,
                ci.ctypes.data_as(u32p) if n else None, ki.ctypes.data_as(u32p) if n else None,
                _p(p) if n else None, None if fp is None else fp.ctypes.data_as(intp), _p(y) if n else None)
        return head, n, log2l, (c, p, y, ci, ki, fc, fp)

    def _cells_host(self, fn, name, commits, commit_index, cell_index, proofs, ys, log2n, challenges, commit_inf,
                    proof_inf, extended, bitrev, extra):
        head, n, log2l, _keep = self._cells_marshal(commits, commit_index, cell_index, proofs, ys, commit_inf,
                                                    proof_inf)
        r = None if challenges is None or not n else as_scalars(challenges)
        assert r is None or r.shape[0] == n
        ok = ctypes.c_int(0)
        _chk(fn(*head, None if r is None else _p(r), n, log2n, log2l, _cosets_flags(extended, bitrev=bitrev), *extra,
                ctypes.byref(ok)), name)
        return bool(ok.value)

    def _cells_each_host(self, fn, name, commits, commit_index, cell_index, proofs, ys, log2n, commit_inf, proof_inf,
                         extended, bitrev, extra):
        head, n, log2l, _keep = self._cells_marshal(commits, commit_index, cell_index, proofs, ys, commit_inf,
                                                    proof_inf)
        ok = np.zeros(n, dtype=np.int32)
        _chk(fn(*head, n, log2n, log2l, _cosets_flags(extended, bitrev=bitrev), *extra,
                ok.ctypes.data_as(intp) if n else None), name)
        return ok.astype(bool)

    def verify_cells_aggregate(self, commits, commit_index, cell_index, proofs, ys, log2n, challenges=None,
                               commit_inf=None, proof_inf=None, extended=False, bitrev=False) -> bool:
        """kzgx_verify_cells_aggregate: one pairing check of count coset openings.  commits (n_commits, 2 w64),
        commit_index / cell_index (count,), proofs (count, 2 w64), ys (count, l, 4) with l = 2^log2l taken from
        the shape; bitrev: cell_index is the chunk of the bit-reversed evaluation array and ys is in its order
        (prove_cosets(..., bitrev=True) output as it comes); challenges None = library-drawn (r_0 = 1)."""
        return self._cells_host(lib().kzgx_verify_cells_aggregate, "kzgx_verify_cells_aggregate", commits,
                                commit_index, cell_index, proofs, ys, log2n, challenges, commit_inf, proof_inf,
                                extended, bitrev, ())

    def verify_cells_aggregate_checked(self, commits, commit_index, cell_index, proofs, ys, log2n, challenges=None,
                                       commit_inf=None, proof_inf=None, extended=False, bitrev=False,
                                       subgroup: bool = False) -> bool:
        """verify_cells_aggregate behind the G1 check of every commit and proof (False if one fails)."""
        return self._cells_host(lib().kzgx_verify_cells_aggregate_checked, "kzgx_verify_cells_aggregate_checked",
                                commits, commit_index, cell_index, proofs, ys, log2n, challenges, commit_inf,
                                proof_inf, extended, bitrev, (int(bool(subgroup)),))

    def verify_cells_aggregate_device(self, d_commits, d_commit_inf, n_commits, d_commit_index, d_cell_index,
                                      d_proofs, d_proof_inf, d_ys, d_challenges, count, log2n, log2l, d_ok,
                                      extended=False, bitrev=False, stream=None):
        """kzgx_verify_cells_aggregate_device: device pointers (uint32 indices and flags), d_ok one uint32,
        enqueued on stream."""
        _chk(lib().kzgx_verify_cells_aggregate_device(
            self.h, d_commits, d_commit_inf, n_commits, d_commit_index, d_cell_index, d_proofs, d_proof_inf, d_ys,
            d_challenges, count, log2n, log2l, _cosets_flags(extended, bitrev=bitrev), d_ok, stream),
            "kzgx_verify_cells_aggregate_device")

    def verify_cells_aggregate_checked_device(self, d_commits, d_commit_inf, n_commits, d_commit_index, d_cell_index,
                                              d_proofs, d_proof_inf, d_ys, d_challenges, count, log2n, log2l,
                                              subgroup, d_ok, extended=False, bitrev=False, stream=None):
        """kzgx_verify_cells_aggregate_checked_device: the same behind the G1 check, still asynchronous."""
        _chk(lib().kzgx_verify_cells_aggregate_checked_device(
            self.h, d_commits, d_commit_inf, n_commits, d_commit_index, d_cell_index, d_proofs, d_proof_inf, d_ys,
            d_challenges, count, log2n, log2l, _cosets_flags(extended, bitrev=bitrev), int(bool(subgroup)), d_ok,
            stream), "kzgx_verify_cells_aggregate_checked_device")

    def verify_cells_each(self, commits, commit_index, cell_index, proofs, ys, log2n, commit_inf=None,
                          proof_inf=None, extended=False, bitrev=False) -> np.ndarray:
        """kzgx_verify_cells_each: verify_cells_aggregate's batch, one boolean per cell (count,) -- the answer
        verify_proof gives for that cell over coset_points(...); no challenges, exact per cell."""
        return self._cells_each_host(lib().kzgx_verify_cells_each, "kzgx_verify_cells_each", commits, commit_index,
                                     cell_index, proofs, ys, log2n, commit_inf, proof_inf, extended, bitrev, ())

    def verify_cells_each_checked(self, commits, commit_index, cell_index, proofs, ys, log2n, commit_inf=None,
                                  proof_inf=None, extended=False, bitrev=False, subgroup: bool = False) -> np.ndarray:
        """verify_cells_each behind the G1 check: False for a cell whose proof or commitment fails it."""
        return self._cells_each_host(lib().kzgx_verify_cells_each_checked, "kzgx_verify_cells_each_checked", commits,
                                     commit_index, cell_index, proofs, ys, log2n, commit_inf, proof_inf, extended,
                                     bitrev, (int(bool(subgroup)),))

    def verify_cells_each_device(self, d_commits, d_commit_inf, n_commits, d_commit_index, d_cell_index, d_proofs,
                                 d_proof_inf, d_ys, count, log2n, log2l, d_ok, extended=False, bitrev=False,
                                 stream=None):
        """kzgx_verify_cells_each_device: device pointers (uint32 indices and flags), d_ok count uint32,
        enqueued on stream."""
        _chk(lib().kzgx_verify_cells_each_device(
            self.h, d_commits, d_commit_inf, n_commits, d_commit_index, d_cell_index, d_proofs, d_proof_inf, d_ys,
            count, log2n, log2l, _cosets_flags(extended, bitrev=bitrev), d_ok, stream),
            "kzgx_verify_cells_each_device")

    def verify_cells_each_checked_device(self, d_commits, d_commit_inf, n_commits, d_commit_index, d_cell_index,
                                         d_proofs, d_proof_inf, d_ys, count, log2n, log2l, subgroup, d_ok,
                                         extended=False, bitrev=False, stream=None):
        """kzgx_verify_cells_each_checked_device: the same behind the G1 check, still asynchronous."""
        _chk(lib().kzgx_verify_cells_each_checked_device(
            self.h, d_commits, d_commit_inf, n_commits, d_commit_index, d_cell_index, d_proofs, d_proof_inf, d_ys,
            count, log2n, log2l, _cosets_flags(extended, bitrev=bitrev), int(bool(subgroup)), d_ok, stream),
            "kzgx_verify_cells_each_checked_device")

    def set_verify_cells_chunk(self, cells: int) -> None:
        """cells per internal chunk of verify_cells_each (0 = the default; at most 65535)"""
        _chk(lib().kzgx_set_verify_cells_chunk(self.h, cells), "kzgx_set_verify_cells_chunk")

    # ---- compressed points ----
    def _records(self, data, rb) -> np.ndarray:
        b = np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else \
            np.ascontiguousarray(data, dtype=np.uint8)
        b = np.ascontiguousarray(b).reshape(-1)
        assert rb and b.shape[0] % rb == 0
        return b

    def _decompress(self, fn, name, group, data, encoding, extra):
        rb = point_bytes(self.curve, group, encoding)
        if rb == 0:  # not offered: the library's own status
            _chk(fn(self.h, None, 0, *extra, None, None, None), name)
        b = self._records(data, rb)
        n = b.shape[0] // rb
        out = np.zeros((n, 2 * group * self.w64), dtype=np.uint64)
        inf = np.zeros(n, dtype=np.int32)
        ok = np.zeros(n, dtype=np.int32)
        _chk(fn(self.h, b.ctypes.data_as(u8p) if n else None, n, *extra, _p(out), inf.ctypes.data_as(intp),
                ok.ctypes.data_as(intp)), name)
        return out, inf.astype(bool), ok.astype(bool)

    def g1_decompress(self, data, encoding=ENC_ZCASH, subgroup: bool = False):
        """kzgx_g1_decompress_batch: packed records -> (points (n, 2 w64), is_inf (n,), ok (n,)); a record that
        does not decode gives all-zero limbs, is_inf and not ok."""
        return self._decompress(lib().kzgx_g1_decompress_batch, "kzgx_g1_decompress_batch", 1, data, encoding,
                                (encoding, int(bool(subgroup))))

    def g2_decompress(self, data, subgroup: bool = False):
        """kzgx_g2_decompress_batch (ZCash encoding): packed 96-byte records -> (points (n, 4 w64), is_inf, ok)."""
        return self._decompress(lib().kzgx_g2_decompress_batch, "kzgx_g2_decompress_batch", 2, data, ENC_ZCASH,
                                (int(bool(subgroup)),))

    def g1_decompress_device(self, d_bytes, count, encoding, subgroup, d_out_xy, d_out_inf, d_ok, d_all_ok,
                             stream=None):
        """kzgx_g1_decompress_batch_device: device pointers (flags uint32; d_out_inf, and one of d_ok / d_all_ok,
        may be None), enqueued on stream."""
        _chk(lib().kzgx_g1_decompress_batch_device(self.h, d_bytes, count, encoding, int(bool(subgroup)), d_out_xy,
                                                   d_out_inf, d_ok, d_all_ok, stream),
             "kzgx_g1_decompress_batch_device")

    def _compress(self, fn, name, group, pts, inf, encoding, extra):
        rb = point_bytes(self.curve, group, encoding)
        if rb == 0:  # not offered: the library's own status
            _chk(fn(self.h, None, None, 0, *extra, None), name)
        xy = np.ascontiguousarray(pts, dtype=np.uint64).reshape(-1, 2 * group * self.w64)
        n = xy.shape[0]
        f = None if inf is None else np.ascontiguousarray(inf, dtype=np.int32)
        assert f is None or f.shape[0] == n
        out = np.zeros(n * rb, dtype=np.uint8)
        _chk(fn(self.h, _p(xy) if n else None, None if f is None else f.ctypes.data_as(intp), n, *extra,
                out.ctypes.data_as(u8p)), name)
        return out.tobytes()

    def g1_compress(self, pts, inf=None, encoding=ENC_ZCASH) -> bytes:
        """kzgx_g1_compress_batch: canonical limbs (+ infinity flags) -> packed records; validates nothing."""
        return self._compress(lib().kzgx_g1_compress_batch, "kzgx_g1_compress_batch", 1, pts, inf, encoding,
                              (encoding,))

    def g2_compress(self, pts, inf=None) -> bytes:
        """kzgx_g2_compress_batch (ZCash encoding)."""
        return self._compress(lib().kzgx_g2_compress_batch, "kzgx_g2_compress_batch", 2, pts, inf, ENC_ZCASH, ())

    def g1_compress_device(self, d_xy, d_inf, count, encoding, d_out, stream=None):
        """kzgx_g1_compress_batch_device: device pointers, enqueued on stream."""
        _chk(lib().kzgx_g1_compress_batch_device(self.h, d_xy, d_inf, count, encoding, d_out, stream),
             "kzgx_g1_compress_batch_device")

    def verify_cells_aggregate_bytes(self, commits, commit_index, cell_index, proofs, ys, log2n, challenges=None,
                                     encoding=ENC_ZCASH, extended=False, bitrev=False, subgroup: bool = False) -> bool:
        """kzgx_verify_cells_aggregate_bytes: verify_cells_aggregate_checked on packed compressed commitments
        and proofs (bytes or uint8 arrays); a record that does not decode gives False."""
        rb = point_bytes(self.curve, 1, encoding)
        if rb == 0:  # not offered: the library's own status
            _chk(lib().kzgx_verify_cells_aggregate_bytes(self.h, None, 0, None, None, None, None, None, 0, log2n, 0,
                                                         0, encoding, 0, None), "kzgx_verify_cells_aggregate_bytes")
        c, p = self._records(commits, rb), self._records(proofs, rb)
        nc, n = c.shape[0] // rb, p.shape[0] // rb
        y = np.ascontiguousarray(ys, dtype=np.uint64)
        assert y.ndim >= 2 and y.shape[-1] == 4
        log2l = _log2_exact(y.shape[-2])
        y = y.reshape(-1, y.shape[-2], 4)
        ci = np.ascontiguousarray(commit_index, dtype=np.uint32).reshape(-1)
        ki = np.ascontiguousarray(cell_index, dtype=np.uint32).reshape(-1)
        r = None if challenges is None or not n else as_scalars(challenges)
        assert y.shape[0] == n and ci.shape[0] == n and ki.shape[0] == n and (r is None or r.shape[0] == n)
        ok = ctypes.c_int(0)
        _chk(lib().kzgx_verify_cells_aggregate_bytes(
            self.h, c.ctypes.data_as(u8p) if nc else None, nc, ci.ctypes.data_as(u32p) if n else None,
            ki.ctypes.data_as(u32p) if n else None, p.ctypes.data_as(u8p) if n else None, _p(y) if n else None,
            None if r is None else _p(r), n, log2n, log2l, _cosets_flags(extended, bitrev=bitrev), encoding,
            int(bool(subgroup)), ctypes.byref(ok)), "kzgx_verify_cells_aggregate_bytes")
        return bool(ok.value)

    def verify_cells_aggregate_bytes_device(self, d_commits, n_commits, d_commit_index, d_cell_index, d_proofs, d_ys,
                                            d_challenges, count, log2n, log2l, encoding, subgroup, d_ok,
                                            extended=False, bitrev=False, stream=None):
        """kzgx_verify_cells_aggregate_bytes_device: the same with device pointers, still asynchronous."""
        _chk(lib().kzgx_verify_cells_aggregate_bytes_device(
            self.h, d_commits, n_commits, d_commit_index, d_cell_index, d_proofs, d_ys, d_challenges, count, log2n,
            log2l, _cosets_flags(extended, bitrev=bitrev), encoding, int(bool(subgroup)), d_ok, stream),
            "kzgx_verify_cells_aggregate_bytes_device")

    # ---- cell recovery ----
    def _recover_host(self, proofs, blob_index, cell_index, ys, n_blobs, log2n, extended, bitrev, want_y,
                      want_coeffs):
        y = np.ascontiguousarray(ys, dtype=np.uint64)
        assert y.ndim >= 2 and y.shape[-1] == 4
        l = y.shape[-2]
        log2l = _log2_exact(l)
        y = y.reshape(-1, l, 4)
        cnt = y.shape[0]
        bi = np.ascontiguousarray(blob_index, dtype=np.uint32).reshape(-1)
        ki = np.ascontiguousarray(cell_index, dtype=np.uint32).reshape(-1)
        assert bi.shape[0] == cnt and ki.shape[0] == cnt
        n = 1 << log2n
        R = max(1, (2 * n) >> log2l)
        oy = np.zeros((n_blobs, R, l, 4), dtype=np.uint64) if want_y else None
        oc = np.zeros((n_blobs, n, 4), dtype=np.uint64) if want_coeffs else None
        ok = np.zeros(n_blobs, dtype=np.int32)
        head = (self.h, bi.ctypes.data_as(u32p) if cnt else None, ki.ctypes.data_as(u32p) if cnt else None,
                _p(y) if cnt else None, cnt, n_blobs, log2n, log2l, _cosets_flags(extended, bitrev=bitrev), _p(oy),
                _p(oc))
        if not proofs:
            _chk(lib().kzgx_recover_cells(*head, ok.ctypes.data_as(intp)), "kzgx_recover_cells")
            return oy, oc, ok.astype(bool)
        xy = np.zeros((n_blobs, R, 2 * self.w64), dtype=np.uint64)
        inf = np.zeros((n_blobs, R), dtype=np.int32)
        _chk(lib().kzgx_recover_cells_and_proofs(*head, _p(xy), inf.ctypes.data_as(intp), ok.ctypes.data_as(intp)),
             "kzgx_recover_cells_and_proofs")
        return oy, oc, xy, inf.astype(bool), ok.astype(bool)

    def recover_cells(self, blob_index, cell_index, ys, n_blobs, log2n, extended=True, bitrev=False, want_y=True,
                      want_coeffs=True):
        """kzgx_recover_cells: rebuild n_blobs polynomials of 2^log2n coefficients from at least half of the
        R = 2^(log2n + 1) / l cells of each.  blob_index / cell_index (count,), ys (count, l, 4) with l taken from
        the shape, a flat list as verify_cells_aggregate takes it (bitrev: cell_index is the chunk of the
        bit-reversed evaluation array and ys is in its order) -> (y (n_blobs, R, l, 4) in prove_cosets' layout or
        None, coeffs (n_blobs, n, 4) or None, ok (n_blobs,) bool).  A blob with ok False is all zero."""
        return self._recover_host(False, blob_index, cell_index, ys, n_blobs, log2n, extended, bitrev, want_y,
                                  want_coeffs)

    def recover_cells_and_proofs(self, blob_index, cell_index, ys, n_blobs, log2n, extended=True, bitrev=False,
                                 want_y=True, want_coeffs=True):
        """kzgx_recover_cells_and_proofs: recover_cells plus every cell's proof, prove_cosets' (xy, is_inf) of the
        recovered polynomials -> (y, coeffs, xy (n_blobs, R, 2 w64), is_inf (n_blobs, R), ok)."""
        return self._recover_host(True, blob_index, cell_index, ys, n_blobs, log2n, extended, bitrev, want_y,
                                  want_coeffs)

    def recover_cells_device(self, d_blob_index, d_cell_index, d_ys, count, n_blobs, log2n, log2l, d_out_y,
                             d_out_coeffs, d_ok, extended=True, bitrev=False, stream=None):
        """kzgx_recover_cells_device: device pointers (uint32 indices, d_ok n_blobs uint32), enqueued on stream."""
        _chk(lib().kzgx_recover_cells_device(self.h, d_blob_index, d_cell_index, d_ys, count, n_blobs, log2n, log2l,
                                             _cosets_flags(extended, bitrev=bitrev), d_out_y, d_out_coeffs, d_ok,
                                             stream), "kzgx_recover_cells_device")

    def recover_cells_and_proofs_device(self, d_blob_index, d_cell_index, d_ys, count, n_blobs, log2n, log2l,
                                        d_out_y, d_out_coeffs, d_out_xy, d_out_inf, d_ok, extended=True,
                                        bitrev=False, stream=None):
        """kzgx_recover_cells_and_proofs_device: the same with the n_blobs x R proofs and their uint32 flags."""
        _chk(lib().kzgx_recover_cells_and_proofs_device(
            self.h, d_blob_index, d_cell_index, d_ys, count, n_blobs, log2n, log2l,
            _cosets_flags(extended, bitrev=bitrev), d_out_y, d_out_coeffs, d_out_xy, d_out_inf, d_ok, stream),
            "kzgx_recover_cells_and_proofs_device")

    # ---- blob proofs ----
    def blob_challenges(self, blobs, log2n, records, bitrev: bool = False):
        """kzgx_blob_challenges: count blobs (bytes / uint8: 32-byte big-endian elements; else uint64 limbs) and
        count 48-byte commitment records -> (z (count, 4) uint64, ok (count,) bool); bitrev is accepted and changes
        nothing (the order hashed is the order given)"""
        a, bm, cnt = _blob_array(blobs, log2n)
        rec = _records48(records)
        assert rec.shape[0] == 48 * cnt
        z = np.zeros((cnt, 4), dtype=np.uint64)
        ok = np.zeros(cnt, dtype=np.int32)
        _chk(lib().kzgx_blob_challenges(self.h, a.ctypes.data if cnt else None, log2n, cnt, _blob_flags(bm, bitrev),
                                        rec.ctypes.data_as(u8p) if cnt else None, _p(z), ok.ctypes.data_as(intp)),
             "kzgx_blob_challenges")
        return z, ok.astype(bool)

    def blob_challenges_device(self, d_blobs, log2n, count, d_records, d_z, d_ok, bytes_mode=False, bitrev=False,
                               stream=None):
        """kzgx_blob_challenges_device: device pointers (d_ok count uint32 or None), enqueued on stream."""
        _chk(lib().kzgx_blob_challenges_device(self.h, d_blobs, log2n, count, _blob_flags(bytes_mode, bitrev),
                                               d_records, d_z, d_ok, stream), "kzgx_blob_challenges_device")

    def evals_at(self, evals, log2n, zs, shared: bool = False, bitrev: bool = False) -> np.ndarray:
        """kzgx_evals_at_batch: y_k = P_k(z_k) for polynomials given by their 2^log2n evaluations (bytes / uint8 or
        limbs as blob_challenges; shared: one polynomial for every z) -> (count, 4) uint64"""
        a, bm, cnt = _blob_array(evals, log2n)
        z = as_scalars(zs)
        m = z.shape[0]
        assert cnt == (1 if shared else m) or m == 0
        y = np.zeros((m, 4), dtype=np.uint64)
        _chk(lib().kzgx_evals_at_batch(self.h, a.ctypes.data if a.size else None, log2n, 0 if shared else 1 << log2n,
                                       _p(z) if m else None, m, _blob_flags(bm, bitrev), _p(y)),
             "kzgx_evals_at_batch")
        return y

    def evals_at_device(self, d_evals, log2n, stride, d_z, count, d_y, bytes_mode=False, bitrev=False, stream=None):
        """kzgx_evals_at_batch_device: device pointers, stride in elements (0: shared), enqueued on stream."""
        _chk(lib().kzgx_evals_at_batch_device(self.h, d_evals, log2n, stride, d_z, count,
                                              _blob_flags(bytes_mode, bitrev), d_y, stream),
             "kzgx_evals_at_batch_device")

    def prove_blobs(self, blobs, log2n, bitrev: bool = False):
        """kzgx_prove_blobs_batch: -> (commitment records, proof records (bytes, 48 per blob), z, y (count, 4));
        an invalid blob raises KzgxError(KZGX_ERR_ARG)"""
        a, bm, cnt = _blob_array(blobs, log2n)
        c = np.zeros(48 * cnt, dtype=np.uint8)
        p = np.zeros(48 * cnt, dtype=np.uint8)
        z = np.zeros((cnt, 4), dtype=np.uint64)
        y = np.zeros((cnt, 4), dtype=np.uint64)
        _chk(lib().kzgx_prove_blobs_batch(self.h, a.ctypes.data if cnt else None, log2n, cnt, _blob_flags(bm, bitrev),
                                          c.ctypes.data_as(u8p), p.ctypes.data_as(u8p), _p(z), _p(y)),
             "kzgx_prove_blobs_batch")
        return c.tobytes(), p.tobytes(), z, y

    def prove_blobs_device(self, d_blobs, log2n, count, d_commits, d_proofs, d_z, d_y, d_ok, bytes_mode=False,
                           bitrev=False, stream=None):
        """kzgx_prove_blobs_batch_device: device pointers (d_z, d_y, d_ok may be None), enqueued on stream."""
        _chk(lib().kzgx_prove_blobs_batch_device(self.h, d_blobs, log2n, count, _blob_flags(bytes_mode, bitrev),
                                                 d_commits, d_proofs, d_z, d_y, d_ok, stream),
             "kzgx_prove_blobs_batch_device")

    def _verify_blobs_marshal(self, blobs, log2n, commits, proofs):
        a, bm, cnt = _blob_array(blobs, log2n)
        c, p = _records48(commits), _records48(proofs)
        assert c.shape[0] == 48 * cnt and p.shape[0] == 48 * cnt
        return a, bm, cnt, c, p

    def verify_blobs(self, blobs, log2n, commits, proofs, challenges=None, bitrev: bool = False,
                     subgroup: bool = False) -> bool:
        """kzgx_verify_blobs_batch: one answer for count (blob, commitment record, proof record) triples;
        challenges (count, 4) or None (library-drawn)"""
        a, bm, cnt, c, p = self._verify_blobs_marshal(blobs, log2n, commits, proofs)
        r = None if challenges is None or not cnt else as_scalars(challenges)
        assert r is None or r.shape[0] == cnt
        ok = ctypes.c_int(0)
        _chk(lib().kzgx_verify_blobs_batch(self.h, a.ctypes.data if cnt else None, log2n, cnt, _blob_flags(bm, bitrev),
                                           c.ctypes.data_as(u8p) if cnt else None,
                                           p.ctypes.data_as(u8p) if cnt else None, None if r is None else _p(r),
                                           int(bool(subgroup)), ctypes.byref(ok)), "kzgx_verify_blobs_batch")
        return bool(ok.value)

    def verify_blobs_each(self, blobs, log2n, commits, proofs, bitrev: bool = False,
                          subgroup: bool = False) -> np.ndarray:
        """kzgx_verify_blobs_each: one verdict per blob -> (count,) bool"""
        a, bm, cnt, c, p = self._verify_blobs_marshal(blobs, log2n, commits, proofs)
        ok = np.zeros(max(cnt, 1), dtype=np.int32)
        _chk(lib().kzgx_verify_blobs_each(self.h, a.ctypes.data if cnt else None, log2n, cnt, _blob_flags(bm, bitrev),
                                          c.ctypes.data_as(u8p) if cnt else None,
                                          p.ctypes.data_as(u8p) if cnt else None, int(bool(subgroup)),
                                          ok.ctypes.data_as(intp)), "kzgx_verify_blobs_each")
        return ok[:cnt].astype(bool)

    def verify_blobs_device(self, d_blobs, log2n, count, d_commits, d_proofs, d_challenges, subgroup, d_ok,
                            bytes_mode=False, bitrev=False, stream=None):
        """kzgx_verify_blobs_batch_device: device pointers, d_ok one uint32, still asynchronous."""
        _chk(lib().kzgx_verify_blobs_batch_device(self.h, d_blobs, log2n, count, _blob_flags(bytes_mode, bitrev),
                                                  d_commits, d_proofs, d_challenges, int(bool(subgroup)), d_ok,
                                                  stream), "kzgx_verify_blobs_batch_device")

    def verify_blobs_each_device(self, d_blobs, log2n, count, d_commits, d_proofs, subgroup, d_ok, bytes_mode=False,
                                 bitrev=False, stream=None):
        """kzgx_verify_blobs_each_device: device pointers, d_ok count uint32, still asynchronous."""
        _chk(lib().kzgx_verify_blobs_each_device(self.h, d_blobs, log2n, count, _blob_flags(bytes_mode, bitrev),
                                                 d_commits, d_proofs, int(bool(subgroup)), d_ok, stream),
             "kzgx_verify_blobs_each_device")
