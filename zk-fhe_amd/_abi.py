"""The C ABI of include/zkfhe.h as data: the ctypes structures, the constants and ONE table of every function's signature, which
load_library() applies when it opens the library.  Nothing else assigns argtypes or restype; tests/test_capi_exports.py compares
the table with the header's prototypes, parameter by parameter."""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libzkfhe_hip.so")
_lib = None

PROF_G1_DECOMPRESS, PROF_MSM_SEGMENTED = 3, 4   # zkfhe_prof_read slots of the batch verifier's kernels (zkfhe.h)
PROF_BFV_SAMPLE, PROF_RNS_NTT, PROF_RNS_EPILOGUE = 5, 6, 7   # ... and of the BFV encryption kernels
PROF_BFV_TENSOR, PROF_BFV_RELIN, PROF_BFV_EVAL_EPILOGUE, PROF_BFV_ELEMENTWISE = 8, 9, 10, 11   # ... and of the BFV evaluation kernels
PROF_BFV_SHARE_SUM, PROF_BFV_DECRYPT_COMBINE = 12, 13   # ... and of the threshold kernels
PROF_BFV_GALOIS, PROF_BFV_SLOT_NTT = 14, 15   # ... and of the slot and rotation kernels
PROF_BFV_HOIST, PROF_BFV_LINEAR = 16, 17   # ... and of the hoisted rotations and linear transforms
PROF_BFV_BSGS_INNER, PROF_BFV_BSGS_GIANT = 18, 19   # ... and of the baby-step/giant-step transform's own kernels
PROF_BFV_DOT = 20   # ... and of the fused inner product's accumulation
PROF_BFV_PCKS_COMBINE, PROF_BFV_REFRESH_COMBINE = 21, 22   # ... and of the key-switch and refresh combines
PROF_G1_FFT = 23   # ... and of the G1 FFT's butterfly kernels
PROF_BFV_BALLOT = 24   # ... and of the ballot box's unpack and sum kernels
PROF_BFV_RESIDENT = 25   # ... and of the resident batches' check, gather and group-sum kernels
PROF_BFV_KEY_SWITCH_WIDE = 26   # ... and of the digit-parallel key switch of the calls that take a resident key set
PROF_BFV_PACK = 27   # ... and of the ring-packing kernels
# per-item statuses of Context.bfv_sum_instances and BallotBox.add (ZKFHE_BALLOT_* of zkfhe.h)
BALLOT_COUNTED, BALLOT_SKIPPED, BALLOT_BAD_GROUP, BALLOT_NOT_A_CIPHERTEXT, BALLOT_WRONG_KEY, BALLOT_REJECTED, BALLOT_REPEATED = range(7)
BALLOT_STATUSES = 7
BALLOT_STATUS_NAMES = ("counted", "skipped", "bad_group", "not_a_ciphertext", "wrong_key", "rejected", "repeated")
SRS_BAD_POWERS, SRS_BAD_LAGRANGE, SRS_BAD_GENERATOR = 1, 2, 4   # the bits of Srs.check (zkfhe_srs_check)


class ZkfheError(RuntimeError):
    pass


class BfvParamsC(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint64), ("q", ctypes.c_uint64), ("t", ctypes.c_uint64), ("b", ctypes.c_uint64)]


def params_tuple(prm):
    """(n, q, t, b) out of a filled BfvParamsC"""
    return tuple(int(getattr(prm, name)) for name, _ in BfvParamsC._fields_)


class _BfvWordsC(ctypes.Structure):
    _fields_ = [(k, ctypes.POINTER(ctypes.c_uint64)) for k in ("pk0", "pk1", "m", "u", "e0", "e1", "c0", "c1")]


class BfvConfigC(ctypes.Structure):
    _fields_ = [("k", ctypes.c_uint32), ("n_gate0", ctypes.c_uint32), ("n_gate1", ctypes.c_uint32), ("n_lookup", ctypes.c_uint32),
                ("n_rlc", ctypes.c_uint32), ("unusable_rows", ctypes.c_uint32), ("lookup_bits", ctypes.c_uint32),
                ("bp_gate0", ctypes.POINTER(ctypes.c_uint32)), ("n_bp_gate0", ctypes.c_uint32),
                ("bp_gate1", ctypes.POINTER(ctypes.c_uint32)), ("n_bp_gate1", ctypes.c_uint32),
                ("bp_rlc", ctypes.POINTER(ctypes.c_uint32)), ("n_bp_rlc", ctypes.c_uint32),
                ("replay", ctypes.c_int), ("transcript", ctypes.c_uint32)]


ALLGATHER_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p)
_U64P = ctypes.POINTER(ctypes.c_uint64)

# One letter per C type.  A lower-case letter is a value or a plain address, its capital the address of one (or of an array of them).
#   v  void *, any handle (zkfhe_ctx *, zkfhe_srs *, ...) and device memory    V  void **, the address of a handle
#   s  char * / uint8_t *: text, seeds, byte buffers                           S  uint8_t **
#   i  int       I  int *         w  uint32_t   W  uint32_t *     n  size_t   N  size_t *
#   u  uint64_t  p  uint64_t *    l  int64_t    j  int32_t *      f  float *  d  double *
#   B  zkfhe_bfv_params *    C  zkfhe_bfv_config *    X  zkfhe_bfv_words *    a  zkfhe_allgather_fn    -  void (a return type only)
_TYPES = {
    "v": ctypes.c_void_p, "V": ctypes.POINTER(ctypes.c_void_p), "s": ctypes.c_char_p, "S": ctypes.POINTER(ctypes.POINTER(ctypes.c_uint8)),
    "i": ctypes.c_int, "I": ctypes.POINTER(ctypes.c_int), "w": ctypes.c_uint32, "W": ctypes.POINTER(ctypes.c_uint32),
    "n": ctypes.c_size_t, "N": ctypes.POINTER(ctypes.c_size_t), "u": ctypes.c_uint64, "p": _U64P, "l": ctypes.c_int64,
    "j": ctypes.POINTER(ctypes.c_int32), "f": ctypes.POINTER(ctypes.c_float), "d": ctypes.POINTER(ctypes.c_double),
    "B": ctypes.POINTER(BfvParamsC), "C": ctypes.POINTER(BfvConfigC), "X": ctypes.POINTER(_BfvWordsC), "a": ALLGATHER_FN, "-": None,
}

# "return:parameters" of every function of include/zkfhe.h, in the header's order
_ABI = {
    "zkfhe_ctx_create": "i:ivV", "zkfhe_ctx_destroy": "i:v", "zkfhe_last_error": "s:v", "zkfhe_sync": "i:v", "zkfhe_stream": "v:v",
    "zkfhe_device_info": "i:vsnIN", "zkfhe_dev_alloc": "i:vnV", "zkfhe_dev_free": "i:vv", "zkfhe_upload": "i:vvvn", "zkfhe_download": "i:vvvn",
    "zkfhe_copy_dev": "i:vvvn", "zkfhe_memset_dev": "i:vvin", "zkfhe_timer_start": "i:v", "zkfhe_timer_stop_ms": "i:vf", "zkfhe_prof_enable": "i:vi",
    "zkfhe_prof_reset": "i:v", "zkfhe_prof_read": "i:vidpd", "zkfhe_prof_read_ops": "i:vid", "zkfhe_ctx_last_proof_marks": "i:vf",
    "zkfhe_ctx_last_proof_commands": "i:vp", "zkfhe_fr_add": "i:vvvvn", "zkfhe_fr_sub": "i:vvvvn", "zkfhe_fr_mul": "i:vvvvn",
    "zkfhe_fr_scale": "i:vvvvn", "zkfhe_fr_to_mont": "i:vvvn", "zkfhe_fr_from_mont": "i:vvvn", "zkfhe_fr_batch_invert": "i:vvn",
    "zkfhe_fr_batch_invert_mul": "i:vvvn", "zkfhe_fr9_op": "i:vivvn", "zkfhe_fr_sqr_chain": "i:vvvni", "zkfhe_fq29_sqr_chain": "i:vvvni",
    "zkfhe_ntt_batch": "i:vvnii", "zkfhe_ntt_batch_to": "i:vvvnii", "zkfhe_coset_ntt_batch": "i:vvvniivi", "zkfhe_basis_create": "i:vvniV",
    "zkfhe_basis_destroy": "i:vv", "zkfhe_basis_len": "n:v", "zkfhe_msm_batch": "i:vvvnv", "zkfhe_msm_sparse": "i:vvvnnv",
    "zkfhe_msm_batch_xyzz": "i:vvvnv", "zkfhe_msm_sparse_xyzz": "i:vvvnnv", "zkfhe_g1_xyzz_to_affine": "i:vnv", "zkfhe_basis_has_multiples": "i:v",
    "zkfhe_basis_table_bits": "i:vI", "zkfhe_basis_table_bytes": "n:vI", "zkfhe_comm_unique_id": "i:s", "zkfhe_comm_create": "i:viisV",
    "zkfhe_comm_create_with_transport": "i:viiavV", "zkfhe_comm_destroy": "i:vv", "zkfhe_comm_rank": "i:v", "zkfhe_comm_world": "i:v",
    "zkfhe_comm_active": "i:v", "zkfhe_comm_point_range": "-:vnNN", "zkfhe_comm_all_gather": "i:vvvvn", "zkfhe_comm_all_gather_async": "i:vvvvn",
    "zkfhe_msm_batch_sharded": "i:vvvvnnv", "zkfhe_msm_batch_sharded_async": "i:vvvvnnv", "zkfhe_comm_join": "i:vvi",
    "zkfhe_comm_record_event": "i:vvv", "zkfhe_g1_add": "i:vvvvn", "zkfhe_g1_mul": "i:vvvvn", "zkfhe_g1_fft": "i:vvii",
    "zkfhe_g1_decompress": "i:vvnvv", "zkfhe_msm_segmented": "i:vvnvvnvnv", "zkfhe_witness_poly_mul_u64": "i:vvvnv",
    "zkfhe_host_poly_mul_u32": "i:ppnpp", "zkfhe_witness_div_mod": "i:vvuvvn", "zkfhe_transcript_create": "i:wV", "zkfhe_transcript_destroy": "-:v",
    "zkfhe_transcript_common_scalar": "i:vs", "zkfhe_transcript_write_scalar": "i:vs", "zkfhe_transcript_common_point": "i:vs",
    "zkfhe_transcript_write_point": "i:vs", "zkfhe_transcript_squeeze": "i:vs", "zkfhe_transcript_bytes": "i:vsnN", "zkfhe_poseidon_permute": "i:s",
    "zkfhe_poseidon_constants": "i:ss", "zkfhe_host_hash_mode": "i:i", "zkfhe_poseidon_hash_many": "i:sNnis", "zkfhe_bfv_build_tables": "i:sBCsiVsn",
    "zkfhe_bfv_tables_free": "-:v", "zkfhe_bfv_auto_config": "i:sBwwwWsn", "zkfhe_bfv_tables_count": "n:vi", "zkfhe_bfv_tables_copy_advice": "i:vp",
    "zkfhe_bfv_tables_copy_fixed": "i:vp", "zkfhe_bfv_tables_copy_instance": "i:vp", "zkfhe_bfv_tables_copy_copies": "i:vp",
    "zkfhe_bfv_tables_copy_break_points": "i:viW", "zkfhe_prover_gate": "i:i", "zkfhe_bfv_mock_check": "i:vspsn",
    "zkfhe_bfv_tables_poke_advice": "i:vwws", "zkfhe_srs_create": "i:vwsnV", "zkfhe_srs_save": "i:vvs", "zkfhe_srs_drop_host_copy": "i:v",
    "zkfhe_srs_load": "i:vsV", "zkfhe_srs_g2": "i:vss", "zkfhe_srs_set_g2": "i:vss", "zkfhe_srs_file_g2": "i:sWss", "zkfhe_chacha20_block": "i:sWs",
    "zkfhe_srs_from_points": "i:vwvvV", "zkfhe_srs_from_monomial": "i:vwvnssV", "zkfhe_srs_load_downsized": "i:vswV", "zkfhe_srs_check": "i:vvsW",
    "zkfhe_srs_create_sharded": "i:vvwsnV", "zkfhe_srs_destroy": "i:vv", "zkfhe_srs_table_bits": "i:vI", "zkfhe_srs_table_info": "i:vIpI",
    "zkfhe_bfv_keygen": "i:vvsBCV", "zkfhe_bfv_pk_destroy": "i:vv", "zkfhe_bfv_pk_release_ctx": "i:vv", "zkfhe_bfv_pk_info": "i:vsWW",
    "zkfhe_bfv_pk_commitments": "i:vss", "zkfhe_bfv_pk_prefix_cache": "i:vippp", "zkfhe_bfv_pk_prehash": "i:vsppp",
    "zkfhe_bfv_pk_break_points": "i:viWW", "zkfhe_bfv_pk_export_vk": "i:vsnN", "zkfhe_bfv_witness_stream": "i:vvssvnN",
    "zkfhe_lookup_permute": "i:vvnnwvvI", "zkfhe_bfv_pk_save": "i:vvs", "zkfhe_bfv_pk_load": "i:vvsV", "zkfhe_snark_encode": "i:snsnsnN",
    "zkfhe_snark_decode": "i:snsNsN", "zkfhe_bfv_verify": "i:snsnsnsnIsn", "zkfhe_bfv_verify_g2": "i:snsnsnssIsn",
    "zkfhe_bfv_verify_batch": "i:vsnnSNSNsnssIsn", "zkfhe_bfv_prove": "i:vvvsssnNsNf", "zkfhe_bfv_prove_words": "i:vvvXssnNsNf",
    "zkfhe_poly_mul_ternary_negacyclic": "i:vvnvnuuvI", "zkfhe_bfv_error_cdt": "i:BpN", "zkfhe_bfv_fhe_keypair": "i:vBsppp",
    "zkfhe_bfv_encrypt": "i:vBppnpsuppppp", "zkfhe_bfv_decrypt": "i:vBpnppp", "zkfhe_bfv_add": "i:vBnppppipp", "zkfhe_bfv_sum": "i:vBnpppp",
    "zkfhe_bfv_add_plain": "i:vBnppnppp", "zkfhe_bfv_mul_plain": "i:vBnppnppp", "zkfhe_bfv_relin_digits": "i:BiN",
    "zkfhe_bfv_relin_keygen": "i:vBpsipp", "zkfhe_bfv_mul": "i:vBnppppppipp", "zkfhe_bfv_noise": "i:vBpnppp", "zkfhe_bfv_dot_max_terms": "i:BiN",
    "zkfhe_bfv_dot": "i:vBnnppnppppipp", "zkfhe_bfv_dot_plain": "i:vBnnppnppp", "zkfhe_bfv_keygen_share": "i:vBssppp",
    "zkfhe_bfv_share_aggregate": "i:vBnnpp", "zkfhe_bfv_relin_share1": "i:vBpssipp", "zkfhe_bfv_relin_share2": "i:vBpsippp",
    "zkfhe_bfv_decrypt_share": "i:vBpnpsuup", "zkfhe_bfv_decrypt_combine": "i:vBnnppp", "zkfhe_bfv_pcks_share": "i:vBpppnpsuupp",
    "zkfhe_bfv_pcks_combine": "i:vBnnppppp", "zkfhe_bfv_refresh_share": "i:vBpsnpsuupp", "zkfhe_bfv_refresh_combine": "i:vBnnsuppppp",
    "zkfhe_bfv_slot_count": "i:BN", "zkfhe_bfv_galois_element": "i:Blip", "zkfhe_bfv_slot_sum_elements": "i:BpN", "zkfhe_bfv_encode_slots": "i:vBnpp",
    "zkfhe_bfv_decode_slots": "i:vBnpp", "zkfhe_bfv_galois_keygen": "i:vBpsuipp", "zkfhe_bfv_apply_galois": "i:vBnppuppipp",
    "zkfhe_bfv_slot_sum": "i:vBnppppipp", "zkfhe_bfv_galois_share": "i:vBpssuipp", "zkfhe_bfv_apply_galois_many": "i:vBnppnpppipp",
    "zkfhe_bfv_linear_transform": "i:vBnppnpppippp", "zkfhe_bfv_linear_transform_bsgs": "i:vBnppnpppnpppippp", "zkfhe_bfv_plan_create": "i:vBnpppipV",
    "zkfhe_bfv_plan_create_bsgs": "i:vBnpppnpppipV", "zkfhe_bfv_plan_apply": "i:vvnpppp", "zkfhe_bfv_plan_info": "i:vBINp",
    "zkfhe_bfv_plan_bytes": "i:Binnnp", "zkfhe_bfv_plan_destroy": "i:vv", "zkfhe_bfv_instances_unpack": "i:Bsnppppj",
    "zkfhe_bfv_sum_instances": "i:vBnSNjnpppj", "zkfhe_bfv_box_create": "i:vsnBppnsnssV", "zkfhe_bfv_box_add": "i:vvnSNSNjjsn",
    "zkfhe_bfv_box_tally": "i:vvppp", "zkfhe_bfv_box_info": "i:vBNp", "zkfhe_bfv_box_destroy": "i:vv", "zkfhe_bfv_cts_alloc": "i:vBnV",
    "zkfhe_bfv_cts_upload": "i:vBnppV", "zkfhe_bfv_cts_store": "i:vvnnpp", "zkfhe_bfv_cts_download": "i:vvnnpp", "zkfhe_bfv_cts_info": "i:vBNp",
    "zkfhe_bfv_cts_destroy": "i:vv", "zkfhe_bfv_box_tally_cts": "i:vvvp", "zkfhe_bfv_cts_add": "i:vvviv", "zkfhe_bfv_cts_add_plain": "i:vvnpv",
    "zkfhe_bfv_cts_mul_plain": "i:vvnpv", "zkfhe_bfv_cts_mul": "i:vvvppiv", "zkfhe_bfv_cts_apply_galois": "i:vvuppiv",
    "zkfhe_bfv_cts_plan_apply": "i:vvvv", "zkfhe_bfv_cts_select": "i:vvnpv", "zkfhe_bfv_cts_sum": "i:vvjnv", "zkfhe_bfv_evk_create": "i:vBippnpppV",
    "zkfhe_bfv_evk_bytes": "i:Biinp", "zkfhe_bfv_evk_info": "i:vBIINpp", "zkfhe_bfv_evk_destroy": "i:vv", "zkfhe_bfv_evk_wide_max": "i:vBiN",
    "zkfhe_bfv_cts_mul_evk": "i:vvvvv", "zkfhe_bfv_cts_apply_galois_evk": "i:vvuvv", "zkfhe_bfv_cts_slot_sum": "i:vvvv",
    "zkfhe_bfv_cts_dot": "i:vvvnvv", "zkfhe_bfv_cts_dot_plain": "i:vvnnpv", "zkfhe_bfv_hybrid_max_p": "i:Bip",
    "zkfhe_bfv_relin_keygen_hybrid": "i:vBupsipppp", "zkfhe_bfv_galois_share_hybrid": "i:vBupssuipppp",
    "zkfhe_bfv_galois_keygen_hybrid": "i:vBupsuipppp", "zkfhe_bfv_evk_create_hybrid": "i:vBuippppnpppppV",
    "zkfhe_bfv_evk_special_modulus": "i:vp", "zkfhe_bfv_pack_elements": "i:BpN",
    "zkfhe_bfv_mul_monomial": "i:vBnppnppp", "zkfhe_bfv_pack": "i:vBnnpppppipp", "zkfhe_bfv_cts_mul_monomial": "i:vvnpv",
    "zkfhe_bfv_cts_pack": "i:vvnpvv", "zkfhe_version": "s:",
}

SIGNATURES = {name: (_TYPES[sig[0]], [_TYPES[c] for c in sig[2:]]) for name, sig in _ABI.items()}   # name -> (restype, argtypes)
EXPORTS = list(SIGNATURES)


def load_library():
    """dlopen the in-tree HIP extension and type every function of SIGNATURES, once.  Raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ZkfheError("HIP extension %s is missing: run `python zk-fhe_amd/build.py` (or __graft_entry__.build())" % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        f = getattr(lib, name)
        f.restype, f.argtypes = restype, argtypes
    _lib = lib
    return lib
