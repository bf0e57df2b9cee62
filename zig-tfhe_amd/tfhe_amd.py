"""Host-side mirror of zig-tfhe's public surface over the MI355X C ABI.

Names follow the reference (src/gates.zig `Gates.nandGate` ..., src/key.zig
`SecretKey` / `CloudKey`, src/tlwe.zig `TLWELv0`, src/params.zig parameter
sets); every method is a thin call into lib/libtfhe_gpu.so (include/tfhe_gpu.h).
There is no CPU fallback: without the built HIP library every entry point
raises.

Batches of ciphertexts are numpy uint32 arrays of shape (B, n+1) — B
TLWELv0 values laid out exactly as `TLWELv0.p` (tlwe.zig:11-12).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from dataclasses import dataclass

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TFHE_GPU_LIB") or os.path.join(HERE, "lib", "libtfhe_gpu.so")  # env: A/B builds

# tfhe_gpu_set_option keys / values (include/tfhe_gpu.h TFHE_OPT_*, TFHE_TWIDDLES_*)
OPTIONS = {"br_form": 1, "br_loader": 2, "ks_form": 3, "ks_narrow": 4, "ks_item_groups": 5, "ks_sel_items": 6,
           "circuit_pack": 7, "twiddles": 8, "arith": 9, "br_sync": 10, "br_spin_cap": 11, "host_pipeline": 12,
           "circuit_split": 13, "host_staging": 17, "cmux_form": 18, "pack_scratch_mb": 19,
           "scatter_scratch_mb": 20, "graph_chunk_queries": 21}
READONLY_OPTIONS = {"fused_admitted": 14, "level_issue_us": 15, "key_row_rms_ppm": 16}  # tfhe_gpu_get_option only
OPTION_DEFAULTS = {"br_form": 0, "br_loader": 1, "ks_form": 3, "ks_narrow": 0, "ks_item_groups": 0,
                   "ks_sel_items": 8, "circuit_pack": 1, "twiddles": 0, "arith": 0, "br_sync": 1, "br_spin_cap": 0,
                   "host_pipeline": 0, "circuit_split": 0, "host_staging": 0, "cmux_form": 0,
                   "pack_scratch_mb": 256, "scatter_scratch_mb": 256, "graph_chunk_queries": 0}
# status codes (include/tfhe_gpu.h TFHE_ERR_*)
ERR_INVALID, ERR_HIP, ERR_NO_KEY, ERR_OOM, ERR_IO, ERR_DEVICE = -1, -2, -3, -4, -5, -6
# 2 split, 4 pair: removed (round 4); 6 duo, 7 wide2: A/B libraries only (tools/ab/, round 5); 5 octo: L = 1
BR_FORMS = {"auto": 0, "whole": 1, "wide": 3, "octo": 5, "duo": 6, "wide2": 7, "plain": 8}
BUILD_PRODUCT, BUILD_AB = 0, 1  # tfhe_gpu_build_kind
TWIDDLES_GLIBC, TWIDDLES_FDLIBM = 0, 1
ARITH_AUTO, ARITH_REFERENCE, ARITH_FUSED_FORCED = 0, 1, 2
STAGING_PAGEABLE, STAGING_PINNED = 0, 1  # TFHE_OPT_HOST_STAGING
CMUX_AUTO, CMUX_PER_WAVE, CMUX_SHARED = 0, 1, 2  # TFHE_OPT_CMUX_FORM

# gate op codes, include/tfhe_gpu.h TFHE_GATE_* (gates.zig:48-121)
NAND, OR, AND, XOR, XNOR, NOR, ANDNY, ANDYN, ORNY, ORYN = range(10)
NOT = 254  # circuits only: negation, no bootstrap
COPY = 255
GATE_NAMES = {"nand": NAND, "or": OR, "and": AND, "xor": XOR, "xnor": XNOR, "nor": NOR,
              "andny": ANDNY, "andyn": ANDYN, "orny": ORNY, "oryn": ORYN}


class TfheParams(C.Structure):
    _fields_ = [("n", C.c_uint32), ("N", C.c_uint32), ("nbit", C.c_uint32), ("L", C.c_uint32),
                ("bgbit", C.c_uint32), ("basebit", C.c_uint32), ("iks_t", C.c_uint32),
                ("_pad", C.c_uint32), ("alpha_lv0", C.c_double), ("alpha_lv1", C.c_double),
                ("alpha_ksk", C.c_double), ("alpha_bsk", C.c_double)]

    def __repr__(self):
        return (f"TfheParams(n={self.n}, N={self.N}, L={self.L}, bgbit={self.bgbit}, "
                f"basebit={self.basebit}, iks_t={self.iks_t})")


class PackedPlan(C.Structure):
    """tfhe_packed_plan: the shape of a packed lookup (tfhe_packed_lookup_plan)."""
    _fields_ = [("stride", C.c_uint32), ("slots", C.c_uint32), ("h", C.c_uint32), ("v", C.c_uint32),
                ("trlwes", C.c_uint32), ("cmuxes", C.c_uint32), ("rot", C.c_uint32 * 10)]

    def __repr__(self):
        return (f"PackedPlan(stride={self.stride}, slots={self.slots}, h={self.h}, v={self.v}, "
                f"trlwes={self.trlwes}, cmuxes={self.cmuxes})")


# params.zig parameter sets (runtime form).  KSK/BSK noise: the reference's
# KSK_ALPHA/BSK_ALPHA (params.zig:419-422) are the 128-bit constants; UINT4
# keeps its own set's alphas.
SECURITY_128_BIT = dict(n=700, N=1024, nbit=10, L=3, bgbit=6, basebit=2, iks_t=9,
                        alpha_lv0=2.0e-5, alpha_lv1=2.0e-8, alpha_ksk=2.0e-5, alpha_bsk=2.0e-8)
SECURITY_80_BIT = dict(n=550, N=1024, nbit=10, L=3, bgbit=6, basebit=2, iks_t=7,
                       alpha_lv0=5.0e-5, alpha_lv1=3.73e-8, alpha_ksk=2.0e-5, alpha_bsk=2.0e-8)
SECURITY_UINT4 = dict(n=820, N=1024, nbit=10, L=1, bgbit=22, basebit=5, iks_t=3,
                      alpha_lv0=0.00000251676160959795544987084234,
                      alpha_lv1=0.00000000000000022204460492503131,
                      alpha_ksk=0.00000251676160959795544987084234,
                      # 2^-52 is below the 32-bit torus resolution; the reference's
                      # f64ToTorus would turn it into a {0,-1} bias that the
                      # L=1/Bg=2^22 gadget amplifies 2^21x
                      alpha_bsk=0.0)
SECURITY_110_BIT = dict(n=630, N=1024, nbit=10, L=3, bgbit=6, basebit=2, iks_t=8,
                        alpha_lv0=3.0517578125e-05, alpha_lv1=2.9802322387695313e-8,
                        alpha_ksk=2.0e-5, alpha_bsk=2.0e-8)
SECURITY_UINT1 = dict(n=700, N=1024, nbit=10, L=2, bgbit=10, basebit=2, iks_t=8,
                      alpha_lv0=2.0e-5, alpha_lv1=2.0e-8, alpha_ksk=2.0e-5, alpha_bsk=2.0e-8)
# UINT2 / UINT3 follow UINT4: the set's lv0 alpha for the KSK, a zero BSK noise
SECURITY_UINT2 = dict(n=687, N=1024, nbit=10, L=1, bgbit=18, basebit=4, iks_t=3,
                      alpha_lv0=0.00002120846893069971872305794214,
                      alpha_lv1=0.00000000000231841227527049948463,
                      alpha_ksk=0.00002120846893069971872305794214,
                      alpha_bsk=0.0)
SECURITY_UINT3 = dict(n=820, N=1024, nbit=10, L=1, bgbit=23, basebit=6, iks_t=2,
                      alpha_lv0=0.00000251676160959795544987084234,
                      alpha_lv1=0.00000000000000022204460492503131,
                      alpha_ksk=0.00000251676160959795544987084234,
                      alpha_bsk=0.0)
PARAM_SETS = {"128": SECURITY_128_BIT, "80": SECURITY_80_BIT, "uint4": SECURITY_UINT4,
              "110": SECURITY_110_BIT, "uint1": SECURITY_UINT1, "uint2": SECURITY_UINT2, "uint3": SECURITY_UINT3}


def make_params(name_or_dict="128") -> TfheParams:
    d = PARAM_SETS[name_or_dict] if isinstance(name_or_dict, str) else name_or_dict
    return TfheParams(**d)


_lib = None
u32p, f64p, u8p, vp = C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(C.c_uint8), C.c_void_p
i32p = C.POINTER(C.c_int32)

_SIGS = {
    "tfhe_gpu_abi_version": (C.c_int, []),
    "tfhe_gpu_build_id": (C.c_char_p, []),
    "tfhe_gpu_build_kind": (C.c_int, []),
    "tfhe_gpu_create": (C.c_int, [C.POINTER(TfheParams), C.c_int, C.POINTER(vp)]),
    "tfhe_gpu_create_on_device": (C.c_int, [C.POINTER(TfheParams), C.c_int, C.POINTER(vp)]),
    "tfhe_gpu_destroy": (None, [vp]),
    "tfhe_gpu_last_error": (C.c_char_p, [vp]),
    "tfhe_gpu_sync": (C.c_int, [vp]),
    "tfhe_gpu_set_stream": (C.c_int, [vp, vp]),
    "tfhe_gpu_reset_stream": (C.c_int, [vp]),
    "tfhe_gpu_create_multi": (C.c_int, [C.POINTER(TfheParams), C.c_int, C.POINTER(C.c_int), C.POINTER(vp)]),
    "tfhe_gpu_num_devices": (C.c_int, [vp]),
    "tfhe_gpu_device_bootstraps": (C.c_int, [vp, C.POINTER(C.c_uint64), C.c_int]),
    "tfhe_gpu_near_tie_items": (C.c_int, [vp, C.POINTER(C.c_uint64)]),
    "tfhe_gpu_set_option": (C.c_int, [vp, C.c_int, C.c_int64]),
    "tfhe_gpu_get_option": (C.c_int, [vp, C.c_int, C.POINTER(C.c_int64)]),
    "tfhe_gpu_last_kernels": (C.c_char_p, [vp]),
    "tfhe_fft_tables": (C.c_int, [C.c_uint32, C.c_int, f64p, f64p, f64p, f64p]),
    "tfhe_gpu_load_cloud_key": (C.c_int, [vp, C.c_uint32, u32p, u32p, f64p, C.c_size_t, u32p, C.c_size_t]),
    "tfhe_gpu_keygen": (C.c_int, [vp, C.c_uint64, C.c_uint64, u32p, u32p, f64p, u32p]),
    "tfhe_gpu_key_blob_bytes": (C.c_int, [vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "tfhe_gpu_key_fingerprint": (C.c_int, [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "tfhe_gpu_export_key_device": (C.c_int, [vp, vp, vp, u32p, u32p]),
    "tfhe_gpu_import_key_device": (C.c_int, [vp, vp, vp, C.c_uint32, u32p]),
    "tfhe_gpu_export_cloud_key": (C.c_int, [vp, C.POINTER(C.c_uint32), u32p, u32p, f64p, u32p]),
    "tfhe_cloud_key_write": (C.c_int, [C.c_char_p, C.POINTER(TfheParams), C.c_uint32, u32p, u32p, f64p, C.c_size_t,
                                       u32p, C.c_size_t]),
    "tfhe_cloud_key_read": (C.c_int, [C.c_char_p, C.POINTER(TfheParams), C.POINTER(C.c_uint32), u32p, u32p, f64p,
                                      C.c_size_t, u32p, C.c_size_t]),
    "tfhe_gpu_save_cloud_key": (C.c_int, [vp, C.c_char_p]),
    "tfhe_gpu_load_cloud_key_file": (C.c_int, [vp, C.c_char_p]),
    "tfhe_gpu_bootstrap_batch": (C.c_int, [vp, u32p, u32p, C.c_size_t]),
    "tfhe_gpu_bootstrap_without_key_switch_batch": (C.c_int, [vp, u32p, u32p, C.c_size_t]),
    "tfhe_gpu_gate_batch": (C.c_int, [vp, u8p, u32p, u32p, u32p, C.c_size_t]),
    "tfhe_gpu_circuit_eval": (C.c_int, [vp, C.c_size_t, u32p, C.c_size_t, u8p, u32p, u32p, C.c_size_t, u32p, u32p,
                                        C.POINTER(C.c_uint32)]),
    "tfhe_gpu_circuit_eval_dev": (C.c_int, [vp, C.c_size_t, vp, C.c_size_t, u8p, u32p, u32p, C.c_size_t, u32p, vp,
                                        C.POINTER(C.c_uint32)]),
    "tfhe_circuit_schedule": (C.c_int, [C.c_size_t, C.c_size_t, u8p, u32p, u32p, C.c_uint32, C.c_int, u32p,
                                        C.POINTER(C.c_uint32)]),
    "tfhe_circuit_partition": (C.c_int, [C.c_size_t, C.c_size_t, u8p, u32p, u32p, C.c_int, u32p]),
    "tfhe_gpu_blind_rotate_batch": (C.c_int, [vp, u32p, u32p, u32p, C.c_size_t]),
    "tfhe_gpu_bootstrap_lut_batch": (C.c_int, [vp, u32p, u32p, u32p, C.c_size_t]),
    "tfhe_gpu_gate_batch_dev": (C.c_int, [vp, vp, vp, vp, vp, C.c_size_t]),
    "tfhe_gpu_bootstrap_batch_dev": (C.c_int, [vp, vp, vp, C.c_size_t]),
    "tfhe_gpu_profile_begin": (C.c_int, [vp]),
    "tfhe_gpu_profile_end": (C.c_int, [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "tfhe_gpu_fft_forward_batch": (C.c_int, [vp, u32p, f64p, C.c_size_t]),
    "tfhe_gpu_fft_inverse_batch": (C.c_int, [vp, f64p, u32p, C.c_size_t]),
    "tfhe_gpu_poly_mul_batch": (C.c_int, [vp, u32p, u32p, u32p, C.c_size_t]),
    "tfhe_gpu_external_product_batch": (C.c_int, [vp, f64p, C.c_uint32, u32p, u32p, C.c_size_t]),
    "tfhe_gpu_key_switch_batch": (C.c_int, [vp, u32p, u32p, C.c_size_t]),
    "tfhe_encrypt_bool_batch": (C.c_int, [C.POINTER(TfheParams), u32p, u8p, C.c_uint64, u32p, C.c_size_t]),
    "tfhe_decrypt_bool_batch": (C.c_int, [C.POINTER(TfheParams), u32p, u32p, u8p, C.c_size_t]),
    "tfhe_encrypt_lwe_message_batch": (C.c_int, [C.POINTER(TfheParams), u32p, u32p, C.c_uint32, C.c_uint64,
                                                 u32p, C.c_size_t]),
    "tfhe_decrypt_lwe_message_batch": (C.c_int, [C.POINTER(TfheParams), u32p, u32p, C.c_uint32, u32p,
                                                 C.c_size_t]),
    "tfhe_lut_generate": (C.c_int, [C.POINTER(TfheParams), C.c_uint32, u32p, u32p]),
    "tfhe_lut_generate_scaled": (C.c_int, [C.POINTER(TfheParams), C.c_uint32, C.c_double, u32p, u32p]),
    "tfhe_lut_generate_full": (C.c_int, [C.POINTER(TfheParams), C.c_uint32, u32p, u32p]),
    "tfhe_decomposition_offset": (C.c_int, [C.POINTER(TfheParams), u32p]),
    "tfhe_secret_key_new": (C.c_int, [C.POINTER(TfheParams), C.c_uint64, u32p, u32p]),
    "tfhe_gpu_reenc_key_load": (C.c_int, [vp, u32p, C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(vp)]),
    "tfhe_gpu_reenc_key_destroy": (None, [vp]),
    "tfhe_gpu_reencrypt_batch": (C.c_int, [vp, vp, u32p, u32p, C.c_size_t]),
    "tfhe_gpu_reencrypt_batch_dev": (C.c_int, [vp, vp, vp, vp, C.c_size_t]),
    "tfhe_gpu_bootstrap_lut_batch_dev": (C.c_int, [vp, vp, vp, vp, C.c_size_t]),
    "tfhe_public_key_gen": (C.c_int, [C.POINTER(TfheParams), u32p, C.c_size_t, C.c_double, C.c_uint64, u32p]),
    "tfhe_public_key_encrypt_bool_batch": (C.c_int, [C.POINTER(TfheParams), u32p, C.c_size_t, u8p, C.c_double,
                                                     C.c_uint64, u32p, C.c_size_t]),
    "tfhe_reenc_key_gen_symmetric": (C.c_int, [C.POINTER(TfheParams), u32p, u32p, C.c_double, C.c_uint32,
                                               C.c_uint32, C.c_uint64, u32p]),
    "tfhe_reenc_key_gen_asymmetric": (C.c_int, [C.POINTER(TfheParams), u32p, u32p, C.c_size_t, C.c_double,
                                                C.c_uint32, C.c_uint32, C.c_uint64, u32p]),
    "tfhe_gpu_trlwe_encrypt_batch": (C.c_int, [vp, u32p, f64p, C.c_double, C.c_uint64, u32p, C.c_size_t]),
    "tfhe_gpu_trlwe_decrypt_bool_batch": (C.c_int, [vp, u32p, u32p, u8p, C.c_size_t]),
    "tfhe_gpu_trgsw_encrypt_batch": (C.c_int, [vp, u32p, u32p, C.c_double, C.c_uint64, f64p, C.c_size_t]),
    "tfhe_gpu_trgsw_set_load": (C.c_int, [vp, f64p, C.c_size_t, C.POINTER(vp)]),
    "tfhe_gpu_trgsw_set_destroy": (None, [vp]),
    "tfhe_gpu_cmux_batch": (C.c_int, [vp, vp, u32p, u32p, u32p, u32p, C.c_size_t]),
    "tfhe_gpu_cmux_batch_dev": (C.c_int, [vp, vp, u32p, vp, vp, vp, C.c_size_t]),
    "tfhe_gpu_table_lookup_batch": (C.c_int, [vp, vp, u32p, C.c_uint32, u32p, u32p, C.c_size_t]),
    "tfhe_gpu_table_lookup_dev": (C.c_int, [vp, vp, u32p, C.c_uint32, vp, vp, C.c_size_t]),
    "tfhe_gpu_sample_extract_batch": (C.c_int, [vp, u32p, u32p, C.c_size_t, C.c_int, u32p, C.c_size_t]),
    "tfhe_gpu_sample_extract_dev": (C.c_int, [vp, vp, u32p, C.c_size_t, C.c_int, vp, C.c_size_t]),
    "tfhe_lookup_table_pack_bits": (C.c_int, [C.POINTER(TfheParams), C.POINTER(C.c_uint64), C.c_size_t, C.c_uint32,
                                              u32p]),
    "tfhe_gpu_rotate_by_bits_batch": (C.c_int, [vp, vp, u32p, u32p, C.c_uint32, u32p, u32p, C.c_size_t]),
    "tfhe_gpu_rotate_by_bits_dev": (C.c_int, [vp, vp, u32p, u32p, C.c_uint32, vp, vp, C.c_size_t]),
    "tfhe_packed_lookup_plan": (C.c_int, [C.POINTER(TfheParams), C.c_uint32, C.c_uint32, C.POINTER(PackedPlan)]),
    "tfhe_lookup_table_pack_slots": (C.c_int, [C.POINTER(TfheParams), C.POINTER(C.c_uint64), C.c_uint32, C.c_uint32,
                                               u32p]),
    "tfhe_gpu_packed_lookup_batch": (C.c_int, [vp, vp, u32p, C.c_uint32, C.c_uint32, u32p, u32p, C.c_size_t]),
    "tfhe_gpu_packed_lookup_dev": (C.c_int, [vp, vp, u32p, C.c_uint32, C.c_uint32, vp, vp, C.c_size_t]),
    "tfhe_gpu_packed_scatter_add_batch": (C.c_int, [vp, vp, u32p, C.c_uint32, C.c_uint32, u32p, u32p, C.c_size_t]),
    "tfhe_gpu_packed_scatter_add_dev": (C.c_int, [vp, vp, u32p, C.c_uint32, C.c_uint32, vp, vp, C.c_size_t]),
    "tfhe_cmux_graph_plan": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, u32p, u32p, u32p, u32p, u32p, C.c_uint32, u32p,
                                       C.c_uint32, u32p, u32p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "tfhe_gpu_cmux_graph_batch": (C.c_int, [vp, vp, u32p, C.c_uint32, u32p, C.c_uint32, C.c_uint32, u32p, u32p, u32p,
                                            u32p, u32p, C.c_uint32, u32p, C.c_int, u32p, C.c_size_t]),
    "tfhe_gpu_cmux_graph_dev": (C.c_int, [vp, vp, u32p, C.c_uint32, vp, C.c_uint32, C.c_uint32, u32p, u32p, u32p, u32p,
                                          u32p, C.c_uint32, u32p, C.c_int, vp, C.c_size_t]),
    "tfhe_gpu_packing_key_gen": (C.c_int, [vp, u32p, u32p, C.c_double, C.c_uint32, C.c_uint32, C.c_uint64, u32p]),
    "tfhe_gpu_packing_key_load": (C.c_int, [vp, u32p, C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(vp)]),
    "tfhe_gpu_packing_key_destroy": (None, [vp]),
    "tfhe_gpu_pack_tlwe_batch": (C.c_int, [vp, vp, u32p, u32p, C.c_size_t, u32p, C.c_size_t]),
    "tfhe_gpu_pack_tlwe_dev": (C.c_int, [vp, vp, vp, u32p, C.c_size_t, vp, C.c_size_t]),
    "tfhe_pack_tlwe": (C.c_int, [C.POINTER(TfheParams), u32p, C.c_uint32, C.c_uint32, u32p, u32p, C.c_size_t, u32p,
                                 C.c_size_t]),
    "tfhe_gpu_lut_set_load": (C.c_int, [vp, u32p, C.c_size_t, C.POINTER(vp)]),
    "tfhe_gpu_lut_set_destroy": (None, [vp]),
    "tfhe_gpu_lut_apply_batch": (C.c_int, [vp, vp, u32p, C.c_size_t, u32p, u32p, i32p, u32p, u32p, u32p, C.c_size_t]),
    "tfhe_gpu_lut_apply_dev": (C.c_int, [vp, vp, vp, C.c_size_t, u32p, u32p, i32p, u32p, u32p, vp, C.c_size_t]),
    "tfhe_gpu_lut_circuit_eval": (C.c_int, [vp, vp, C.c_size_t, u32p, C.c_size_t, u32p, u32p, i32p, u32p, u32p,
                                            C.c_size_t, u32p, u32p, C.POINTER(C.c_uint32)]),
    "tfhe_gpu_lut_circuit_eval_dev": (C.c_int, [vp, vp, C.c_size_t, vp, C.c_size_t, u32p, u32p, i32p, u32p, u32p,
                                                C.c_size_t, u32p, vp, C.POINTER(C.c_uint32)]),
    "tfhe_lut_circuit_schedule": (C.c_int, [C.c_size_t, C.c_size_t, u32p, u32p, u32p, C.POINTER(C.c_uint32)]),
    "tfhe_lut_round_tlwe": (C.c_int, [C.POINTER(TfheParams), C.c_uint32, u32p, u32p, C.c_size_t]),
    "tfhe_lut_interleave": (C.c_int, [C.POINTER(TfheParams), u32p, C.c_uint32, u32p]),
    "tfhe_gpu_lut_apply_multi_batch": (C.c_int, [vp, vp, u32p, C.c_size_t, u32p, u32p, i32p, u32p, u32p, u32p, u32p,
                                                 C.c_size_t]),
    "tfhe_gpu_lut_apply_multi_dev": (C.c_int, [vp, vp, vp, C.c_size_t, u32p, u32p, i32p, u32p, u32p, u32p, vp,
                                               C.c_size_t]),
    "tfhe_gpu_lut_circuit_eval_multi": (C.c_int, [vp, vp, C.c_size_t, u32p, C.c_size_t, u32p, u32p, i32p, u32p, u32p,
                                                  u32p, C.c_size_t, u32p, u32p, C.POINTER(C.c_uint32)]),
    "tfhe_gpu_lut_circuit_eval_multi_dev": (C.c_int, [vp, vp, C.c_size_t, vp, C.c_size_t, u32p, u32p, i32p, u32p,
                                                      u32p, u32p, C.c_size_t, u32p, vp, C.POINTER(C.c_uint32)]),
    "tfhe_lut_circuit_schedule_multi": (C.c_int, [C.c_size_t, C.c_size_t, u32p, u32p, u32p, u32p,
                                                  C.POINTER(C.c_uint32)]),
    "tfhe_lut_spread": (C.c_int, [C.POINTER(TfheParams), u32p, C.c_uint32, C.c_uint32, u32p, C.c_size_t]),
    "tfhe_gpu_lut_spread_batch": (C.c_int, [vp, u32p, C.c_uint32, C.c_uint32, u32p, C.c_size_t]),
    "tfhe_gpu_lut_spread_dev": (C.c_int, [vp, vp, C.c_uint32, C.c_uint32, vp, C.c_size_t]),
    "tfhe_gpu_bootstrap_lut_each_batch": (C.c_int, [vp, u32p, u32p, u32p, C.c_size_t]),
    "tfhe_gpu_bootstrap_lut_each_dev": (C.c_int, [vp, vp, vp, vp, C.c_size_t]),
    "tfhe_gpu_lut_apply2_batch": (C.c_int, [vp, vp, vp, C.c_uint32, u32p, C.c_size_t, u32p, u32p, u32p, u32p,
                                            C.c_size_t]),
    "tfhe_gpu_lut_apply2_dev": (C.c_int, [vp, vp, vp, C.c_uint32, vp, C.c_size_t, u32p, u32p, u32p, vp, C.c_size_t]),
    "tfhe_gpu_lut_circuit_eval_select": (C.c_int, [vp, vp, vp, C.c_uint32, C.c_size_t, u32p, C.c_size_t, u32p, u32p,
                                                   i32p, u32p, u32p, u32p, u32p, u32p, u32p, C.c_size_t, u32p, u32p,
                                                   C.POINTER(C.c_uint32)]),
    "tfhe_gpu_lut_circuit_eval_select_dev": (C.c_int, [vp, vp, vp, C.c_uint32, C.c_size_t, vp, C.c_size_t, u32p, u32p,
                                                       i32p, u32p, u32p, u32p, u32p, u32p, u32p, C.c_size_t, u32p, vp,
                                                       C.POINTER(C.c_uint32)]),
    "tfhe_gpu_lut_select_batch": (C.c_int, [vp, vp, C.c_uint32, u32p, C.c_size_t, u32p, u32p, i32p, u32p, u32p, u32p,
                                            u32p, C.c_size_t]),
    "tfhe_gpu_lut_select_dev": (C.c_int, [vp, vp, C.c_uint32, vp, C.c_size_t, u32p, u32p, i32p, u32p, u32p, u32p, vp,
                                          C.c_size_t]),
    "tfhe_lut_circuit_schedule_select": (C.c_int, [C.c_size_t, C.c_size_t, u32p, u32p, u32p, C.c_uint32, u32p, u32p,
                                                   u32p, C.POINTER(C.c_uint32)]),
    "tfhe_lut_generate_ext": (C.c_int, [C.POINTER(TfheParams), C.c_uint32, C.c_uint32, u32p, u32p]),
    "tfhe_lut_ext_rotate": (C.c_int, [C.POINTER(TfheParams), C.c_uint32, u32p, C.c_uint32, u32p]),
    "tfhe_lut_ext_mod_switch": (C.c_int, [C.POINTER(TfheParams), C.c_uint32, C.c_uint32]),
    "tfhe_gpu_blind_rotate_ext_batch": (C.c_int, [vp, C.c_uint32, u32p, u32p, u32p, C.c_size_t]),
    "tfhe_gpu_lut_apply_ext_batch": (C.c_int, [vp, vp, C.c_uint32, u32p, C.c_size_t, u32p, u32p, i32p, u32p, u32p, u32p,
                                               C.c_size_t]),
    "tfhe_gpu_lut_apply_ext_dev": (C.c_int, [vp, vp, C.c_uint32, vp, C.c_size_t, u32p, u32p, i32p, u32p, u32p, vp,
                                             C.c_size_t]),
    "tfhe_gpu_bootstrap_lut_each_ext_batch": (C.c_int, [vp, C.c_uint32, u32p, u32p, u32p, C.c_size_t]),
    "tfhe_gpu_bootstrap_lut_each_ext_dev": (C.c_int, [vp, C.c_uint32, vp, vp, vp, C.c_size_t]),
    "tfhe_gpu_lut_select_ext_batch": (C.c_int, [vp, vp, C.c_uint32, C.c_uint32, u32p, C.c_size_t, u32p, u32p, i32p, u32p,
                                                u32p, u32p, u32p, C.c_size_t]),
    "tfhe_gpu_lut_select_ext_dev": (C.c_int, [vp, vp, C.c_uint32, C.c_uint32, vp, C.c_size_t, u32p, u32p, i32p, u32p,
                                              u32p, u32p, vp, C.c_size_t]),
    "tfhe_gpu_lut_circuit_eval_ext": (C.c_int, [vp, vp, vp, C.c_uint32, C.c_size_t, u32p, C.c_size_t, u32p, u32p, i32p,
                                                u32p, u32p, u32p, u32p, u32p, u32p, u32p, C.c_size_t, u32p, u32p,
                                                C.POINTER(C.c_uint32)]),
    "tfhe_gpu_lut_circuit_eval_ext_dev": (C.c_int, [vp, vp, vp, C.c_uint32, C.c_size_t, vp, C.c_size_t, u32p, u32p,
                                                    i32p, u32p, u32p, u32p, u32p, u32p, u32p, u32p, C.c_size_t, u32p,
                                                    vp, C.POINTER(C.c_uint32)]),
    "tfhe_lut_circuit_schedule_ext": (C.c_int, [C.c_size_t, C.c_size_t, u32p, u32p, u32p, C.c_uint32, u32p, u32p, u32p,
                                                u32p, C.POINTER(C.c_uint32), u32p]),
}
EXPORTED_SYMBOLS = tuple(_SIGS)


def load_library(path: str = LIB_PATH) -> C.CDLL:
    """Load the HIP library; raises (no fallback) if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(path):
        raise RuntimeError(f"libtfhe_gpu.so not built ({path}); run __graft_entry__.build() "
                           "or `make -C zig-tfhe_amd`")
    # If PyTorch is present, load its HIP runtime first: its libamdhip64 has
    # the same SONAME, so this library then binds to it and device pointers /
    # streams from torch are valid here (one runtime per process).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def _u32(a):
    a = np.ascontiguousarray(a, dtype=np.uint32)
    return a, a.ctypes.data_as(u32p)


def _f64(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(f64p)


_ABSENT = object()  # an argument the C entry does not take (None is one it takes as NULL)


def build_id() -> str:
    """tfhe_gpu_build_id: hash of the gfx950 kernels object the loaded library carries."""
    return load_library().tfhe_gpu_build_id().decode()


def build_kind() -> int:
    """tfhe_gpu_build_kind: BUILD_PRODUCT, or BUILD_AB for a development build
    (knock-out / timing / losing-form variants), which contexts refuse unless
    TFHE_ALLOW_AB_BUILD=1."""
    return load_library().tfhe_gpu_build_kind()


class TfheError(RuntimeError):
    """A nonzero C-ABI status; `status` is the TFHE_ERR_* code."""

    def __init__(self, msg: str, status: int = 0):
        super().__init__(msg)
        self.status = status


def fft_tables(N: int = 1024, source: int = TWIDDLES_GLIBC):
    """tfhe_fft_tables: (twist_re, twist_im, stage_re, stage_im) as the context builds them."""
    lib = load_library()
    t = [np.zeros(N // 2, np.float64), np.zeros(N // 2, np.float64), np.zeros(N // 2 - 1, np.float64),
         np.zeros(N // 2 - 1, np.float64)]
    rc = lib.tfhe_fft_tables(N, source, *[a.ctypes.data_as(f64p) for a in t])
    if rc != 0:
        raise TfheError(f"tfhe_fft_tables: status {rc}")
    return tuple(t)


class Context:
    """One HIP device + its resident CloudKey (tfhe_gpu_ctx), or with
    `devices` a multi-device context (tfhe_gpu_create_multi): batches are
    sharded over the devices, the key is broadcast once over RCCL."""

    def __init__(self, params="128", device: int = 0, devices=None):
        self.lib = load_library()
        self.params = make_params(params) if not isinstance(params, TfheParams) else params
        h = vp()
        if devices is None:
            rc = self.lib.tfhe_gpu_create_on_device(C.byref(self.params), device, C.byref(h))
            what = "tfhe_gpu_create_on_device"
        else:
            devs = (C.c_int * len(devices))(*devices)
            rc = self.lib.tfhe_gpu_create_multi(C.byref(self.params), len(devices), devs, C.byref(h))
            what = "tfhe_gpu_create_multi"
            device = devices[0]
        if rc != 0:  # tfhe_gpu_last_error(NULL): this thread's last failed create
            raise TfheError(f"{what} failed ({rc}): {self.lib.tfhe_gpu_last_error(None).decode()}", rc)
        self.h = h
        self.device = device

    @classmethod
    def multi(cls, params="128", num_devices: int = 1, devices=None):
        return cls(params, devices=list(devices) if devices is not None else list(range(num_devices)))

    @property
    def num_devices(self) -> int:
        return self.lib.tfhe_gpu_num_devices(self.h)

    def near_tie_items(self) -> int:
        """Items the margin guard recomputed in the reference's expression trees
        (tfhe_gpu_near_tie_items), as of the last synchronisation."""
        v = C.c_uint64()
        self.check(self.lib.tfhe_gpu_near_tie_items(self.h, C.byref(v)), "near_tie_items")
        return v.value

    def device_bootstraps(self) -> np.ndarray:
        """Blind rotations launched per device since creation (tfhe_gpu_device_bootstraps)."""
        n = self.num_devices
        out = np.zeros(n, np.uint64)
        rc = self.lib.tfhe_gpu_device_bootstraps(self.h, out.ctypes.data_as(C.POINTER(C.c_uint64)), n)
        if rc < 0:
            self.check(rc, "device_bootstraps")
        return out

    def set_option(self, name: str, value: int):
        """tfhe_gpu_set_option (kernel forms, twiddle source; OPTIONS)."""
        if name == "br_form" and isinstance(value, str):
            value = int(value) if value.isdigit() else BR_FORMS[value]
        key = READONLY_OPTIONS[name] if name in READONLY_OPTIONS else OPTIONS[name]  # read-only: the library refuses
        self.check(self.lib.tfhe_gpu_set_option(self.h, key, int(value)), f"set_option({name})")

    def get_option(self, name: str) -> int:
        v = C.c_int64()
        key = READONLY_OPTIONS[name] if name in READONLY_OPTIONS else OPTIONS[name]
        self.check(self.lib.tfhe_gpu_get_option(self.h, key, C.byref(v)), f"get_option({name})")
        return v.value

    def reset_options(self):
        for k, v in OPTION_DEFAULTS.items():
            if self.get_option(k) != v:
                self.set_option(k, v)

    @contextlib.contextmanager
    def options(self, **kw):
        """Temporarily set options (A/B runs, tests).  On exit each option named
        in `kw` goes back to the value it had on entry (not to its default:
        a `twiddles` choice made before the block survives it)."""
        before = {k: self.get_option(k) for k in kw}
        try:
            for k, v in kw.items():
                self.set_option(k, v)
            yield self
        finally:
            for k, v in before.items():
                if self.get_option(k) != v:
                    self.set_option(k, v)

    def last_kernels(self) -> str:
        """Kernel names of this context's last bootstrap launch (tfhe_gpu_last_kernels)."""
        return self.lib.tfhe_gpu_last_kernels(self.h).decode()

    def close(self):
        if getattr(self, "h", None):
            self.lib.tfhe_gpu_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc: int, what: str):
        if rc != 0:
            raise TfheError(f"{what}: status {rc}: {self.lib.tfhe_gpu_last_error(self.h).decode()}", rc)

    @property
    def n1(self) -> int:
        return self.params.n + 1

    # ---- keys
    def load_cloud_key(self, offset, testvec, bk, ksk):
        tv, _ = _u32(testvec)
        bk, bkp = _f64(bk)
        ksk, kp = _u32(ksk)
        N = self.params.N
        self.check(self.lib.tfhe_gpu_load_cloud_key(self.h, offset, tv[:N].ctypes.data_as(u32p),
                                                    tv[N:].ctypes.data_as(u32p), bkp, bk.size, kp, ksk.size),
                   "load_cloud_key")

    def keygen(self, secret_seed: int, cloud_seed: int, want_host_copy: bool = False):
        p = self.params
        k0 = np.zeros(p.n, np.uint32)
        k1 = np.zeros(p.N, np.uint32)
        bk = ksk = None
        bkp = kp = None
        if want_host_copy:
            bk = np.zeros((p.n, 2 * p.L, 2, p.N), np.float64)
            ksk = np.zeros((p.N * p.iks_t * (1 << p.basebit), p.n + 1), np.uint32)
            bkp, kp = bk.ctypes.data_as(f64p), ksk.ctypes.data_as(u32p)
        self.check(self.lib.tfhe_gpu_keygen(self.h, secret_seed, cloud_seed, k0.ctypes.data_as(u32p),
                                            k1.ctypes.data_as(u32p), bkp, kp), "keygen")
        return SecretKey(p, k0, k1), (bk, ksk)

    def export_cloud_key(self):
        """The loaded CloudKey in the reference layout: (offset, testvec 2N, bk (n,2L,2,N) f64,
        ksk (N*t*2^basebit, n+1) u32; k = 0 rows zero)."""
        p = self.params
        off = C.c_uint32()
        tv = np.zeros(2 * p.N, np.uint32)
        bk = np.zeros((p.n, 2 * p.L, 2, p.N), np.float64)
        ksk = np.zeros((p.N * p.iks_t * (1 << p.basebit), p.n + 1), np.uint32)
        self.check(self.lib.tfhe_gpu_export_cloud_key(self.h, C.byref(off), tv[:p.N].ctypes.data_as(u32p),
                                                      tv[p.N:].ctypes.data_as(u32p), bk.ctypes.data_as(f64p),
                                                      ksk.ctypes.data_as(u32p)), "export_cloud_key")
        return off.value, tv, bk, ksk

    def save_cloud_key(self, path: str):
        """Key file (include/tfhe_gpu.h 'Cloud-key files'): the reference has no serialization."""
        self.check(self.lib.tfhe_gpu_save_cloud_key(self.h, os.fsencode(path)), "save_cloud_key")

    def load_cloud_key_file(self, path: str):
        self.check(self.lib.tfhe_gpu_load_cloud_key_file(self.h, os.fsencode(path)), "load_cloud_key_file")

    def key_blob_bytes(self):
        a, b = C.c_size_t(), C.c_size_t()
        self.check(self.lib.tfhe_gpu_key_blob_bytes(self.h, C.byref(a), C.byref(b)), "key_blob_bytes")
        return a.value, b.value

    def key_fingerprint(self):
        """tfhe_gpu_key_fingerprint: (bk, ksk) 64-bit sums of the resident device key."""
        a, b = C.c_uint64(), C.c_uint64()
        self.check(self.lib.tfhe_gpu_key_fingerprint(self.h, C.byref(a), C.byref(b)), "key_fingerprint")
        return a.value, b.value

    def export_key_device(self, bk_dev_ptr: int, ksk_dev_ptr: int):
        off = C.c_uint32()
        tv = np.zeros(2 * self.params.N, np.uint32)
        self.check(self.lib.tfhe_gpu_export_key_device(self.h, vp(bk_dev_ptr), vp(ksk_dev_ptr), C.byref(off),
                                                       tv.ctypes.data_as(u32p)), "export_key_device")
        return off.value, tv

    def import_key_device(self, bk_dev_ptr: int, ksk_dev_ptr: int, offset: int, testvec):
        tv, tvp = _u32(testvec)
        self.check(self.lib.tfhe_gpu_import_key_device(self.h, vp(bk_dev_ptr), vp(ksk_dev_ptr), offset, tvp),
                   "import_key_device")

    def set_stream(self, stream_ptr: int | None):
        """Run on a HIP stream handle (e.g. torch.cuda.current_stream().cuda_stream; 0 is the
        device's null stream, torch's default stream); None: back to the context's own stream."""
        if stream_ptr is None:
            self.check(self.lib.tfhe_gpu_reset_stream(self.h), "reset_stream")
        else:
            self.check(self.lib.tfhe_gpu_set_stream(self.h, vp(stream_ptr)), "set_stream")

    def sync(self):
        self.check(self.lib.tfhe_gpu_sync(self.h), "sync")

    def profile_begin(self):
        self.check(self.lib.tfhe_gpu_profile_begin(self.h), "profile_begin")

    def profile_end(self):
        """-> (blind_rotate_ms_total, key_switch_ms_total, launches), HIP events on the ctx stream."""
        br, ks, n = C.c_double(), C.c_double(), C.c_int()
        self.check(self.lib.tfhe_gpu_profile_end(self.h, C.byref(br), C.byref(ks), C.byref(n)), "profile_end")
        return br.value, ks.value, n.value

    # ---- batch bootstrap API
    def bootstrap_batch(self, cts):
        cts, cp = _u32(cts)
        out = np.zeros_like(cts)
        self.check(self.lib.tfhe_gpu_bootstrap_batch(self.h, cp, out.ctypes.data_as(u32p), cts.shape[0]),
                   "bootstrap_batch")
        return out

    def bootstrap_without_key_switch_batch(self, cts):
        """VanillaBootstrap.bootstrapWithoutKeySwitch (vanilla.zig:58-69): the
        reference's hybrid sampleExtractIndex2 form, n+1 words per item."""
        cts, cp = _u32(cts)
        out = np.zeros_like(cts)
        self.check(self.lib.tfhe_gpu_bootstrap_without_key_switch_batch(self.h, cp, out.ctypes.data_as(u32p),
                                                                        cts.shape[0]),
                   "bootstrap_without_key_switch_batch")
        return out

    def circuit_eval(self, inputs, ops, in_a, in_b, out_wires):
        """Level-scheduled gate DAG (tfhe_gpu_circuit_eval).  -> (outputs, bootstrap depth)."""
        inputs, ip = _u32(np.asarray(inputs, np.uint32).reshape(-1, self.params.n + 1))
        ops = np.ascontiguousarray(ops, np.uint8)
        in_a, ap = _u32(in_a)
        in_b, bp = _u32(in_b)
        out_wires, op_ = _u32(out_wires)
        out = np.zeros((out_wires.size, self.params.n + 1), np.uint32)
        lv = C.c_uint32()
        self.check(self.lib.tfhe_gpu_circuit_eval(self.h, inputs.shape[0], ip, ops.size, ops.ctypes.data_as(u8p), ap,
                                                  bp, out_wires.size, op_, out.ctypes.data_as(u32p), C.byref(lv)),
                   "circuit_eval")
        return out, lv.value

    def circuit_eval_dev(self, inputs_ptr, n_inputs, ops, in_a, in_b, out_wires, outputs_ptr):
        """tfhe_gpu_circuit_eval_dev: inputs / outputs in HBM (async on the context stream). -> depth."""
        ops = np.ascontiguousarray(ops, np.uint8)
        in_a, ap = _u32(in_a)
        in_b, bp = _u32(in_b)
        out_wires, op_ = _u32(out_wires)
        lv = C.c_uint32()
        self.check(self.lib.tfhe_gpu_circuit_eval_dev(self.h, n_inputs, vp(inputs_ptr), ops.size, ops.ctypes.data_as(u8p),
                                                      ap, bp, out_wires.size, op_, vp(outputs_ptr), C.byref(lv)),
                   "circuit_eval_dev")
        return lv.value

    def gate_batch(self, ops, a, b):
        ops = np.ascontiguousarray(ops, dtype=np.uint8)
        a, ap = _u32(a)
        b, bp = _u32(b)
        out = np.zeros_like(a)
        self.check(self.lib.tfhe_gpu_gate_batch(self.h, ops.ctypes.data_as(u8p), ap, bp,
                                                out.ctypes.data_as(u32p), ops.size), "gate_batch")
        return out

    def blind_rotate_batch(self, cts, testvec=None):
        cts, cp = _u32(cts)
        out = np.zeros((cts.shape[0], 2 * self.params.N), np.uint32)
        tvp = None
        if testvec is not None:
            tv, tvp = _u32(testvec)
        self.check(self.lib.tfhe_gpu_blind_rotate_batch(self.h, cp, tvp, out.ctypes.data_as(u32p),
                                                        cts.shape[0]), "blind_rotate_batch")
        return out

    def bootstrap_lut_batch(self, cts, testvec):
        cts, cp = _u32(cts)
        tv, tvp = _u32(testvec)
        out = np.zeros_like(cts)
        self.check(self.lib.tfhe_gpu_bootstrap_lut_batch(self.h, cp, tvp, out.ctypes.data_as(u32p),
                                                         cts.shape[0]), "bootstrap_lut_batch")
        return out

    def gate_batch_dev(self, ops_ptr, a_ptr, b_ptr, out_ptr, B):
        self.check(self.lib.tfhe_gpu_gate_batch_dev(self.h, vp(ops_ptr), vp(a_ptr), vp(b_ptr), vp(out_ptr), B),
                   "gate_batch_dev")

    def bootstrap_batch_dev(self, in_ptr, out_ptr, B):
        self.check(self.lib.tfhe_gpu_bootstrap_batch_dev(self.h, vp(in_ptr), vp(out_ptr), B), "bootstrap_batch_dev")

    def bootstrap_lut_batch_dev(self, in_ptr, tv_ptr, out_ptr, B):
        self.check(self.lib.tfhe_gpu_bootstrap_lut_batch_dev(self.h, vp(in_ptr), vp(tv_ptr), vp(out_ptr), B),
                   "bootstrap_lut_batch_dev")

    # ---- stage entry points
    def fft_forward(self, polys):
        x, xp = _u32(np.atleast_2d(polys))
        out = np.zeros(x.shape, np.float64)
        self.check(self.lib.tfhe_gpu_fft_forward_batch(self.h, xp, out.ctypes.data_as(f64p), x.shape[0]),
                   "fft_forward")
        return out

    def fft_inverse(self, freqs):
        f, fp = _f64(np.atleast_2d(freqs))
        out = np.zeros(f.shape, np.uint32)
        self.check(self.lib.tfhe_gpu_fft_inverse_batch(self.h, fp, out.ctypes.data_as(u32p), f.shape[0]),
                   "fft_inverse")
        return out

    def poly_mul(self, a, b):
        a, ap = _u32(np.atleast_2d(a))
        b, bp = _u32(np.atleast_2d(b))
        out = np.zeros(a.shape, np.uint32)
        self.check(self.lib.tfhe_gpu_poly_mul_batch(self.h, ap, bp, out.ctypes.data_as(u32p), a.shape[0]),
                   "poly_mul")
        return out

    def external_product(self, trlwes, trgsw_fft=None, bk_index=0):
        x, xp = _u32(np.atleast_2d(trlwes))
        out = np.zeros(x.shape, np.uint32)
        tp = None
        if trgsw_fft is not None:
            tg, tp = _f64(trgsw_fft)
        self.check(self.lib.tfhe_gpu_external_product_batch(self.h, tp, bk_index, xp, out.ctypes.data_as(u32p),
                                                            x.shape[0]), "external_product")
        return out

    def key_switch(self, lv1):
        x, xp = _u32(np.atleast_2d(lv1))
        out = np.zeros((x.shape[0], self.n1), np.uint32)
        self.check(self.lib.tfhe_gpu_key_switch_batch(self.h, xp, out.ctypes.data_as(u32p), x.shape[0]),
                   "key_switch")
        return out

    # ---- leveled operations: TRLWE / TRGSW encryption, CMUX, table lookup, extraction
    def trlwe_encrypt(self, key_lv1, mu, alpha: float | None = None, seed0: int = 1):
        """TRLWELv1.encryptF64 (trlwe.zig:30-64) of B plaintext polynomials mu (B, N) f64;
        item i uses DefaultPrng(seed0 + i).  -> (B, 2N) uint32."""
        mu, mp = _f64(np.atleast_2d(mu))
        out = np.zeros((mu.shape[0], 2 * self.params.N), np.uint32)
        alpha = self.params.alpha_lv1 if alpha is None else alpha
        self.check(self.lib.tfhe_gpu_trlwe_encrypt_batch(self.h, _u32(key_lv1)[1], mp, alpha, seed0,
                                                         out.ctypes.data_as(u32p), mu.shape[0]), "trlwe_encrypt")
        return out

    def trlwe_decrypt_bool(self, key_lv1, cts):
        """TRLWELv1.decryptBool (trlwe.zig:85-98): (B, 2N) -> (B, N) bool."""
        cts, cp = _u32(np.atleast_2d(cts))
        out = np.zeros((cts.shape[0], self.params.N), np.uint8)
        self.check(self.lib.tfhe_gpu_trlwe_decrypt_bool_batch(self.h, _u32(key_lv1)[1], cp, out.ctypes.data_as(u8p),
                                                              cts.shape[0]), "trlwe_decrypt_bool")
        return out.astype(bool)

    def trgsw_encrypt(self, key_lv1, mu, alpha: float | None = None, seed0: int = 1):
        """TRGSWLv1.encryptTorus + TRGSWLv1FFT.new (trgsw.zig:35-91) of the S torus words mu;
        TRGSW s draws its row seeds from DefaultPrng(seed0 + s).  -> (S, 2L, 2, N) f64."""
        mu, mp = _u32(np.atleast_1d(mu))
        p = self.params
        out = np.zeros((mu.size, 2 * p.L, 2, p.N), np.float64)
        alpha = p.alpha_bsk if alpha is None else alpha
        self.check(self.lib.tfhe_gpu_trgsw_encrypt_batch(self.h, _u32(key_lv1)[1], mp, alpha, seed0,
                                                         out.ctypes.data_as(f64p), mu.size), "trgsw_encrypt")
        return out

    def cmux(self, selectors: "TrgswSet", sel, in0, in1):
        """trgsw.cmux (trgsw.zig:260-284): out[i] = in1[i] where selectors[sel[i]] encrypts 1, else in0[i]."""
        sel, sp = _u32(np.atleast_1d(sel))
        in0, p0 = _u32(np.atleast_2d(in0))
        in1, p1 = _u32(np.atleast_2d(in1))
        out = np.zeros_like(in0)
        self.check(self.lib.tfhe_gpu_cmux_batch(self.h, selectors.h, sp, p0, p1, out.ctypes.data_as(u32p), sel.size),
                   "cmux")
        return out

    def cmux_dev(self, selectors: "TrgswSet", sel, in0_ptr, in1_ptr, out_ptr):
        """tfhe_gpu_cmux_batch_dev: the ciphertexts in HBM (sel stays a host array), async on the context stream."""
        sel, sp = _u32(np.atleast_1d(sel))
        self.check(self.lib.tfhe_gpu_cmux_batch_dev(self.h, selectors.h, sp, vp(in0_ptr), vp(in1_ptr), vp(out_ptr),
                                                    sel.size), "cmux_dev")

    def table_lookup(self, selectors: "TrgswSet", addr, table):
        """tfhe_gpu_table_lookup_batch: table (2^k, 2N) TRLWELv1, addr (Q, k) selector indices, bit 0 first.
        -> (Q, 2N): table[address_q]."""
        table, tp = _u32(np.atleast_2d(table))
        addr, ap = _u32(np.atleast_2d(addr))
        k = addr.shape[1]
        if table.shape[0] != 1 << k:
            raise ValueError(f"table_lookup: {k} address bits need a table of {1 << k} entries, got {table.shape[0]}")
        out = np.zeros((addr.shape[0], 2 * self.params.N), np.uint32)
        self.check(self.lib.tfhe_gpu_table_lookup_batch(self.h, selectors.h, ap, k, tp, out.ctypes.data_as(u32p),
                                                        addr.shape[0]), "table_lookup")
        return out

    def table_lookup_dev(self, selectors: "TrgswSet", addr, table_ptr, out_ptr):
        """tfhe_gpu_table_lookup_dev: table (2^k TRLWELv1) and outputs (Q TRLWELv1) in HBM, async."""
        addr, ap = _u32(np.atleast_2d(addr))
        self.check(self.lib.tfhe_gpu_table_lookup_dev(self.h, selectors.h, ap, addr.shape[1], vp(table_ptr),
                                                      vp(out_ptr), addr.shape[0]), "table_lookup_dev")

    def _graph_out_words(self, extract: int) -> int:
        if extract not in (0, 1, 2):
            raise ValueError(f"cmux_graph: extract is 0 (TRLWELv1), 1 (TLWELv1) or 2 (TLWELv0), got {extract}")
        return (2 * self.params.N, self.params.N + 1, self.n1)[extract]

    def cmux_graph(self, selectors: "TrgswSet", addr, graph: "CmuxGraph", leaves, extract: int = 0):
        """tfhe_gpu_cmux_graph_batch: `graph` evaluated for each of the Q rows of addr (Q, k) selector indices, variable
        j of the graph being address bit j; leaves (nL, 2N) TRLWELv1 shared by the queries.  -> (Q, R, words): the
        roots as TRLWELv1 (extract = 0), sampleExtractIndex(., 0) of them (1), or that key-switched to TLWELv0 (2)."""
        leaves, lp = _u32(np.atleast_2d(leaves))
        addr, ap = _u32(np.asarray(addr, np.uint32).reshape(-1, graph.k) if graph.k else np.zeros((len(addr), 0), np.uint32))
        if leaves.shape != (graph.n_leaves, 2 * self.params.N):
            raise ValueError(f"cmux_graph: the graph has {graph.n_leaves} leaves of {2 * self.params.N} words, got "
                             f"{leaves.shape}")
        out = np.zeros((addr.shape[0], len(graph.roots), self._graph_out_words(extract)), np.uint32)
        self.check(self.lib.tfhe_gpu_cmux_graph_batch(self.h, selectors.h, ap, graph.k, lp, graph.n_leaves,
                                                      *graph.pointers(), extract, out.ctypes.data_as(u32p),
                                                      addr.shape[0]), "cmux_graph")
        return out

    def cmux_graph_dev(self, selectors: "TrgswSet", addr, graph: "CmuxGraph", leaves_ptr, out_ptr, extract: int = 0):
        """tfhe_gpu_cmux_graph_dev: the leaves (nL TRLWELv1) and the Q * R outputs in HBM (addr and the graph stay
        host arrays), async on the context stream; the outputs must not overlap the leaves."""
        addr, ap = _u32(np.asarray(addr, np.uint32).reshape(-1, graph.k) if graph.k else np.zeros((len(addr), 0), np.uint32))
        self._graph_out_words(extract)
        self.check(self.lib.tfhe_gpu_cmux_graph_dev(self.h, selectors.h, ap, graph.k, vp(leaves_ptr), graph.n_leaves,
                                                    *graph.pointers(), extract, vp(out_ptr), addr.shape[0]),
                   "cmux_graph_dev")

    def sample_extract(self, trlwes, coef, key_switch: bool = False):
        """sampleExtractIndex (trlwe.zig:146-162) at coefficients coef of each TRLWE, then optionally
        identityKeySwitching: -> (B, C, N+1) TLWELv1 or (B, C, n+1) TLWELv0."""
        x, xp = _u32(np.atleast_2d(trlwes))
        coef, cp = _u32(np.atleast_1d(coef))
        out = np.zeros((x.shape[0], coef.size, self.n1 if key_switch else self.params.N + 1), np.uint32)
        self.check(self.lib.tfhe_gpu_sample_extract_batch(self.h, xp, cp, coef.size, int(key_switch),
                                                          out.ctypes.data_as(u32p), x.shape[0]), "sample_extract")
        return out

    def sample_extract_dev(self, trlwe_ptr, B, coef, out_ptr, key_switch: bool = False):
        """tfhe_gpu_sample_extract_dev: B TRLWELv1 and the B * C outputs in HBM (coef stays a host array), async."""
        coef, cp = _u32(np.atleast_1d(coef))
        self.check(self.lib.tfhe_gpu_sample_extract_dev(self.h, vp(trlwe_ptr), cp, coef.size, int(key_switch),
                                                        vp(out_ptr), B), "sample_extract_dev")

    def rotate_by_bits(self, selectors: "TrgswSet", sel, rot, trlwes):
        """tfhe_gpu_rotate_by_bits_batch: acc <- cmux(acc, X^rot[j] acc, selectors[sel[b, j]]) for j = 0 .. h-1 on
        each of the B TRLWELv1 `trlwes`; sel (B, h) selector indices, rot (h,) exponents in [0, 2N].  -> (B, 2N)."""
        rot, rp = _u32(np.atleast_1d(rot))
        x, xp = _u32(np.atleast_2d(trlwes))
        sel, sp = _u32(np.asarray(sel, np.uint32).reshape(x.shape[0], -1))
        if sel.shape[1] != rot.size:
            raise ValueError(f"rotate_by_bits: {rot.size} exponents need {rot.size} selectors per item, got {sel.shape[1]}")
        out = np.zeros_like(x)
        self.check(self.lib.tfhe_gpu_rotate_by_bits_batch(self.h, selectors.h, sp, rp, rot.size, xp,
                                                          out.ctypes.data_as(u32p), x.shape[0]), "rotate_by_bits")
        return out

    def rotate_by_bits_dev(self, selectors: "TrgswSet", sel, rot, in_ptr, out_ptr):
        """tfhe_gpu_rotate_by_bits_dev: the B = len(sel) TRLWELv1 and the outputs in HBM (sel (B, h) and rot stay
        host arrays), async on the context stream; the outputs must not overlap the inputs."""
        rot, rp = _u32(np.atleast_1d(rot))
        sel, sp = _u32(np.atleast_2d(sel))
        if sel.shape[1] != rot.size:
            raise ValueError(f"rotate_by_bits_dev: {rot.size} exponents need {rot.size} selectors per item, got {sel.shape[1]}")
        self.check(self.lib.tfhe_gpu_rotate_by_bits_dev(self.h, selectors.h, sp, rp, rot.size, vp(in_ptr), vp(out_ptr),
                                                        sel.shape[0]), "rotate_by_bits_dev")

    def packed_lookup(self, selectors: "TrgswSet", addr, width: int, table):
        """tfhe_gpu_packed_lookup_batch: table (2^v, 2N) TRLWELv1 holding 2^k entries of `width` bits side by side
        (packed_lookup_plan / lookup_table_pack_slots), addr (Q, k) selector indices, bit 0 first.  -> (Q, 2N):
        coefficient c < width of row q carries bit c of table[address_q]."""
        table, tp = _u32(np.atleast_2d(table))
        addr, ap = _u32(np.atleast_2d(addr))
        k = addr.shape[1]
        plan = packed_lookup_plan(self.params, k, width)
        if table.shape[0] != plan.trlwes:
            raise ValueError(f"packed_lookup: k = {k}, width = {width} need a table of {plan.trlwes} TRLWEs, "
                             f"got {table.shape[0]}")
        out = np.zeros((addr.shape[0], 2 * self.params.N), np.uint32)
        self.check(self.lib.tfhe_gpu_packed_lookup_batch(self.h, selectors.h, ap, k, width, tp, out.ctypes.data_as(u32p),
                                                         addr.shape[0]), "packed_lookup")
        return out

    def packed_lookup_dev(self, selectors: "TrgswSet", addr, width: int, table_ptr, out_ptr):
        """tfhe_gpu_packed_lookup_dev: the packed table and the Q outputs (TRLWELv1) in HBM, async."""
        addr, ap = _u32(np.atleast_2d(addr))
        self.check(self.lib.tfhe_gpu_packed_lookup_dev(self.h, selectors.h, ap, addr.shape[1], width, vp(table_ptr),
                                                       vp(out_ptr), addr.shape[0]), "packed_lookup_dev")

    def packed_scatter_add(self, selectors: "TrgswSet", addr, width: int, deltas, table):
        """tfhe_gpu_packed_scatter_add_batch, the write beside packed_lookup: deltas (Q, 2N) TRLWELv1, addr (Q, k)
        selector indices, bit 0 first; delta q is rotated to the slot of entry address_q, routed by the demux tree to
        that entry's TRLWE and added there (wrapping u32), so the phase of the entry's coefficients 0 .. width-1
        grows by that of delta q's; queries with one address all add.  -> the new table (2^v, 2N); `table` itself
        is not changed."""
        table, _ = _u32(np.atleast_2d(table))
        addr, ap = _u32(np.atleast_2d(addr))
        k = addr.shape[1]
        plan = packed_lookup_plan(self.params, k, width)
        if table.shape[0] != plan.trlwes:
            raise ValueError(f"packed_scatter_add: k = {k}, width = {width} need a table of {plan.trlwes} TRLWEs, "
                             f"got {table.shape[0]}")
        deltas, dp = _u32(np.asarray(deltas, np.uint32).reshape(addr.shape[0], 2 * self.params.N))
        out = table.copy()
        self.check(self.lib.tfhe_gpu_packed_scatter_add_batch(self.h, selectors.h, ap, k, width, dp,
                                                              out.ctypes.data_as(u32p), addr.shape[0]),
                   "packed_scatter_add")
        return out

    def packed_scatter_add_dev(self, selectors: "TrgswSet", addr, width: int, delta_ptr, table_ptr, table_trlwes=None):
        """tfhe_gpu_packed_scatter_add_dev: the Q deltas and the packed table in HBM, the table updated in place,
        async on the context stream; the deltas must not overlap the table.  table_ptr: a device address with
        table_trlwes, the number of TRLWELv1 behind it, or a tensor (data_ptr / numel), whose size is then checked
        like packed_scatter_add's table."""
        addr, ap = _u32(np.atleast_2d(addr))
        k = addr.shape[1]
        plan = packed_lookup_plan(self.params, k, width)
        if hasattr(table_ptr, "data_ptr"):
            table_trlwes, table_ptr = table_ptr.numel() * table_ptr.element_size() // (8 * self.params.N), table_ptr.data_ptr()
        if hasattr(delta_ptr, "data_ptr"):
            delta_ptr = delta_ptr.data_ptr()
        if table_trlwes is not None and table_trlwes != plan.trlwes:
            raise ValueError(f"packed_scatter_add_dev: k = {k}, width = {width} need a table of {plan.trlwes} TRLWEs, "
                             f"got {table_trlwes}")
        self.check(self.lib.tfhe_gpu_packed_scatter_add_dev(self.h, selectors.h, ap, k, width, vp(delta_ptr),
                                                            vp(table_ptr), addr.shape[0]), "packed_scatter_add_dev")

    def packed_write(self, selectors: "TrgswSet", key: "PackingKey", addr, width: int, new_cts, table):
        """Set entry address_q of a packed table to new_cts[q] ((Q, width, n+1) TLWELv0, fresh +-1/8 per bit), from
        existing calls around packed_scatter_add; needs the cloud key and a packing key.  -> the new table.
          1. packed_lookup at the addresses;
          2. sample_extract at coefficients 0 .. width-1 with the key switch: the entries' old bits;
          3. their plain bootstrap (tfhe_gpu_bootstrap_batch): old', fresh +-1/8;
          4. delta = new - old' on all n+1 words: 0 or +-1/4 per bit;
          5. pack_tlwe of each query's deltas into coefficients 0 .. width-1;
          6. packed_scatter_add.
        The addresses of one call must be distinct for set semantics: the library cannot see them, and two writes to
        one entry would both subtract the old value.  Every write adds noise to every entry of the table (the demux
        tree leaves noise in the leaves it does not address, and the packed delta has noise in every coefficient), so
        a table is refreshed after a number of writes by sample_extract, bootstrap and pack_table."""
        addr = np.ascontiguousarray(np.atleast_2d(addr), np.uint32)
        Q = addr.shape[0]
        new = np.asarray(new_cts, np.uint32).reshape(Q, width, self.n1)
        coef = np.arange(width, dtype=np.uint32)
        read = self.packed_lookup(selectors, addr, width, table)
        old = self.sample_extract(read, coef, key_switch=True)
        fresh = self.bootstrap_batch(old.reshape(Q * width, self.n1)).reshape(Q, width, self.n1)
        delta = self.pack_tlwe(key, new - fresh, coef)
        return self.packed_scatter_add(selectors, addr, width, delta, table)

    # ---- packing key switch: TLWELv0 -> coefficient slots of TRLWELv1 ----
    def pack_tlwe(self, key: "PackingKey", cts, coef):
        """tfhe_gpu_pack_tlwe_batch: cts (B, C, n+1) TLWELv0 (or (C, n+1): B = 1), coef (C,) distinct coefficients
        < N.  -> (B, 2N) TRLWELv1 whose coefficient coef[c] of row b carries the phase of cts[b, c]."""
        coef, cp = _u32(np.atleast_1d(coef))
        x, xp = _u32(np.asarray(cts, np.uint32).reshape(-1, max(coef.size, 1), self.n1))
        out = np.zeros((x.shape[0], 2 * self.params.N), np.uint32)
        self.check(self.lib.tfhe_gpu_pack_tlwe_batch(self.h, key.h, xp, cp, coef.size, out.ctypes.data_as(u32p),
                                                     x.shape[0]), "pack_tlwe")
        return out

    def pack_tlwe_dev(self, key: "PackingKey", in_ptr, B, coef, out_ptr):
        """tfhe_gpu_pack_tlwe_dev: the B * C TLWELv0 and the B TRLWELv1 in HBM (coef stays a host array), async."""
        coef, cp = _u32(np.atleast_1d(coef))
        self.check(self.lib.tfhe_gpu_pack_tlwe_dev(self.h, key.h, vp(in_ptr), cp, coef.size, vp(out_ptr), B),
                   "pack_tlwe_dev")

    def pack_table(self, key: "PackingKey", cts, k: int, width: int):
        """The packed table of packed_lookup from 2^k * width TLWELv0 computed on the server (entry-major, then
        bit): one pack call with B = plan.trlwes and coef[s * width + c] = s * stride + c.  -> (trlwes, 2N)."""
        plan = packed_lookup_plan(self.params, k, width)
        slots = 1 << plan.h
        x = np.asarray(cts, np.uint32).reshape(-1, self.n1)
        if x.shape[0] != (width << k):
            raise ValueError(f"pack_table: k = {k}, width = {width} need {width << k} ciphertexts, got {x.shape[0]}")
        coef = (np.arange(slots, dtype=np.uint32)[:, None] * plan.stride + np.arange(width, dtype=np.uint32)).reshape(-1)
        return self.pack_tlwe(key, x.reshape(plan.trlwes, slots * width, self.n1), coef)

    # ---- LUT circuits: linear combination, then bootstrap with the node's own table ----
    def _lut_batch(self, what, head, pool, nodes, theta=_ABSENT, m=None, dev=None):
        """The flat node batches, tfhe_gpu_<what>_batch(h, *head, pool, P, <nodes>, out, B): the nodes are lut_apply's
        with theta behind them where the entry takes one, or with m lut_select's.  pool (P, n+1) -> (outputs, n+1);
        with dev = (P, out_ptr) tfhe_gpu_<what>_dev on the pool pointer, nothing returned."""
        if m is None:
            d = pack_lut_nodes(nodes)
            desc = d.pointers()
        else:
            d, src, konst = _select_nodes(nodes, m)
            desc = (*d.pointers()[:4], src.ctypes.data_as(u32p), konst.ctypes.data_as(u32p))
        n_out = d.B
        if theta is not _ABSENT:
            th, thp = _theta(theta, d.B)
            desc += (thp,)
            n_out = d.B if th is None else int((1 << th.astype(np.uint64)).sum())
        if dev:
            self.check(getattr(self.lib, f"tfhe_gpu_{what}_dev")(self.h, *head, vp(pool), dev[0], *desc, vp(dev[1]), d.B),
                       what + "_dev")
            return None
        pool, pp = _u32(np.asarray(pool, np.uint32).reshape(-1, self.n1))
        out = np.zeros((n_out, self.n1), np.uint32)
        self.check(getattr(self.lib, f"tfhe_gpu_{what}_batch")(self.h, *head, pp, pool.shape[0], *desc,
                                                                out.ctypes.data_as(u32p), d.B), what)
        return out

    def _lut_circuit(self, what, lut_set, inputs, nodes, out_wires, key=(), theta=_ABSENT, select=_ABSENT, eta=_ABSENT,
                     dev=None):
        """The lut_circuit_eval family, tfhe_gpu_<what>: key = (packing_key, m) and theta, select, eta where the entry
        takes them.  inputs (n_inputs, n+1) -> (outputs, depth); with dev = (n_inputs, outputs_ptr) tfhe_gpu_<what>_dev
        on the inputs pointer -> depth."""
        d = pack_lut_nodes(nodes)
        more = [] if theta is _ABSENT else [_theta(theta, d.B)[1]]
        if select is not _ABSENT:
            more += _select_arrays(select, d.B)[1]
        if eta is not _ABSENT:
            more.append(_theta(eta, d.B)[1])
        head = [self.h, lut_set.h] + ([key[0].h if key[0] is not None else None, key[1]] if key else [])
        ow, owp = _u32(out_wires)
        depth = C.c_uint32(0)
        if dev:
            self.check(getattr(self.lib, f"tfhe_gpu_{what}_dev")(*head, dev[0], vp(inputs), d.B, *d.pointers(), *more,
                                                                  ow.size, owp, vp(dev[1]), C.byref(depth)), what + "_dev")
            return depth.value
        inputs, ip = _u32(np.asarray(inputs, np.uint32).reshape(-1, self.n1))
        out = np.zeros((ow.size, self.n1), np.uint32)
        self.check(getattr(self.lib, f"tfhe_gpu_{what}")(*head, inputs.shape[0], ip, d.B, *d.pointers(), *more, ow.size,
                                                          owp, out.ctypes.data_as(u32p), C.byref(depth)), what)
        return out, depth.value

    def lut_apply(self, lut_set: "LutSet", pool, nodes):
        """tfhe_gpu_lut_apply_batch: node i = (lut, terms[, const]) computes x = sum coef * pool[src] over its
        terms [(src, coef), ...] plus const on the b word (wrapping u32), then bootstraps x with lut_set[lut].
        pool (P, n+1) -> (B, n+1)."""
        return self._lut_batch("lut_apply", (lut_set.h,), pool, nodes)

    def lut_apply_dev(self, lut_set: "LutSet", pool_ptr, P, nodes, out_ptr):
        """tfhe_gpu_lut_apply_dev: the pool (P TLWELv0) and the B outputs in HBM (the nodes stay a host
        description), async on the context stream."""
        self._lut_batch("lut_apply", (lut_set.h,), pool_ptr, nodes, dev=(P, out_ptr))

    def blind_rotate_ext(self, eta: int, cts, testvecs):
        """tfhe_gpu_blind_rotate_ext_batch (stage entry): the extended blind rotation of (B, n+1) TLWELv0 under one
        extended test vector (E = 2^eta components, lut_generate_ext) -> (B, E, 2N), all E accumulators."""
        cts, cp = _u32(np.asarray(cts, np.uint32).reshape(-1, self.n1))
        E = 1 << eta if 0 <= eta < 8 else 1  # the library refuses eta > 2 itself
        tv, tvp = _u32(testvecs)
        out = np.zeros((cts.shape[0], E, 2 * self.params.N), np.uint32)
        self.check(self.lib.tfhe_gpu_blind_rotate_ext_batch(self.h, eta, cp, tvp, out.ctypes.data_as(u32p),
                                                            cts.shape[0]), "blind_rotate_ext")
        return out

    def lut_apply_ext(self, lut_set: "LutSet", eta: int, pool, nodes):
        """tfhe_gpu_lut_apply_ext_batch: lut_apply with the extended bootstrap; node i's lut names the extended table
        lut_set[lut * E .. lut * E + E - 1], E = 2^eta (lut_generate_ext).  eta = 0 is lut_apply."""
        return self._lut_batch("lut_apply_ext", (lut_set.h, eta), pool, nodes)

    def lut_apply_ext_dev(self, lut_set: "LutSet", eta: int, pool_ptr, P, nodes, out_ptr):
        """tfhe_gpu_lut_apply_ext_dev: the pool and the B outputs in HBM, async on the context stream."""
        self._lut_batch("lut_apply_ext", (lut_set.h, eta), pool_ptr, nodes, dev=(P, out_ptr))

    def lut_apply_multi(self, lut_set: "LutSet", pool, nodes, theta=None):
        """tfhe_gpu_lut_apply_multi_batch: lut_apply with theta[i] per node (None: all 0); node i gives the 2^theta[i]
        outputs of its interleaved table lut_set[lut] (lut_interleave) from one blind rotation of the rounded x.
        pool (P, n+1) -> (sum 2^theta, n+1), node-major."""
        return self._lut_batch("lut_apply_multi", (lut_set.h,), pool, nodes, theta=theta)

    def lut_apply_multi_dev(self, lut_set: "LutSet", pool_ptr, P, nodes, theta, out_ptr):
        """tfhe_gpu_lut_apply_multi_dev: the pool and the sum 2^theta outputs in HBM, async on the context stream."""
        self._lut_batch("lut_apply_multi", (lut_set.h,), pool_ptr, nodes, theta=theta, dev=(P, out_ptr))

    # ---- bivariate LUT bootstrap: spread, a test vector per item, the fused node ----
    def lut_spread(self, trlwes, w: int, rot: int):
        """tfhe_gpu_lut_spread_batch: (B, 2N) TRLWELv1 -> (B, 2N): on each half the negacyclic window sum of width w,
        multiplied by X^rot (lut_spread_host is the definition).  w = N/m, rot = 2N - N/(2m) turns slots x*w into the
        generator's test vector."""
        x, xp = _u32(np.asarray(trlwes, np.uint32).reshape(-1, 2 * self.params.N))
        out = np.zeros_like(x)
        self.check(self.lib.tfhe_gpu_lut_spread_batch(self.h, xp, w, rot, out.ctypes.data_as(u32p), x.shape[0]),
                   "lut_spread")
        return out

    def lut_spread_dev(self, in_ptr, w: int, rot: int, out_ptr, B):
        """tfhe_gpu_lut_spread_dev: the B TRLWELv1 in HBM (out_ptr may be in_ptr), async on the context stream."""
        self.check(self.lib.tfhe_gpu_lut_spread_dev(self.h, vp(in_ptr), w, rot, vp(out_ptr), B), "lut_spread_dev")

    def bootstrap_lut_each(self, cts, testvecs):
        """tfhe_gpu_bootstrap_lut_each_batch: bootstrap_lut_batch with one test vector per item: cts (B, n+1),
        testvecs (B, 2N) TRLWELv1 (any a) -> (B, n+1)."""
        cts, cp = _u32(np.asarray(cts, np.uint32).reshape(-1, self.n1))
        tv, tvp = _u32(np.asarray(testvecs, np.uint32).reshape(-1, 2 * self.params.N))
        if tv.shape[0] != cts.shape[0]:
            raise ValueError(f"bootstrap_lut_each: {cts.shape[0]} ciphertexts need as many test vectors, got {tv.shape[0]}")
        out = np.zeros_like(cts)
        self.check(self.lib.tfhe_gpu_bootstrap_lut_each_batch(self.h, cp, tvp, out.ctypes.data_as(u32p), cts.shape[0]),
                   "bootstrap_lut_each")
        return out

    def bootstrap_lut_each_dev(self, in_ptr, tv_ptr, out_ptr, B):
        """tfhe_gpu_bootstrap_lut_each_dev: inputs, the B test vectors and outputs in HBM, async."""
        self.check(self.lib.tfhe_gpu_bootstrap_lut_each_dev(self.h, vp(in_ptr), vp(tv_ptr), vp(out_ptr), B),
                   "bootstrap_lut_each_dev")

    def lut_apply2(self, lut_set: "LutSet", packing_key: "PackingKey", m: int, pool, nodes):
        """tfhe_gpu_lut_apply2_batch: node b = (fn, x_src, y_src) computes f_fn(pool[x_src], pool[y_src]) for two
        m-ary digits, lut_set = lut_generate2 tables of F functions ((F * m, 2N)): m level-1 bootstraps of y, the
        pack, the spread, one bootstrap of x with the packed test vector.  pool (P, n+1) -> (B, n+1)."""
        pool, pp = _u32(np.asarray(pool, np.uint32).reshape(-1, self.n1))
        fn, xs, ys = _apply2_nodes(nodes)
        out = np.zeros((fn.size, self.n1), np.uint32)
        self.check(self.lib.tfhe_gpu_lut_apply2_batch(self.h, lut_set.h, packing_key.h, m, pp, pool.shape[0],
                                                      fn.ctypes.data_as(u32p), xs.ctypes.data_as(u32p),
                                                      ys.ctypes.data_as(u32p), out.ctypes.data_as(u32p), fn.size),
                   "lut_apply2")
        return out

    def lut_apply2_dev(self, lut_set: "LutSet", packing_key: "PackingKey", m: int, pool_ptr, P, nodes, out_ptr):
        """tfhe_gpu_lut_apply2_dev: the pool and the B outputs in HBM (the nodes stay a host description), async."""
        fn, xs, ys = _apply2_nodes(nodes)
        self.check(self.lib.tfhe_gpu_lut_apply2_dev(self.h, lut_set.h, packing_key.h, m, vp(pool_ptr), P,
                                                    fn.ctypes.data_as(u32p), xs.ctypes.data_as(u32p),
                                                    ys.ctypes.data_as(u32p), vp(out_ptr), fn.size), "lut_apply2_dev")

    def lut_circuit_eval_multi(self, lut_set: "LutSet", inputs, nodes, theta, out_wires):
        """tfhe_gpu_lut_circuit_eval_multi: node g drives 2^theta[g] consecutive wires -> (outputs, depth)."""
        return self._lut_circuit("lut_circuit_eval_multi", lut_set, inputs, nodes, out_wires, theta=theta)

    def lut_circuit_eval_multi_dev(self, lut_set: "LutSet", inputs_ptr, n_inputs, nodes, theta, out_wires, outputs_ptr):
        """tfhe_gpu_lut_circuit_eval_multi_dev: inputs and outputs in HBM, async; returns the bootstrap depth."""
        return self._lut_circuit("lut_circuit_eval_multi", lut_set, inputs_ptr, nodes, out_wires, theta=theta,
                                 dev=(n_inputs, outputs_ptr))

    def lut_circuit_eval(self, lut_set: "LutSet", inputs, nodes, out_wires):
        """tfhe_gpu_lut_circuit_eval: nodes as in lut_apply with wires for sources -> (outputs, depth)."""
        return self._lut_circuit("lut_circuit_eval", lut_set, inputs, nodes, out_wires)

    def lut_circuit_eval_dev(self, lut_set: "LutSet", inputs_ptr, n_inputs, nodes, out_wires, outputs_ptr):
        """tfhe_gpu_lut_circuit_eval_dev: inputs and outputs in HBM, async; returns the bootstrap depth."""
        return self._lut_circuit("lut_circuit_eval", lut_set, inputs_ptr, nodes, out_wires, dev=(n_inputs, outputs_ptr))

    # ---- select nodes: a node whose table is made of wires (include/tfhe_gpu.h "Select nodes") ----
    def lut_circuit_eval_select(self, lut_set: "LutSet", packing_key: "PackingKey", m: int, inputs, nodes, theta,
                                select, out_wires):
        """tfhe_gpu_lut_circuit_eval_select: select = (sel_off, sel_wire, sel_konst), node g being a select node
        over its m entries sel_wire[sel_off[g] : sel_off[g+1]] (LUT_ENTRY_CONST: the constant sel_konst[j]), or
        None for lut_circuit_eval_multi -> (outputs, depth)."""
        return self._lut_circuit("lut_circuit_eval_select", lut_set, inputs, nodes, out_wires, key=(packing_key, m),
                                 theta=theta, select=select)

    def lut_circuit_eval_select_dev(self, lut_set: "LutSet", packing_key: "PackingKey", m: int, inputs_ptr, n_inputs,
                                    nodes, theta, select, out_wires, outputs_ptr):
        """tfhe_gpu_lut_circuit_eval_select_dev: inputs and outputs in HBM, async; returns the bootstrap depth."""
        return self._lut_circuit("lut_circuit_eval_select", lut_set, inputs_ptr, nodes, out_wires, key=(packing_key, m),
                                 theta=theta, select=select, dev=(n_inputs, outputs_ptr))

    def lut_select(self, packing_key: "PackingKey", m: int, pool, nodes):
        """tfhe_gpu_lut_select_batch: node b = (terms, entries[, const]) bootstraps x = sum coef * pool[src] + const
        with the test vector packed from its m entries, each a pool index or ("const", word): the output decrypts
        to what entry number x decrypts to.  pool (P, n+1) -> (B, n+1)."""
        return self._lut_batch("lut_select", (packing_key.h, m), pool, nodes, m=m)

    def lut_select_dev(self, packing_key: "PackingKey", m: int, pool_ptr, P, nodes, out_ptr):
        """tfhe_gpu_lut_select_dev: the pool and the B outputs in HBM (the nodes stay a host description), async."""
        self._lut_batch("lut_select", (packing_key.h, m), pool_ptr, nodes, m=m, dev=(P, out_ptr))

    # ---- extended nodes: an eta per node, select nodes on extended tables (include/tfhe_gpu.h "Extended nodes") ----
    def bootstrap_lut_each_ext(self, eta: int, cts, testvecs):
        """tfhe_gpu_bootstrap_lut_each_ext_batch: the extended bootstrap of item i with its one test vector
        testvecs[i] (any a) in all 2^eta components: cts (B, n+1), testvecs (B, 2N) -> (B, n+1)."""
        cts, cp = _u32(np.asarray(cts, np.uint32).reshape(-1, self.n1))
        tv, tvp = _u32(np.asarray(testvecs, np.uint32).reshape(-1, 2 * self.params.N))
        if tv.shape[0] != cts.shape[0]:
            raise ValueError(f"bootstrap_lut_each_ext: {cts.shape[0]} ciphertexts need as many test vectors, got {tv.shape[0]}")
        out = np.zeros_like(cts)
        self.check(self.lib.tfhe_gpu_bootstrap_lut_each_ext_batch(self.h, eta, cp, tvp, out.ctypes.data_as(u32p),
                                                                  cts.shape[0]), "bootstrap_lut_each_ext")
        return out

    def bootstrap_lut_each_ext_dev(self, eta: int, in_ptr, tv_ptr, out_ptr, B):
        """tfhe_gpu_bootstrap_lut_each_ext_dev: inputs, the B test vectors and outputs in HBM, async."""
        self.check(self.lib.tfhe_gpu_bootstrap_lut_each_ext_dev(self.h, eta, vp(in_ptr), vp(tv_ptr), vp(out_ptr), B),
                   "bootstrap_lut_each_ext_dev")

    def lut_select_ext(self, packing_key: "PackingKey", m: int, eta: int, pool, nodes):
        """tfhe_gpu_lut_select_ext_batch: lut_select with the extended bootstrap, so m may be 32 (eta = 1) or 64
        (eta = 2) at the UINT4 key's margin; nodes as lut_select takes them.  pool (P, n+1) -> (B, n+1)."""
        return self._lut_batch("lut_select_ext", (packing_key.h, m, eta), pool, nodes, m=m)

    def lut_select_ext_dev(self, packing_key: "PackingKey", m: int, eta: int, pool_ptr, P, nodes, out_ptr):
        """tfhe_gpu_lut_select_ext_dev: the pool and the B outputs in HBM, async."""
        self._lut_batch("lut_select_ext", (packing_key.h, m, eta), pool_ptr, nodes, m=m, dev=(P, out_ptr))

    def lut_circuit_eval_ext(self, lut_set: "LutSet", packing_key: "PackingKey", m: int, inputs, nodes, theta, select,
                             eta, out_wires):
        """tfhe_gpu_lut_circuit_eval_ext: lut_circuit_eval_select with eta per node (None: that call); an ordinary
        node with eta > 0 reads the extended table lut of the set, a select node with eta > 0 runs the extended
        bootstrap on its packed table -> (outputs, depth)."""
        return self._lut_circuit("lut_circuit_eval_ext", lut_set, inputs, nodes, out_wires, key=(packing_key, m or 0),
                                 theta=theta, select=select, eta=eta)

    def lut_circuit_eval_ext_dev(self, lut_set: "LutSet", packing_key: "PackingKey", m: int, inputs_ptr, n_inputs, nodes,
                                 theta, select, eta, out_wires, outputs_ptr):
        """tfhe_gpu_lut_circuit_eval_ext_dev: inputs and outputs in HBM, async; returns the bootstrap depth."""
        return self._lut_circuit("lut_circuit_eval_ext", lut_set, inputs_ptr, nodes, out_wires, key=(packing_key, m or 0),
                                 theta=theta, select=select, eta=eta, dev=(n_inputs, outputs_ptr))


@dataclass
class SecretKey:
    """key.SecretKey (key.zig:34-58): binary lv0 / lv1 keys."""
    params: TfheParams
    key_lv0: np.ndarray
    key_lv1: np.ndarray

    def encrypt_bool(self, bits, seed0: int = 1):
        """TLWELv0.encryptBool per bit, DefaultPrng(seed0 + i) in place of getUniqueSeed()."""
        lib = load_library()
        bits = np.ascontiguousarray(np.atleast_1d(bits), dtype=np.uint8)
        out = np.zeros((bits.size, self.params.n + 1), np.uint32)
        rc = lib.tfhe_encrypt_bool_batch(C.byref(self.params), _u32(self.key_lv0)[1], bits.ctypes.data_as(u8p),
                                         seed0, out.ctypes.data_as(u32p), bits.size)
        if rc:
            raise TfheError(f"encrypt_bool: {rc}")
        return out

    def decrypt_bool(self, cts):
        lib = load_library()
        cts, cp = _u32(np.atleast_2d(cts))
        out = np.zeros(cts.shape[0], np.uint8)
        rc = lib.tfhe_decrypt_bool_batch(C.byref(self.params), _u32(self.key_lv0)[1], cp,
                                         out.ctypes.data_as(u8p), cts.shape[0])
        if rc:
            raise TfheError(f"decrypt_bool: {rc}")
        return out.astype(bool)

    def encrypt_lwe_message(self, msgs, m: int, seed0: int = 1):
        lib = load_library()
        msgs, mp = _u32(np.atleast_1d(msgs))
        out = np.zeros((msgs.size, self.params.n + 1), np.uint32)
        rc = lib.tfhe_encrypt_lwe_message_batch(C.byref(self.params), _u32(self.key_lv0)[1], mp, m, seed0,
                                                out.ctypes.data_as(u32p), msgs.size)
        if rc:
            raise TfheError(f"encrypt_lwe_message: {rc}")
        return out

    def decrypt_lwe_message(self, cts, m: int):
        lib = load_library()
        cts, cp = _u32(np.atleast_2d(cts))
        out = np.zeros(cts.shape[0], np.uint32)
        rc = lib.tfhe_decrypt_lwe_message_batch(C.byref(self.params), _u32(self.key_lv0)[1], cp, m,
                                                out.ctypes.data_as(u32p), cts.shape[0])
        if rc:
            raise TfheError(f"decrypt_lwe_message: {rc}")
        return out


def decomposition_offset(params: TfheParams) -> int:
    """genDecompositionOffset (key.zig:121-131) of a parameter set (tfhe_decomposition_offset)."""
    v = C.c_uint32()
    rc = load_library().tfhe_decomposition_offset(C.byref(params), C.byref(v))
    if rc:
        raise TfheError(f"decomposition_offset: {rc}")
    return v.value


def secret_key_new(params: TfheParams, seed: int) -> SecretKey:
    """key.SecretKey.new (key.zig:41-57) with DefaultPrng(seed) in place of getUniqueSeed()."""
    lib = load_library()
    k0, k1 = np.zeros(params.n, np.uint32), np.zeros(params.N, np.uint32)
    rc = lib.tfhe_secret_key_new(C.byref(params), seed, k0.ctypes.data_as(u32p), k1.ctypes.data_as(u32p))
    if rc:
        raise TfheError(f"secret_key_new: {rc}")
    return SecretKey(params, k0, k1)


class PublicKeyLv0:
    """proxy_reenc.PublicKeyLv0 (proxy_reenc.zig:35-121): `size` encryptions of zero under key_lv0.
    Encryption e uses DefaultPrng(seed0 + e); size defaults to 2n (:44-54)."""

    def __init__(self, sk: SecretKey, seed0: int, size: int | None = None, alpha: float | None = None):
        p = self.params = sk.params
        size = 2 * p.n if size is None else size
        alpha = p.alpha_lv0 if alpha is None else alpha
        self.encryptions = np.zeros((size, p.n + 1), np.uint32)
        rc = load_library().tfhe_public_key_gen(C.byref(p), _u32(sk.key_lv0)[1], size, alpha, seed0,
                                                self.encryptions.ctypes.data_as(u32p))
        if rc:
            raise TfheError(f"public_key_gen: {rc}")

    def encrypt_bool(self, bits, seed0: int = 1, alpha: float | None = None):
        """encryptBool (:116-120); item i uses DefaultPrng(seed0 + i)."""
        p = self.params
        alpha = p.alpha_lv0 if alpha is None else alpha
        bits = np.ascontiguousarray(np.atleast_1d(bits), dtype=np.uint8)
        out = np.zeros((bits.size, p.n + 1), np.uint32)
        rc = load_library().tfhe_public_key_encrypt_bool_batch(
            C.byref(p), self.encryptions.ctypes.data_as(u32p), self.encryptions.shape[0],
            bits.ctypes.data_as(u8p), alpha, seed0, out.ctypes.data_as(u32p), bits.size)
        if rc:
            raise TfheError(f"public_key_encrypt_bool: {rc}")
        return out


class ProxyReencryptionKey:
    """proxy_reenc.ProxyReencryptionKey (proxy_reenc.zig:124-257): key_encryptions[(base*t*i)+(base*j)+k]
    = Enc_to(k * key_from[i] / 2^((j+1)*basebit)), k = 0 entries zero. Defaults: KSK_ALPHA and the
    parameter set's BASEBIT / IKS_T (:131-147). The c-th encryption uses DefaultPrng(seed0 + c)."""

    def __init__(self, key_encryptions: np.ndarray, basebit: int, t: int):
        self.key_encryptions, self.basebit, self.t = key_encryptions, basebit, t
        self.base = 1 << basebit

    @classmethod
    def _gen(cls, params, fn, extra, key_from, alpha, basebit, t, seed0):
        alpha = params.alpha_ksk if alpha is None else alpha
        basebit = params.basebit if basebit is None else basebit
        t = params.iks_t if t is None else t
        out = np.zeros(((1 << basebit) * t * params.n, params.n + 1), np.uint32)
        rc = fn(C.byref(params), _u32(key_from)[1], *extra, alpha, basebit, t, seed0, out.ctypes.data_as(u32p))
        if rc:
            raise TfheError(f"reenc_key_gen: {rc}")
        return cls(out, basebit, t)

    @classmethod
    def new_symmetric(cls, key_from: SecretKey, key_to: SecretKey, seed0: int, alpha=None, basebit=None, t=None):
        """newSymmetricWithParams (:214-256)."""
        return cls._gen(key_from.params, load_library().tfhe_reenc_key_gen_symmetric, [_u32(key_to.key_lv0)[1]],
                        key_from.key_lv0, alpha, basebit, t, seed0)

    @classmethod
    def new_asymmetric(cls, key_from: SecretKey, pk_to: PublicKeyLv0, seed0: int, alpha=None, basebit=None,
                       t=None):
        """newAsymmetricWithParams (:150-196)."""
        pk = pk_to.encryptions
        return cls._gen(key_from.params, load_library().tfhe_reenc_key_gen_asymmetric,
                        [pk.ctypes.data_as(u32p), pk.shape[0]], key_from.key_lv0, alpha, basebit, t, seed0)


class HipReencryptor:
    """reencryptTLWELv0 (proxy_reenc.zig:267-306) for a batch of TLWELv0, on the GPU: the re-encryption
    key lives in HBM (padded rows, like the KSK) and each ciphertext is one lane of the key-switch kernel."""

    def __init__(self, ctx: Context, key: ProxyReencryptionKey):
        self.ctx, self.h = ctx, vp()
        ke, kp = _u32(key.key_encryptions)
        ctx.check(ctx.lib.tfhe_gpu_reenc_key_load(ctx.h, kp, ke.size, key.basebit, key.t, C.byref(self.h)),
                  "reenc_key_load")

    def close(self):
        if self.h:
            self.ctx.lib.tfhe_gpu_reenc_key_destroy(self.h)
            self.h = vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reencrypt(self, cts):
        x, xp = _u32(np.atleast_2d(cts))
        out = np.zeros_like(x)
        self.ctx.check(self.ctx.lib.tfhe_gpu_reencrypt_batch(self.ctx.h, self.h, xp, out.ctypes.data_as(u32p),
                                                             x.shape[0]), "reencrypt")
        return out

    def reencrypt_dev(self, in_ptr, out_ptr, B):
        """Device-resident batch (async on the context stream): B TLWELv0 at in_ptr -> out_ptr."""
        self.ctx.check(self.ctx.lib.tfhe_gpu_reencrypt_batch_dev(self.ctx.h, self.h, vp(in_ptr), vp(out_ptr), B),
                       "reencrypt_dev")


class TrgswSet:
    """S TRGSWLv1FFT selectors (reference layout (S, 2L, 2, N) f64, as Context.trgsw_encrypt returns them)
    resident in HBM in the device layout (tfhe_gpu_trgsw_set): the `selectors` of Context.cmux /
    table_lookup, addressed by index."""

    def __init__(self, ctx: Context, trgsw_fft):
        self.ctx, self.h = ctx, vp()
        p = ctx.params
        t, tp = _f64(trgsw_fft)
        per = 2 * p.L * 2 * p.N
        if t.size == 0 or t.size % per:
            raise ValueError(f"TrgswSet: a TRGSWLv1FFT has 2L*2*N = {per} doubles, got {t.size}")
        self.size = t.size // per
        ctx.check(ctx.lib.tfhe_gpu_trgsw_set_load(ctx.h, tp, self.size, C.byref(self.h)), "trgsw_set_load")

    def close(self):
        if self.h:
            self.ctx.lib.tfhe_gpu_trgsw_set_destroy(self.h)
            self.h = vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PackingKey:
    """The packing key of Context.pack_tlwe / pack_table resident in HBM (tfhe_gpu_packing_key): rows
    (n * t * 2^basebit, 2N) uint32, row base*t*i + base*j + k a TRLWELv1 encryption of k * key_lv0[i] /
    2^((j+1)*basebit) at coefficient 0 (k = 0 rows zero).  Only the matrix-core layout stays on the device."""

    def __init__(self, ctx: Context, rows, basebit: int, t: int):
        self.ctx, self.h, self.basebit, self.t = ctx, vp(), basebit, t
        r, rp = _u32(rows)
        ctx.check(ctx.lib.tfhe_gpu_packing_key_load(ctx.h, rp, r.size, basebit, t, C.byref(self.h)), "packing_key_load")

    @staticmethod
    def default_shape(params: TfheParams):
        """The set's own (basebit, iks_t) where the one-hot GEMM has that shape, else (2, 8)."""
        b, t = params.basebit, params.iks_t
        return (b, t) if (b == 2 and 7 <= t <= 9) or (b == 5 and 2 <= t <= 3) else (2, 8)

    @staticmethod
    def generate_rows(ctx: Context, sk: "SecretKey", seed0: int, alpha=None, basebit=None, t=None):
        """tfhe_gpu_packing_key_gen: -> (rows (n * t * 2^basebit, 2N) uint32, basebit, t); row idx uses
        DefaultPrng(seed0 + idx).  Defaults: default_shape and alpha_lv1."""
        p = ctx.params
        db, dt = PackingKey.default_shape(p)
        basebit, t = db if basebit is None else basebit, dt if t is None else t
        alpha = p.alpha_lv1 if alpha is None else alpha
        rows = np.zeros((p.n * t << basebit, 2 * p.N), np.uint32)
        ctx.check(ctx.lib.tfhe_gpu_packing_key_gen(ctx.h, _u32(sk.key_lv0)[1], _u32(sk.key_lv1)[1], alpha, basebit, t,
                                                   seed0, rows.ctypes.data_as(u32p)), "packing_key_gen")
        return rows, basebit, t

    @classmethod
    def generate(cls, ctx: Context, sk: "SecretKey", seed0: int, alpha=None, basebit=None, t=None):
        rows, basebit, t = cls.generate_rows(ctx, sk, seed0, alpha, basebit, t)
        return cls(ctx, rows, basebit, t)

    def close(self):
        if self.h:
            self.ctx.lib.tfhe_gpu_packing_key_destroy(self.h)
            self.h = vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pack_tlwe_host(params: TfheParams, rows, basebit: int, t: int, cts, coef) -> np.ndarray:
    """tfhe_pack_tlwe (host only): the definition Context.pack_tlwe computes on the device, word for word."""
    coef, cp = _u32(np.atleast_1d(coef))
    x, xp = _u32(np.asarray(cts, np.uint32).reshape(-1, max(coef.size, 1), params.n + 1))
    r, rp = _u32(rows)
    out = np.zeros((x.shape[0], 2 * params.N), np.uint32)
    rc = load_library().tfhe_pack_tlwe(C.byref(params), rp, basebit, t, xp, cp, coef.size, out.ctypes.data_as(u32p),
                                       x.shape[0])
    if rc:
        raise TfheError(f"pack_tlwe_host: {rc}", rc)
    return out


LUT_MULTI_MAX_LOG = 3


def _theta(theta, B):
    """theta per node for the C ABI: (array or None, pointer or NULL)."""
    if theta is None:
        return None, None
    th = np.ascontiguousarray(theta, np.uint32).reshape(-1)
    if th.size != B:
        raise ValueError(f"theta needs one entry per node ({B}), got {th.size}")
    return th, th.ctypes.data_as(u32p)


def lut_round_tlwe(params: TfheParams, theta: int, cts) -> np.ndarray:
    """tfhe_lut_round_tlwe (host only): round_theta of the multi-output bootstrap on every word, (B, n+1) u32."""
    x, xp = _u32(np.asarray(cts, np.uint32).reshape(-1, params.n + 1))
    out = np.zeros_like(x)
    rc = load_library().tfhe_lut_round_tlwe(C.byref(params), theta, xp, out.ctypes.data_as(u32p), x.shape[0])
    if rc:
        raise TfheError(f"lut_round_tlwe: {rc}", rc)
    return out


def lut_interleave(params: TfheParams, tables) -> np.ndarray:
    """tfhe_lut_interleave (host only): 1, 2, 4 or 8 test vectors ((nu, 2N) u32) -> the one whose coefficient j,
    after a rotation by a multiple of nu, holds table j's value."""
    t, tp = _u32(np.asarray(tables, np.uint32).reshape(-1, 2 * params.N))
    nu = t.shape[0]
    if nu not in (1, 2, 4, 8):
        raise ValueError(f"lut_interleave takes 1, 2, 4 or 8 tables, got {nu}")
    out = np.zeros(2 * params.N, np.uint32)
    rc = load_library().tfhe_lut_interleave(C.byref(params), tp, nu.bit_length() - 1, out.ctypes.data_as(u32p))
    if rc:
        raise TfheError(f"lut_interleave: {rc}", rc)
    return out


def lut_spread_host(params: TfheParams, trlwes, w: int, rot: int) -> np.ndarray:
    """tfhe_lut_spread (host only): the definition Context.lut_spread computes on the device, word for word."""
    x, xp = _u32(np.asarray(trlwes, np.uint32).reshape(-1, 2 * params.N))
    out = np.zeros_like(x)
    rc = load_library().tfhe_lut_spread(C.byref(params), xp, w, rot, out.ctypes.data_as(u32p), x.shape[0])
    if rc:
        raise TfheError(f"lut_spread_host: {rc}", rc)
    return out


LUT_ENTRY_CONST = 0xFFFFFFFF  # TFHE_LUT_ENTRY_CONST: a select node's entry that is a constant


def _select_entries(entries, m: int, what: str):
    """m entries of a select node, each a wire / pool index or ("const", word) -> (sources, constants)."""
    entries = list(entries)
    if len(entries) != m:
        raise ValueError(f"{what}: a select node has m = {m} entries, got {len(entries)}")
    src, konst = [], []
    for e in entries:
        if isinstance(e, tuple):
            if len(e) != 2 or e[0] != "const":
                raise ValueError(f'{what}: an entry is a wire or ("const", word), got {e!r}')
            src.append(LUT_ENTRY_CONST)
            konst.append(int(e[1]) & 0xFFFFFFFF)
        else:
            src.append(int(e))
            konst.append(0)
    return src, konst


def _select_arrays(select, B):
    """(sel_off, sel_wire, sel_konst) or None -> (the arrays kept alive, their three pointers or NULLs)."""
    if select is None:
        return None, (None, None, None)
    arrs = [np.ascontiguousarray(a, np.uint32).reshape(-1) for a in select]
    if arrs[0].size != B + 1 or arrs[1].size != arrs[2].size:
        raise ValueError("select: sel_off needs one entry per node and one more, sel_wire and sel_konst one per entry")
    return arrs, tuple(a.ctypes.data_as(u32p) for a in arrs)


def _select_nodes(nodes, m: int):
    """nodes of Context.lut_select, (terms, entries[, const]) each -> (LutNodes with lut = 0, sel_src, sel_konst)."""
    flat, src, konst = [], [], []
    for node in nodes:
        terms, entries, k = (*node, 0) if len(node) == 2 else node
        s, c = _select_entries(entries, m, "lut_select")
        src += s
        konst += c
        flat.append((0, terms, k))
    return pack_lut_nodes(flat), np.array(src, np.uint32), np.array(konst, np.uint32)


def _apply2_nodes(nodes):
    """nodes of Context.lut_apply2: (fn, x_src, y_src) arrays, or a sequence of such triples -> three u32 arrays."""
    if isinstance(nodes, tuple) and len(nodes) == 3 and all(np.ndim(a) == 1 for a in nodes):
        cols = [np.ascontiguousarray(a, np.uint32) for a in nodes]
    else:
        t = np.asarray(list(nodes), np.uint32).reshape(-1, 3)
        cols = [np.ascontiguousarray(t[:, j]) for j in range(3)]
    if not (cols[0].size == cols[1].size == cols[2].size):
        raise ValueError("lut_apply2: fn, x_src and y_src need one entry per node each")
    return cols


class LutSet:
    """T test vectors ((T, 2N) u32 TRLWELv1, e.g. lut_generate's) resident in HBM (tfhe_gpu_lut_set): the
    tables of Context.lut_apply and LutCircuit, addressed by index."""

    def __init__(self, ctx: Context, tables):
        self.ctx, self.h = ctx, vp()
        t, tp = _u32(tables)
        per = 2 * ctx.params.N
        if t.size == 0 or t.size % per:
            raise ValueError(f"LutSet: a test vector has 2N = {per} words, got {t.size}")
        self.size = t.size // per
        ctx.check(ctx.lib.tfhe_gpu_lut_set_load(ctx.h, tp, self.size, C.byref(self.h)), "lut_set_load")

    def close(self):
        if self.h:
            self.ctx.lib.tfhe_gpu_lut_set_destroy(self.h)
            self.h = vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LutNodes:
    """The C ABI's description of B LUT nodes: CSR terms (term_off, src, coef), konst and lut per node."""

    def __init__(self, term_off, src, coef, konst, lut):
        self.term_off = np.ascontiguousarray(term_off, np.uint32)
        self.src = np.ascontiguousarray(src, np.uint32)
        self.coef = np.ascontiguousarray(coef, np.int32)
        self.konst = np.ascontiguousarray(konst, np.uint32)
        self.lut = np.ascontiguousarray(lut, np.uint32)
        self.B = self.lut.size
        if self.term_off.size != self.B + 1 or self.konst.size != self.B or self.src.size != self.coef.size:
            raise ValueError("LutNodes: term_off needs B + 1 entries, konst and lut B, src and coef one per term")

    def pointers(self):
        return (self.term_off.ctypes.data_as(u32p), self.src.ctypes.data_as(u32p), self.coef.ctypes.data_as(i32p),
                self.konst.ctypes.data_as(u32p), self.lut.ctypes.data_as(u32p))


def pack_lut_nodes(nodes) -> LutNodes:
    """nodes: a LutNodes, or a sequence of (lut, terms) / (lut, terms, const) with terms = [(source, coef), ...];
    const is a Torus word added to the b word."""
    if isinstance(nodes, LutNodes):
        return nodes
    off, src, coef, konst, lut = [0], [], [], [], []
    for node in nodes:
        t, terms, k = (*node, 0) if len(node) == 2 else node
        for s, c in terms:
            src.append(s)
            coef.append(c)
        off.append(len(src))
        konst.append(int(k) & 0xFFFFFFFF)
        lut.append(t)
    return LutNodes(off, src, coef, konst, lut)


class LutCircuit:
    """DAG builder for Context.lut_circuit_eval: every node is a small integer combination of earlier wires
    followed by a programmable bootstrap with one table of a LutSet, or (select, node2, lookup) with a table
    packed on the device from m earlier wires or constants.  Evaluated level by level, one combination launch
    and one bootstrap launch per level, every wire in HBM.

        c = LutCircuit(); a, b = c.input(), c.input(); s = c.node(0, [(a, 1), (b, 1)]); c.output(s)
        outs, depth = c.run(ctx, lut_set, [ct_a, ct_b])
    """

    def __init__(self):
        self.n_inputs = 0
        self.nodes = []  # (lut, terms, const)
        self.theta = []  # per node: log2 of its output count
        self.sel = []    # per node: None, or a select node's m entries (a wire or ("const", word) each)
        self.m = None    # the select nodes' m (one per circuit)
        self.eta = []    # per node: 0, or the extended bootstrap's eta (1 or 2)
        self.n_wires = 0
        self.outputs = []

    def input(self) -> int:
        if self.nodes:
            raise ValueError("declare every input before the first node")
        self.n_inputs += 1
        self.n_wires += 1
        return self.n_inputs - 1

    def node(self, lut: int, terms=(), const: int = 0, outputs: int = 1, eta: int = 0):
        """-> the node's wire; with outputs = 2, 4 or 8 (a multi-output node: lut is a lut_interleave table, the
        input is rounded to log2(outputs) fewer bits) the list of its wires, one per interleaved table.  eta = 1 or
        2: the extended bootstrap, lut naming the extended table (lut_generate_ext's 2^eta entries from lut * 2^eta)."""
        if outputs not in (1, 2, 4, 8):
            raise ValueError("a node has 1, 2, 4 or 8 outputs")
        if eta not in (0, 1, 2) or (eta and outputs != 1):
            raise ValueError("a node's eta is 0, 1 or 2, and an extended node has one output")
        w = self.n_wires
        terms = [(int(s), int(c)) for s, c in terms]
        if any(not 0 <= s < w for s, _ in terms):
            raise ValueError("node terms must read existing wires")
        self.nodes.append((int(lut), terms, int(const)))
        self.theta.append(outputs.bit_length() - 1)
        self.sel.append(None)
        self.eta.append(eta)
        self.n_wires += outputs
        return w if outputs == 1 else list(range(w, w + outputs))

    def select(self, terms, entries, const: int = 0, eta: int = 0) -> int:
        """A select node: the digit x = sum coef * wire over terms (+ const) picks one of the m = len(entries)
        entries, each an earlier wire or ("const", word); the table is packed from the entries on the device
        (tfhe_gpu_lut_circuit_eval_select).  -> the node's wire, which decrypts to what entry number x decrypts to.
        eta = 1 or 2: x is read by the extended bootstrap (tfhe_gpu_lut_circuit_eval_ext), which keeps the margin
        of m = 16 at m = 32 or 64 on the UINT4 key."""
        if eta not in (0, 1, 2):
            raise ValueError("a node's eta is 0, 1 or 2")
        entries = list(entries)
        m = len(entries)
        if m < 2 or m & (m - 1) or (self.m is not None and m != self.m):
            raise ValueError(f"a select node has m entries, m a power of two >= 2 and one m per circuit "
                             f"({self.m}); got {m}")
        src, _ = _select_entries(entries, m, "select")
        w = self.n_wires
        terms = [(int(s), int(c)) for s, c in terms]
        if any(not 0 <= s < w for s, _ in terms) or any(e != LUT_ENTRY_CONST and not 0 <= e < w for e in src):
            raise ValueError("a select node's terms and entries must read existing wires")
        self.m = m
        self.nodes.append((0, terms, int(const)))
        self.theta.append(0)
        self.sel.append(entries)
        self.eta.append(eta)
        self.n_wires += 1
        return w

    def node2(self, lut_base: int, x_terms, y_terms, m: int, eta: int = 0) -> int:
        """A bivariate node f(x, y) over two m-ary digits: m ordinary nodes with the tables lut_base + i
        (y -> f(i, y), lut_generate2's rows) over y_terms and one select node over x_terms -> its wire.  eta is the
        select node's: x may then be an m-ary digit with m up to 64; the m nodes over y stay ordinary."""
        if self.m is not None and m != self.m:
            raise ValueError(f"node2: the circuit's select nodes have m = {self.m}, got {m}")
        return self.select(x_terms, [self.node(lut_base + i, y_terms) for i in range(m)], eta=eta)

    def lookup(self, digit_terms_list, lut_base: int, m: int, eta: int = 0) -> int:
        """A k-digit lookup over plaintext tables: digit_terms_list holds the terms of the k digits, most
        significant first, and the set the m^(k-1) tables f(i_1, .., i_{k-1}, .) from lut_base in row-major order.
        m^(k-1) ordinary nodes on the last digit, then nested select nodes for the earlier digits -> the wire.
        eta is the select nodes'; the nodes on the last digit stay ordinary."""
        digits = list(digit_terms_list)
        if not digits:
            raise ValueError("lookup: no digits")
        k = len(digits)
        row = [self.node(lut_base + i, digits[-1]) for i in range(m ** (k - 1))]
        for terms in reversed(digits[:-1]):
            row = [self.select(terms, row[j * m:(j + 1) * m], eta=eta) for j in range(len(row) // m)]
        return row[0]

    @property
    def multi(self) -> bool:
        return any(self.theta)

    @property
    def has_select(self) -> bool:
        return any(e is not None for e in self.sel)

    @property
    def has_ext(self) -> bool:
        return any(self.eta)

    def select_arrays(self):
        """(sel_off, sel_wire, sel_konst) of tfhe_gpu_lut_circuit_eval_select, or None without select nodes."""
        if not self.has_select:
            return None
        off, wire, konst = [0], [], []
        for e in self.sel:
            if e is not None:
                s, c = _select_entries(e, self.m, "select")
                wire += s
                konst += c
            off.append(len(wire))
        return np.array(off, np.uint32), np.array(wire, np.uint32), np.array(konst, np.uint32)

    def output(self, *wires):
        self.outputs.extend(wires)

    def radix_add(self, a_digits, b_digits, msg_lut: int, carry_lut: int):
        """Radix addition, least significant digit first: per digit s = a_i + b_i + carry, message =
        LUT_msg(s), carry = LUT_carry(s).  -> the message wires, then the final carry as an extra digit."""
        out, carry = [], None
        for a, b in zip(a_digits, b_digits):
            terms = [(a, 1), (b, 1)] + ([(carry, 1)] if carry is not None else [])
            out.append(self.node(msg_lut, terms))
            carry = self.node(carry_lut, terms)
        return out + [carry]

    def radix_add_fused(self, a_digits, b_digits, lut: int):
        """radix_add with one two-output node per digit: lut is lut_interleave of the (message, carry) tables, at
        half the message modulus radix_add's tables may use (one bit of room pays for the second output)."""
        out, carry = [], None
        for a, b in zip(a_digits, b_digits):
            terms = [(a, 1), (b, 1)] + ([(carry, 1)] if carry is not None else [])
            msg, carry = self.node(lut, terms, outputs=2)
            out.append(msg)
        return out + [carry]

    def packed(self) -> LutNodes:
        return pack_lut_nodes(self.nodes)

    def schedule(self):
        """The level of every node as tfhe_gpu_lut_circuit_eval runs it (host only) -> (levels, depth)."""
        lib = load_library()
        d = self.packed()
        levels = np.zeros(max(d.B, 1), np.uint32)
        depth = C.c_uint32(0)
        if self.has_ext:
            return self.schedule_ext()[:2]
        if self.has_select:
            sel, selp = _select_arrays(self.select_arrays(), d.B)
            rc = lib.tfhe_lut_circuit_schedule_select(self.n_inputs, d.B, d.term_off.ctypes.data_as(u32p),
                                                      d.src.ctypes.data_as(u32p), _theta(self.theta, d.B)[1], self.m,
                                                      selp[0], selp[1], levels.ctypes.data_as(u32p), C.byref(depth))
        elif self.multi:
            rc = lib.tfhe_lut_circuit_schedule_multi(self.n_inputs, d.B, d.term_off.ctypes.data_as(u32p),
                                                     d.src.ctypes.data_as(u32p), _theta(self.theta, d.B)[1],
                                                     levels.ctypes.data_as(u32p), C.byref(depth))
        else:
            rc = lib.tfhe_lut_circuit_schedule(self.n_inputs, d.B, d.term_off.ctypes.data_as(u32p),
                                               d.src.ctypes.data_as(u32p), levels.ctypes.data_as(u32p), C.byref(depth))
        if rc:
            raise TfheError(f"lut_circuit_schedule: status {rc}", rc)
        return levels[:d.B], depth.value

    def schedule_ext(self):
        """tfhe_lut_circuit_schedule_ext (host only) -> (levels, depth, groups): groups[lv - 1, e] is the number of
        level lv's nodes with eta = e, the items of that level's launch for e."""
        d = self.packed()
        levels = np.zeros(max(d.B, 1), np.uint32)
        groups = np.zeros(3 * max(d.B, 1), np.uint32)
        depth = C.c_uint32(0)
        sel, selp = _select_arrays(self.select_arrays(), d.B)
        rc = load_library().tfhe_lut_circuit_schedule_ext(
            self.n_inputs, d.B, d.term_off.ctypes.data_as(u32p), d.src.ctypes.data_as(u32p), _theta(self.theta, d.B)[1],
            self.m or 0, selp[0], selp[1], _theta(self.eta, d.B)[1], levels.ctypes.data_as(u32p), C.byref(depth),
            groups.ctypes.data_as(u32p))
        if rc:
            raise TfheError(f"lut_circuit_schedule_ext: status {rc}", rc)
        return levels[:d.B], depth.value, groups[:3 * depth.value].reshape(-1, 3)

    def _select_m(self, packing_key, m):
        if packing_key is None:
            raise ValueError("a circuit with select nodes needs a packing_key")
        if m is not None and m != self.m:
            raise ValueError(f"the circuit's select nodes have m = {self.m}, got {m}")
        return self.m

    def run(self, ctx: "Context", lut_set: LutSet, inputs, packing_key: "PackingKey" = None, m: int = None):
        """packing_key (and m, which must be the select nodes' own) for a circuit with select nodes."""
        inputs = np.asarray(inputs, np.uint32).reshape(-1, ctx.params.n + 1)
        if inputs.shape[0] != self.n_inputs:
            raise ValueError(f"circuit has {self.n_inputs} inputs, got {inputs.shape[0]}")
        if self.has_ext:
            m = self._select_m(packing_key, m) if self.has_select else 0
            return ctx.lut_circuit_eval_ext(lut_set, packing_key, m, inputs, self.packed(), self.theta,
                                            self.select_arrays(), self.eta, np.array(self.outputs, np.uint32))
        if self.has_select:
            m = self._select_m(packing_key, m)
            return ctx.lut_circuit_eval_select(lut_set, packing_key, m, inputs,
                                               self.packed(), self.theta, self.select_arrays(),
                                               np.array(self.outputs, np.uint32))
        if self.multi:
            return ctx.lut_circuit_eval_multi(lut_set, inputs, self.packed(), self.theta,
                                              np.array(self.outputs, np.uint32))
        return ctx.lut_circuit_eval(lut_set, inputs, self.packed(), np.array(self.outputs, np.uint32))

    def run_dev(self, ctx: "Context", lut_set: LutSet, inputs_ptr, outputs_ptr, packing_key: "PackingKey" = None,
                m: int = None):
        """Inputs (n_inputs TLWELv0) and outputs in HBM; returns the bootstrap depth."""
        if self.has_ext:
            m = self._select_m(packing_key, m) if self.has_select else 0
            return ctx.lut_circuit_eval_ext_dev(lut_set, packing_key, m, inputs_ptr, self.n_inputs, self.packed(),
                                                self.theta, self.select_arrays(), self.eta,
                                                np.array(self.outputs, np.uint32), outputs_ptr)
        if self.has_select:
            m = self._select_m(packing_key, m)
            return ctx.lut_circuit_eval_select_dev(lut_set, packing_key, m, inputs_ptr,
                                                   self.n_inputs, self.packed(), self.theta, self.select_arrays(),
                                                   np.array(self.outputs, np.uint32), outputs_ptr)
        if self.multi:
            return ctx.lut_circuit_eval_multi_dev(lut_set, inputs_ptr, self.n_inputs, self.packed(), self.theta,
                                                  np.array(self.outputs, np.uint32), outputs_ptr)
        return ctx.lut_circuit_eval_dev(lut_set, inputs_ptr, self.n_inputs, self.packed(),
                                        np.array(self.outputs, np.uint32), outputs_ptr)


class CmuxGraph:
    """A CMUX graph (include/tfhe_gpu.h "CMUX graphs"): n_leaves leaves (value ids 0 .. n_leaves-1) and inner nodes
    over k encrypted bits, node v (value id n_leaves + v) being cmux(X^rlo value[lo], X^rhi value[hi], bit var): hi
    where the bit is 1.  Children are earlier values.  Context.cmux_graph evaluates the roots for a batch of queries;
    plan() and evaluate_plain() need no device.  The builders (less_than, equals_const, dfa, popcount) share equal
    nodes and drop a node whose two sides are the same value unrotated."""

    def __init__(self, k: int, n_leaves: int):
        self.k, self.n_leaves = int(k), int(n_leaves)
        self.var, self.lo, self.hi, self.rlo, self.rhi, self.roots = [], [], [], [], [], []
        self._shared = {}

    @property
    def n_nodes(self) -> int:
        return len(self.var)

    def node(self, var: int, lo: int, hi: int, rlo: int = 0, rhi: int = 0) -> int:
        """A new node; -> its value id.  Checked by plan() and the device calls, not here."""
        for a, x in zip((self.var, self.lo, self.hi, self.rlo, self.rhi), (var, lo, hi, rlo, rhi)):
            a.append(int(x))
        return self.n_leaves + len(self.var) - 1

    def _mux(self, var: int, lo: int, hi: int) -> int:
        """node() for the builders: lo itself when hi is the same value, and one node per (var, lo, hi)."""
        if lo == hi:
            return lo
        key = (var, lo, hi)
        if key not in self._shared:
            self._shared[key] = self.node(var, lo, hi)
        return self._shared[key]

    def root(self, *ids):
        self.roots.extend(int(i) for i in ids)
        return self

    def pointers(self):
        """(V, var, lo, hi, rlo, rhi, R, roots) as the C entries take them; the arrays live as long as self."""
        self._arrays = [np.array(a, np.uint32) for a in (self.var, self.lo, self.hi, self.rlo, self.rhi, self.roots)]
        p = [a.ctypes.data_as(u32p) if a.size else None for a in self._arrays]
        return (self.n_nodes, *p[:5], len(self.roots), p[5])

    def plan(self, N: int = 1024):
        """tfhe_cmux_graph_plan: (level per node, slot per node, depth, n_slots); TfheError where it refuses."""
        level, slot = np.zeros(self.n_nodes, np.uint32), np.zeros(self.n_nodes, np.uint32)
        depth, n_slots = C.c_uint32(), C.c_uint32()
        V, var, lo, hi, rlo, rhi, R, roots = self.pointers()
        rc = load_library().tfhe_cmux_graph_plan(self.n_leaves, V, self.k, var, lo, hi, rlo, rhi, R, roots, N,
                                                 level.ctypes.data_as(u32p) if V else None,
                                                 slot.ctypes.data_as(u32p) if V else None, C.byref(depth), C.byref(n_slots))
        if rc != 0:
            raise TfheError(f"cmux_graph_plan: status {rc}", rc)
        return level, slot, depth.value, n_slots.value

    def evaluate_plain(self, bits, N: int = 1024):
        """What the graph selects for plain bits (k of them): per root (leaf id, total rotation mod 2N), the root
        being X^rotation * leaf."""
        out = []
        for v in self.roots:
            rot = 0
            while v >= self.n_leaves:
                i = v - self.n_leaves
                b = int(bits[self.var[i]]) & 1
                rot += self.rhi[i] if b else self.rlo[i]
                v = self.hi[i] if b else self.lo[i]
            out.append((v, rot % (2 * N)))
        return out

    @staticmethod
    def bool_leaves(N: int = 1024) -> np.ndarray:
        """The two trivial leaves of the builders' decision diagrams: leaf 0 = false (-1/8 at every coefficient),
        leaf 1 = true (+1/8).  (2, 2N)."""
        out = np.zeros((2, 2 * N), np.uint32)
        out[0, N:], out[1, N:] = 0xE0000000, 0x20000000
        return out

    @staticmethod
    def testvec_leaf(values, N: int = 1024) -> np.ndarray:
        """A trivial test-vector leaf: coefficient c is +1/8 where values[c] is true, -1/8 elsewhere.  (1, 2N)."""
        out = np.zeros((1, 2 * N), np.uint32)
        out[0, N:] = 0xE0000000
        out[0, N:N + len(values)] = np.where(np.asarray(values, bool), 0x20000000, 0xE0000000)
        return out

    @classmethod
    def less_than(cls, nbits: int) -> "CmuxGraph":
        """a < b for two nbits-bit numbers: variables interleaved, most significant first (variable 2i is bit
        nbits-1-i of a, variable 2i+1 that bit of b); leaves as in bool_leaves; 3 nodes per bit pair."""
        g = cls(2 * nbits, 2)
        rest = 0  # a == b on the bits below: not less
        for i in reversed(range(nbits)):
            a0 = g._mux(2 * i + 1, rest, 1)  # a_i = 0: less if b_i = 1
            a1 = g._mux(2 * i + 1, 0, rest)  # a_i = 1: not less if b_i = 0
            rest = g._mux(2 * i, a0, a1)
        return g.root(rest)

    @classmethod
    def equals_const(cls, nbits: int, c: int) -> "CmuxGraph":
        """x == c for an nbits-bit x, variable j being bit j of x (least significant first)."""
        g = cls(nbits, 2)
        cur = 1
        for j in range(nbits):
            cur = g._mux(j, cur, 0) if (c >> j) & 1 == 0 else g._mux(j, 0, cur)
        return g.root(cur)

    @classmethod
    def dfa(cls, n_states: int, delta, accepting, length: int, bits_per_symbol: int) -> "CmuxGraph":
        """Does the automaton (start state 0, delta[state][symbol], accepting: a set of states) accept the string of
        `length` symbols?  Variable p * bits_per_symbol + b is bit b (least significant first) of symbol p.  Only
        the states reachable at a position get nodes."""
        g = cls(length * bits_per_symbol, 2)
        reach = [{0}]
        for _ in range(length):
            reach.append({int(delta[s][a]) for s in reach[-1] for a in range(1 << bits_per_symbol)})
        val = {s: int(s in accepting) for s in range(n_states)}
        for p in reversed(range(length)):
            nxt = {}
            for s in sorted(reach[p]):
                items = [val[int(delta[s][a])] for a in range(1 << bits_per_symbol)]
                for b in range(bits_per_symbol):
                    items = [g._mux(p * bits_per_symbol + b, items[2 * i], items[2 * i + 1]) for i in range(len(items) // 2)]
                nxt[s] = items[0]
            val = nxt
        return g.root(val[0])

    @classmethod
    def popcount(cls, nbits: int, N: int = 1024) -> "CmuxGraph":
        """A chain over one test-vector leaf tv (leaf 0): every set bit multiplies by X^(2N-1) = X^-1, so coefficient
        0 of the root is tv[popcount of the bits]."""
        g = cls(nbits, 1)
        cur = 0
        for j in range(nbits):
            cur = g.node(j, cur, cur, 0, 2 * N - 1)
        return g.root(cur)


def lookup_table_pack_bits(params: TfheParams, values, width: int) -> np.ndarray:
    """tfhe_lookup_table_pack_bits: entry e as a trivial TRLWELv1 whose coefficient c < width is
    +1/8 if bit c of values[e] is set, else -1/8.  -> (len(values), 2N) uint32."""
    vals = np.ascontiguousarray(np.atleast_1d(values), dtype=np.uint64)
    out = np.zeros((vals.size, 2 * params.N), np.uint32)
    rc = load_library().tfhe_lookup_table_pack_bits(C.byref(params), vals.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                    vals.size, width, out.ctypes.data_as(u32p))
    if rc:
        raise TfheError(f"lookup_table_pack_bits: status {rc}", rc)
    return out


def packed_lookup_plan(params: TfheParams, k: int, width: int) -> PackedPlan:
    """tfhe_packed_lookup_plan: the shape of a packed lookup of 2^k entries of `width` bits (stride, slots, h
    rotation steps, v tree levels, trlwes, cmuxes per query, rot[j] = 2N - stride * 2^j)."""
    plan = PackedPlan()
    rc = load_library().tfhe_packed_lookup_plan(C.byref(params), k, width, C.byref(plan))
    if rc:
        raise TfheError(f"packed_lookup_plan(k = {k}, width = {width}): status {rc}", rc)
    return plan


def lookup_table_pack_slots(params: TfheParams, values, width: int) -> np.ndarray:
    """tfhe_lookup_table_pack_slots: the 2^k values (width <= 64 bits each) as the packed table of
    Context.packed_lookup, +-1/8 per bit, unused coefficients 0.  -> (trlwes, 2N) uint32."""
    vals = np.ascontiguousarray(np.atleast_1d(values), dtype=np.uint64)
    k = int(vals.size).bit_length() - 1
    if vals.size != 1 << k or k == 0:
        raise ValueError(f"lookup_table_pack_slots: {vals.size} values are not 2^k, k >= 1")
    plan = packed_lookup_plan(params, k, width)
    out = np.zeros((plan.trlwes, 2 * params.N), np.uint32)
    rc = load_library().tfhe_lookup_table_pack_slots(C.byref(params), vals.ctypes.data_as(C.POINTER(C.c_uint64)), k,
                                                     width, out.ctypes.data_as(u32p))
    if rc:
        raise TfheError(f"lookup_table_pack_slots: status {rc}", rc)
    return out


class bit_utils:
    """bit_utils.zig (host-side plaintext plumbing of the examples): `convert` (:9-16) packs
    bits LSB first into an unsigned integer; `AsBits(T).toBits` (:24-27, :42-50) unpacks the
    width of T; `AsBits(T).encrypt` (:29-39) encrypts every bit (DefaultPrng(seed0 + i) per bit
    in place of getUniqueSeed())."""

    @staticmethod
    def convert(bits, width: int | None = None) -> int:
        bits = list(bits)
        width = len(bits) if width is None else width
        v = 0
        for i, b in enumerate(bits[:width]):
            v |= (1 if b else 0) << i
        return v

    @staticmethod
    def to_bits(value: int, width: int) -> np.ndarray:
        return np.array([(int(value) >> i) & 1 for i in range(width)], dtype=bool)

    @staticmethod
    def encrypt(value: int, width: int, sk: SecretKey, seed0: int = 1) -> np.ndarray:
        return sk.encrypt_bool(bit_utils.to_bits(value, width).astype(np.uint8), seed0=seed0)


def lut_generate(params: TfheParams, m: int, f) -> np.ndarray:
    """Generator.generateLookupTable (lut/generator.zig:85-135) for f: x -> f(x), x < m."""
    lib = load_library()
    table = np.array([f(x) for x in range(m)], dtype=np.uint32)
    tv = np.zeros(2 * params.N, np.uint32)
    rc = lib.tfhe_lut_generate(C.byref(params), m, table.ctypes.data_as(u32p), tv.ctypes.data_as(u32p))
    if rc:
        raise TfheError(f"lut_generate: {rc}")
    return tv


def lut_generate_ext(params: TfheParams, eta: int, m: int, f) -> np.ndarray:
    """tfhe_lut_generate_ext: the extended test vector of f (a callable or a table of m values) for the extended
    bootstrap, (E, 2N) with E = 2^eta: component j holds coefficients j, j + E, ... of the degree-N*E test vector."""
    table = np.array([f(x) for x in range(m)] if callable(f) else f, dtype=np.uint32)
    if table.shape != (m,):
        raise ValueError("lut_generate_ext: the table must have m entries")
    out = np.zeros((1 << eta if 0 <= eta < 8 else 1, 2 * params.N), np.uint32)
    rc = load_library().tfhe_lut_generate_ext(C.byref(params), eta, m, table.ctypes.data_as(u32p),
                                              out.ctypes.data_as(u32p))
    if rc != 0:
        raise TfheError(f"lut_generate_ext: status {rc}", rc)
    return out


def lut_ext_rotate_host(params: TfheParams, eta: int, comps, a: int) -> np.ndarray:
    """tfhe_lut_ext_rotate: X^a on the E = 2^eta components (E, 2N) of a polynomial pair of degree N*E,
    0 <= a <= 2N*E."""
    E = 1 << eta if 0 <= eta < 8 else 1
    x, xp = _u32(np.asarray(comps, np.uint32).reshape(E, 2 * params.N))
    out = np.zeros_like(x)
    rc = load_library().tfhe_lut_ext_rotate(C.byref(params), eta, xp, a, out.ctypes.data_as(u32p))
    if rc != 0:
        raise TfheError(f"lut_ext_rotate: status {rc}", rc)
    return out


def lut_ext_mod_switch(params: TfheParams, eta: int, word: int) -> int:
    """tfhe_lut_ext_mod_switch: (word + 2^(sh-1)) >> sh, sh = 32 - (nbit + 1) - eta: a position in [0, 2N*E]."""
    rc = load_library().tfhe_lut_ext_mod_switch(C.byref(params), eta, int(word) & 0xFFFFFFFF)
    if rc < 0:
        raise TfheError(f"lut_ext_mod_switch: status {rc}", rc)
    return rc


def lut_generate2(params: TfheParams, m: int, f) -> np.ndarray:
    """The m level-1 tables of a bivariate f(x, y) for Context.lut_apply2: row i = lut_generate of y -> f(i, y),
    (m, 2N) u32.  The tables of F functions stacked ((F * m, 2N)) make the call's LutSet."""
    return np.stack([lut_generate(params, m, lambda y, i=i: f(i, y)) for i in range(m)])


class Encoder:
    """lut/encoder.zig Encoder: message x -> f64ToTorus((x mod m) * scale);
    new(m) uses scale 1/(2m) (encoder.zig:29-42), with_scale a custom one (:49-54)."""

    def __init__(self, message_modulus: int, scale: float | None = None):
        self.message_modulus = int(message_modulus)
        self.scale = 1.0 / (2.0 * float(message_modulus)) if scale is None else float(scale)

    @classmethod
    def new(cls, message_modulus: int) -> "Encoder":
        return cls(message_modulus)

    @classmethod
    def with_scale(cls, message_modulus: int, scale: float) -> "Encoder":
        return cls(message_modulus, scale)


class LookupTable:
    """lut/lookup_table.zig LookupTable: a TRLWELv1 (a ++ b, 2N words) that the
    blind rotation uses as its test vector (tfhe_gpu_bootstrap_lut_batch)."""

    def __init__(self, poly=None, N: int = 1024):
        self.poly = np.zeros(2 * N, np.uint32) if poly is None else np.array(poly, np.uint32).reshape(-1)
        if self.poly.size != 2 * int(N):
            raise ValueError(f"LookupTable: a TRLWELv1 has 2N = {2 * int(N)} words (a ++ b), got {self.poly.size}")

    @classmethod
    def new(cls, N: int = 1024) -> "LookupTable":  # :23-27
        return cls(N=N)

    @classmethod
    def from_poly(cls, poly, N: int = 1024) -> "LookupTable":  # :33-35 (a copy of the TRLWELv1's words)
        return cls(poly, N)

    @property
    def a(self):
        return self.poly[: self.poly.size // 2]

    @property
    def b(self):
        return self.poly[self.poly.size // 2:]

    def get_poly(self) -> np.ndarray:  # :38-45
        return self.poly

    def copy_from(self, other: "LookupTable"):  # :51-54
        self.poly[:] = other.poly

    def clear(self):  # :57-61
        self.poly[:] = 0

    def is_empty(self) -> bool:  # :64-77
        return not self.poly.any()


class Generator:
    """lut/generator.zig Generator over the C ABI's table generation
    (tfhe_lut_generate_scaled / _full): poly_degree = lookup_table_size = N
    (the reference's poly_extend_factor 1)."""

    def __init__(self, encoder: Encoder, params: TfheParams | None = None):
        self.encoder = encoder
        self.params = params if params is not None else make_params("128")
        self.poly_degree_ = self.lookup_table_size_ = int(self.params.N)

    @classmethod
    def new(cls, message_modulus: int, params: TfheParams | None = None) -> "Generator":  # :29-41
        return cls(Encoder.new(message_modulus), params)

    @classmethod
    def with_scale(cls, message_modulus: int, scale: float, params: TfheParams | None = None) -> "Generator":  # :47-56
        return cls(Encoder.with_scale(message_modulus, scale), params)

    def message_modulus(self) -> int:  # :230-232
        return self.encoder.message_modulus

    def poly_degree(self) -> int:  # :235-237
        return self.poly_degree_

    def lookup_table_size(self) -> int:  # :240-242
        return self.lookup_table_size_

    def _check_lut(self, lut: LookupTable):
        """The C side writes 2N words into lut.poly: refuse anything else before the call."""
        p = lut.poly
        if not (isinstance(p, np.ndarray) and p.dtype == np.uint32 and p.flags.c_contiguous
                and p.size == 2 * int(self.params.N)):
            raise ValueError(f"LookupTable.poly must be a C-contiguous uint32 array of 2N = {2 * int(self.params.N)} "
                             f"words for these params, got {getattr(p, 'dtype', type(p))} of size {getattr(p, 'size', '?')}")

    def generate_lookup_table_assign(self, f, lut: LookupTable):  # :85-135
        self._check_lut(lut)
        m = self.encoder.message_modulus
        # Encoder.encode reduces f(x) (a usize) mod m in 64 bits (encoder.zig:66-74): reduce in
        # Python first, so f(x) >= 2^32 neither overflows the uint32 table nor wraps before the mod
        table = np.array([int(f(x)) % m for x in range(m)], dtype=np.uint32)
        rc = load_library().tfhe_lut_generate_scaled(C.byref(self.params), m, self.encoder.scale,
                                                     table.ctypes.data_as(u32p), lut.poly.ctypes.data_as(u32p))
        if rc:
            raise TfheError(f"lut_generate_scaled: {rc}", rc)

    def generate_lookup_table(self, f) -> LookupTable:  # :65-69
        lut = LookupTable.new(self.params.N)
        self.generate_lookup_table_assign(f, lut)
        return lut

    def generate_lookup_table_full_assign(self, f, lut: LookupTable):  # :155-191: f(x) is a Torus value
        self._check_lut(lut)
        m = self.encoder.message_modulus
        vals = np.array([int(f(x)) & 0xFFFFFFFF for x in range(m)], dtype=np.uint32)
        rc = load_library().tfhe_lut_generate_full(C.byref(self.params), m, vals.ctypes.data_as(u32p),
                                                   lut.poly.ctypes.data_as(u32p))
        if rc:
            raise TfheError(f"lut_generate_full: {rc}", rc)

    def generate_lookup_table_full(self, f) -> LookupTable:  # :144-148
        lut = LookupTable.new(self.params.N)
        self.generate_lookup_table_full_assign(f, lut)
        return lut

    def generate_lookup_table_custom(self, f, message_modulus: int, scale: float) -> LookupTable:  # :202-213
        return Generator(Encoder.with_scale(message_modulus, scale), self.params).generate_lookup_table(f)

    def mod_switch(self, x: int) -> int:  # :223-227, the reference's f64 expression
        scaled = (float(int(x) & 0xFFFFFFFF) / 4294967295.0) * float(self.lookup_table_size_)
        return int(scaled + 0.5) % self.lookup_table_size_


def cloud_key_write(path: str, params: TfheParams, offset: int, testvec, bk, ksk):
    """Write a CloudKey (reference layout) as a key file; host only (tfhe_cloud_key_write)."""
    lib = load_library()
    tv, _ = _u32(testvec)
    bk, bkp = _f64(bk)
    ksk, kp = _u32(ksk)
    N = params.N
    rc = lib.tfhe_cloud_key_write(os.fsencode(path), C.byref(params), offset, tv[:N].ctypes.data_as(u32p),
                                  tv[N:].ctypes.data_as(u32p), bkp, bk.size, kp, ksk.size)
    if rc:
        raise TfheError(f"cloud_key_write: status {rc}")


def cloud_key_read(path: str, params: TfheParams):
    """-> (offset, testvec 2N, bk (n,2L,2,N), ksk (N*t*2^basebit, n+1)); raises TfheError
    (status -5: I/O, -1: not a key file of this parameter set or checksum mismatch)."""
    lib = load_library()
    p = params
    off = C.c_uint32()
    tv = np.zeros(2 * p.N, np.uint32)
    bk = np.zeros((p.n, 2 * p.L, 2, p.N), np.float64)
    ksk = np.zeros((p.N * p.iks_t * (1 << p.basebit), p.n + 1), np.uint32)
    rc = lib.tfhe_cloud_key_read(os.fsencode(path), C.byref(p), C.byref(off), tv[:p.N].ctypes.data_as(u32p),
                                 tv[p.N:].ctypes.data_as(u32p), bk.ctypes.data_as(f64p), bk.size,
                                 ksk.ctypes.data_as(u32p), ksk.size)
    if rc:
        raise TfheError(f"cloud_key_read: status {rc}")
    return off.value, tv, bk, ksk


class HipBootstrap:
    """The bootstrap strategy object (bootstrap.zig:30-47, vanilla.zig:24-76)
    on the MI355X: bootstrap / bootstrap_without_key_switch / name, each over a
    single TLWELv0 (n+1,) or a batch (B, n+1).  The cloud key is the one the
    Context holds (the reference passes it per call)."""

    def __init__(self, ctx: Context):
        self.ctx = ctx

    @staticmethod
    def _run(fn, ct):
        ct = np.asarray(ct, np.uint32)
        out = fn(np.atleast_2d(ct))
        return out[0] if ct.ndim == 1 else out

    def bootstrap(self, ct):  # vanilla.zig:38-52
        return self._run(self.ctx.bootstrap_batch, ct)

    def bootstrap_without_key_switch(self, ct):  # vanilla.zig:58-69
        return self._run(self.ctx.bootstrap_without_key_switch_batch, ct)

    def name(self) -> str:  # vanilla.zig:72-75
        return "mi355x"


class Gates:
    """gates.Gates (gates.zig:25-152) on the MI355X bootstrap strategy.

    Each *_gate accepts single ciphertexts (n+1,) or batches (B, n+1); NOT /
    COPY / CONSTANT need no bootstrap and stay on the host like the reference.
    """

    def __init__(self, ctx: Context):
        self.ctx = ctx

    def bootstrap_strategy(self) -> str:  # gates.zig:43-45
        return "mi355x"

    def _gate(self, op, a, b):
        a = np.atleast_2d(np.asarray(a, np.uint32))
        b = np.atleast_2d(np.asarray(b, np.uint32))
        single = np.asarray(a).ndim == 2 and a.shape[0] == 1
        out = self.ctx.gate_batch(np.full(a.shape[0], op, np.uint8), a, b)
        return out[0] if single else out

    def nand_gate(self, a, b): return self._gate(NAND, a, b)
    def or_gate(self, a, b): return self._gate(OR, a, b)
    def and_gate(self, a, b): return self._gate(AND, a, b)
    def xor_gate(self, a, b): return self._gate(XOR, a, b)
    def xnor_gate(self, a, b): return self._gate(XNOR, a, b)
    def nor_gate(self, a, b): return self._gate(NOR, a, b)
    def and_ny_gate(self, a, b): return self._gate(ANDNY, a, b)
    def and_yn_gate(self, a, b): return self._gate(ANDYN, a, b)
    def or_ny_gate(self, a, b): return self._gate(ORNY, a, b)
    def or_yn_gate(self, a, b): return self._gate(ORYN, a, b)

    def mux_naive(self, a, b, c):
        """muxNaive (gates.zig:124-129): AND(a,b) || AND(NOT a, c), then OR — 2 levels."""
        a = np.atleast_2d(np.asarray(a, np.uint32))
        b = np.atleast_2d(np.asarray(b, np.uint32))
        c = np.atleast_2d(np.asarray(c, np.uint32))
        B = a.shape[0]
        lvl1 = self.ctx.gate_batch(np.full(2 * B, AND, np.uint8), np.concatenate([a, self.not_gate(a)]),
                                   np.concatenate([b, c]))
        return self.ctx.gate_batch(np.full(B, OR, np.uint8), lvl1[:B], lvl1[B:])

    @staticmethod
    def not_gate(a):  # gates.zig:132-135 (TLWELv0.neg)
        return (np.uint32(0) - np.asarray(a, np.uint32)).astype(np.uint32)

    @staticmethod
    def copy(a):  # gates.zig:138-141
        return np.array(a, np.uint32, copy=True)

    def constant(self, value: bool):  # gates.zig:144-151
        res = np.zeros(self.ctx.n1, np.uint32)
        mu = 0x20000000  # f64ToTorus(0.125)
        res[-1] = mu if value else (1 - mu) & 0xFFFFFFFF
        return res


class Circuit:
    """Gate DAG builder for Context.circuit_eval: the
    reference's circuits are sequences of Gates calls (gates.zig:48-151,
    examples/add_two_numbers.zig:24-73); here they are recorded as wires and
    evaluated level by level, one batched bootstrap launch per level.

        c = Circuit(); a, b = c.input(), c.input(); s = c.xor(a, b); c.output(s)
        outs, depth = c.run(ctx, [ct_a, ct_b])
    """

    def __init__(self):
        self.n_inputs = 0
        self.ops, self.ia, self.ib = [], [], []
        self.outputs = []

    def input(self) -> int:
        if self.ops:
            raise ValueError("declare every input before the first gate")
        self.n_inputs += 1
        return self.n_inputs - 1

    def gate(self, op: int, a: int, b: int | None = None) -> int:
        w = self.n_inputs + len(self.ops)
        if not (0 <= a < w) or (b is not None and not (0 <= b < w)):
            raise ValueError("gate inputs must be existing wires")
        self.ops.append(op)
        self.ia.append(a)
        self.ib.append(a if b is None else b)
        return w

    # gates.zig:48-151
    def nand(self, a, b): return self.gate(NAND, a, b)
    def or_(self, a, b): return self.gate(OR, a, b)
    def and_(self, a, b): return self.gate(AND, a, b)
    def xor(self, a, b): return self.gate(XOR, a, b)
    def xnor(self, a, b): return self.gate(XNOR, a, b)
    def nor(self, a, b): return self.gate(NOR, a, b)
    def and_ny(self, a, b): return self.gate(ANDNY, a, b)
    def and_yn(self, a, b): return self.gate(ANDYN, a, b)
    def or_ny(self, a, b): return self.gate(ORNY, a, b)
    def or_yn(self, a, b): return self.gate(ORYN, a, b)
    def not_(self, a): return self.gate(NOT, a)
    def copy(self, a): return self.gate(COPY, a)

    def mux(self, a, b, c):
        """muxNaive (gates.zig:124-129): OR(AND(a, b), AND(NOT a, c)) — 2 bootstrap levels."""
        return self.or_(self.and_(a, b), self.and_(self.not_(a), c))

    def full_adder(self, a, b, cin):
        """examples/add_two_numbers.zig:24-47: (sum, carry)."""
        x = self.xor(a, b)
        ab = self.and_(a, b)
        xc = self.and_(x, cin)
        return self.xor(x, cin), self.or_(ab, xc)

    def ripple_add(self, a_bits, b_bits, cin):
        """examples/add_two_numbers.zig:50-73: LSB-first bit wires -> (sum wires, carry)."""
        out, carry = [], cin
        for a, b in zip(a_bits, b_bits):
            s, carry = self.full_adder(a, b, carry)
            out.append(s)
        return out, carry

    def output(self, *wires):
        self.outputs.extend(wires)

    def schedule(self, cus: int = 256, pack: bool = True):
        """The level of every gate as tfhe_gpu_circuit_eval runs it on a device
        with `cus` CUs (host only, tfhe_circuit_schedule) -> (levels, depth)."""
        lib = load_library()
        ops = np.array(self.ops, np.uint8)
        ia, iap = _u32(np.array(self.ia, np.uint32))
        ib, ibp = _u32(np.array(self.ib, np.uint32))
        levels = np.zeros(max(len(self.ops), 1), np.uint32)
        depth = C.c_uint32(0)
        rc = lib.tfhe_circuit_schedule(self.n_inputs, ops.size, ops.ctypes.data_as(u8p), iap, ibp, cus, int(pack),
                                       levels.ctypes.data_as(u32p), C.byref(depth))
        if rc:
            raise TfheError(f"circuit_schedule: status {rc}")
        return levels[:ops.size], depth.value

    def partition(self, num_devices: int):
        """The device of every gate a multi-device context's circuit_eval uses
        (host only, tfhe_circuit_partition)."""
        lib = load_library()
        ops = np.array(self.ops, np.uint8)
        ia, iap = _u32(np.array(self.ia, np.uint32))
        ib, ibp = _u32(np.array(self.ib, np.uint32))
        dev = np.zeros(max(len(self.ops), 1), np.uint32)
        rc = lib.tfhe_circuit_partition(self.n_inputs, ops.size, ops.ctypes.data_as(u8p), iap, ibp, num_devices,
                                        dev.ctypes.data_as(u32p))
        if rc:
            raise TfheError(f"circuit_partition: status {rc}")
        return dev[:ops.size]

    def run(self, ctx: "Context", inputs):
        inputs = np.asarray(inputs, np.uint32).reshape(-1, ctx.params.n + 1)
        if inputs.shape[0] != self.n_inputs:
            raise ValueError(f"circuit has {self.n_inputs} inputs, got {inputs.shape[0]}")
        return ctx.circuit_eval(inputs, np.array(self.ops, np.uint8), np.array(self.ia, np.uint32),
                                np.array(self.ib, np.uint32), np.array(self.outputs, np.uint32))

    def run_dev(self, ctx: "Context", inputs_ptr, outputs_ptr):
        """Inputs (n_inputs TLWELv0) and outputs in HBM; returns the bootstrap depth."""
        return ctx.circuit_eval_dev(inputs_ptr, self.n_inputs, np.array(self.ops, np.uint8),
                                    np.array(self.ia, np.uint32), np.array(self.ib, np.uint32),
                                    np.array(self.outputs, np.uint32), outputs_ptr)
