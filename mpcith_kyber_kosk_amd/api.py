"""ctypes binding of libkosk_mi355x.so -- the host-side mirror of the reference
API (kosk.hpp:18-24) plus the kernel-level entry points used by tests/bench.

There is NO CPU fallback: constructing :class:`Kosk` without a usable HIP device
raises, and importing this module without the built library raises.
"""
import ctypes as C
import os

from . import build as _build

_HERE = os.path.dirname(os.path.abspath(__file__))
# KOSK_LIB_PATH: another build of the same library (A/B measurements of two trees on one GPU box); never a different product
LIB_PATH = os.environ.get("KOSK_LIB_PATH") or os.path.join(_HERE, "libkosk_mi355x.so")


class KoskError(RuntimeError):
    pass


def _load():
    if not os.path.exists(LIB_PATH):
        _build.build()
    lib = C.CDLL(LIB_PATH)
    u8p, u16p, i16p, sz, vp = C.POINTER(C.c_uint8), C.POINTER(C.c_uint16), C.POINTER(C.c_int16), C.c_size_t, C.c_void_p
    sig = {
        "kosk_pk_bytes": (sz, [C.c_int]), "kosk_sk_bytes": (sz, [C.c_int]),
        "kosk_proof_bytes": (sz, [C.c_int]), "kosk_tape_bytes": (sz, [C.c_int]),
        "kosk_proof_field": (C.c_int, [C.c_int, C.c_int, C.POINTER(sz), C.POINTER(sz)]),
        "kosk_create": (C.c_int, [C.POINTER(vp), C.c_int, C.c_int, C.c_int]),
        "kosk_options_init": (None, [vp]),
        "kosk_create_ex": (C.c_int, [C.POINTER(vp), C.c_int, C.c_int, C.c_int, vp]),
        "kosk_destroy": (None, [vp]),
        "kosk_last_error": (C.c_char_p, [vp]),
        "kosk_set_randombytes": (C.c_int, [vp, vp, vp]),
        "kosk_verifiable_keygen_batch": (C.c_int, [vp, C.c_int, vp, sz, vp, vp, vp]),
        "kosk_verify_batch": (C.c_int, [vp, C.c_int, vp, vp, vp]),
        "kosk_verify_fail_masks": (C.c_int, [vp, vp, C.c_int]),
        "kosk_randomness_bytes": (sz, [C.c_int]),
        "kosk_range_proof_bytes": (sz, [C.c_int]),
        "kosk_mlwe_inst_bytes": (sz, [C.c_int]),
        "kosk_prepare_randomness": (C.c_int, [vp, C.c_int, vp, sz, vp]),
        "kosk_prepare_range_proof": (C.c_int, [vp, C.c_int, vp, sz, vp]),
        "kosk_prove_prepared": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, sz, vp]),
        "kosk_verify_inst": (C.c_int, [vp, C.c_int, vp, vp, vp]),
        "kosk_compact_proof_bytes": (sz, [C.c_int]),
        "kosk_proof_compress": (C.c_int, [C.c_int, vp, vp]),
        "kosk_proof_decompress": (C.c_int, [C.c_int, vp, vp]),
        "kosk_fetch_proofs_compact": (C.c_int, [vp, C.c_int, vp]),
        "kosk_verifiable_keygen_batch_compact": (C.c_int, [vp, C.c_int, vp, sz, vp, vp, vp]),
        "kosk_verify_batch_compact": (C.c_int, [vp, C.c_int, vp, vp, vp]),
        "kosk_stage_verifier_inputs_compact": (C.c_int, [vp, C.c_int, vp, vp]),
        "kosk_stage_prover_inputs": (C.c_int, [vp, C.c_int, vp, sz, vp, vp]),
        "kosk_prove_resident": (C.c_int, [vp, C.c_int]),
        "kosk_fetch_proofs": (C.c_int, [vp, C.c_int, vp]),
        "kosk_stage_verifier_inputs": (C.c_int, [vp, C.c_int, vp, vp]),
        "kosk_verify_resident": (C.c_int, [vp, C.c_int, vp]),
        "kosk_verifiable_keygen_resident": (C.c_int, [vp, C.c_int, vp, sz, vp, vp]),
        "kosk_verify_resident_pk": (C.c_int, [vp, C.c_int, vp, vp]),
        "kosk_resident_digests": (C.c_int, [vp, C.c_int, C.POINTER(vp), C.POINTER(sz)]),
        "kosk_set_round_hook": (C.c_int, [vp, vp, vp]),
        "kosk_phase_seconds": (C.c_int, [vp, C.POINTER(C.c_double), C.c_int]),
        "kosk_path_count": (C.c_int, [vp, C.c_int, C.POINTER(C.c_long)]),
        "kosk_host_threads": (C.c_int, [vp]),
        "kosk_host_alloc": (vp, [sz]),
        "kosk_host_free": (None, [vp]),
        "kosk_sha3_256_batch": (C.c_int, [vp, vp, sz, sz, vp, C.c_int]),
        "kosk_shake256_batch": (C.c_int, [vp, vp, sz, sz, vp, sz, C.c_int]),
        "kosk_sha3_256_batch_pair": (C.c_int, [vp, vp, sz, sz, vp, C.c_int]),
        "kosk_sha3_256_batch_wave": (C.c_int, [vp, vp, sz, sz, vp, C.c_int]),
        "kosk_fs_alpha_device": (C.c_int, [vp, vp, sz, C.c_int, vp, vp]),
        "kosk_fs_opened_device": (C.c_int, [vp, vp, sz, C.c_int, vp, vp, C.c_int, vp]),
        "kosk_commit_hash_lanes": (C.c_int, [vp, vp, sz, C.c_int, vp, C.c_int, vp]),
        "kosk_ntt256_batch": (C.c_int, [vp, vp, vp, C.c_int]),
        "kosk_lagrange_expand": (C.c_int, [vp, vp, vp, C.c_int]),
        "kosk_recon_secrets": (C.c_int, [vp, vp, vp, C.c_int, C.c_int]),
        "kosk_profile_enable": (C.c_int, [vp, C.c_int]),
        "kosk_profile_read": (C.c_int, [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_long)]),
        "kosk_profile_read_units": (C.c_int, [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_long), C.POINTER(C.c_long)]),
        "kosk_combine_stats": (C.c_int, [vp, C.POINTER(C.c_long), C.POINTER(C.c_long)]),
        "kosk_stream_timer_start": (C.c_int, [vp]),
        "kosk_stream_timer_stop": (C.c_int, [vp, C.POINTER(C.c_double)]),
        "kosk_device_synchronize": (C.c_int, [vp]),
        "kosk_streams": (C.c_int, [vp]),
        "kosk_resident_proofs": (C.c_int, [vp, C.POINTER(vp), C.POINTER(sz)]),
        "kosk_keygen": (C.c_int, [C.c_int, vp, vp, vp, vp, vp, vp, vp]),
        "kosk_fs_alpha": (C.c_int, [C.c_int, vp, vp]),
        "kosk_fs_opened": (C.c_int, [vp, vp, vp]),
        "kosk_host_sha3_256": (None, [vp, vp, sz]),
        "kosk_host_shake256": (None, [vp, sz, vp, sz]),
        "kosk_host_sha3_256_multi": (C.c_int, [vp, vp, sz, sz, C.c_int, C.c_int]),
        "kosk_lagrange_table": (C.c_int, [C.c_int, vp]),
    }
    # seeded proving (kosk-seedtape-v1)
    seeded = {
        "kosk_tape_from_seed": (C.c_int, [C.c_int, vp, vp]),
        "kosk_set_entropy": (C.c_int, [vp, C.c_int]),
        "kosk_tape_expand_device": (C.c_int, [vp, C.c_int, vp, sz, vp, sz]),
        "kosk_verifiable_keygen_seeded_batch": (C.c_int, [vp, C.c_int, vp, sz, vp, vp, vp]),
        "kosk_verifiable_keygen_seeded_batch_compact": (C.c_int, [vp, C.c_int, vp, sz, vp, vp, vp]),
        "kosk_verifiable_keygen_seeded_resident": (C.c_int, [vp, C.c_int, vp, sz, vp, vp]),
        "kosk_stage_prover_inputs_seeded": (C.c_int, [vp, C.c_int, vp, sz, vp, vp]),
    }
    # an older build named by KOSK_LIB_PATH (the "before" leg of an A/B measurement) has no seeded entry points: its explicit-tape
    # calls must stay usable from this binding.  The tree's own library has to export everything
    if not (os.environ.get("KOSK_LIB_PATH") and not hasattr(lib, "kosk_tape_from_seed")):
        sig.update(seeded)
    # Kyber KEM; optional under the same rule (and only then)
    kem = {
        "kosk_ct_bytes": (sz, [C.c_int]),
        "kosk_kem_enc_batch": (C.c_int, [vp, C.c_int, vp, vp, vp, vp]),
        "kosk_kem_dec_batch": (C.c_int, [vp, C.c_int, vp, vp, vp]),
        "kosk_kem_enc_verified": (C.c_int, [vp, C.c_int, vp, vp, vp, vp]),
    }
    if not (os.environ.get("KOSK_LIB_PATH") and not hasattr(lib, "kosk_kem_enc_batch")):
        sig.update(kem)
    # proofs for existing keys; optional under the same rule (and only then)
    keyproof = {
        "kosk_witness_from_sk": (C.c_int, [vp, C.c_int, vp, vp, vp]),
        "kosk_stage_prover_keys": (C.c_int, [vp, C.c_int, vp, vp, sz, vp]),
        "kosk_stage_prover_keys_seeded": (C.c_int, [vp, C.c_int, vp, vp, sz, vp]),
        "kosk_prove_keys_batch": (C.c_int, [vp, C.c_int, vp, vp, sz, vp, vp]),
        "kosk_prove_keys_seeded_batch": (C.c_int, [vp, C.c_int, vp, vp, sz, vp, vp]),
    }
    if not (os.environ.get("KOSK_LIB_PATH") and not hasattr(lib, "kosk_witness_from_sk")):
        sig.update(keyproof)
    # context-bound proofs (kosk-bind-v1); optional under the same rule (and only then)
    bound = {
        "kosk_bind_value": (C.c_int, [C.c_int, vp, vp, vp]),
        "kosk_bind_device": (C.c_int, [vp, C.c_int, vp, vp, sz, vp]),
        "kosk_fs_alpha_bound": (C.c_int, [C.c_int, vp, vp, vp]),
        "kosk_fs_opened_bound": (C.c_int, [vp, vp, vp, vp]),
        "kosk_fs_alpha_bound_device": (C.c_int, [vp, vp, sz, C.c_int, vp, vp, vp]),
        "kosk_fs_opened_bound_device": (C.c_int, [vp, vp, sz, C.c_int, vp, vp, vp, C.c_int, vp]),
        "kosk_set_contexts": (C.c_int, [vp, C.c_int, vp, sz]),
    }
    if not (os.environ.get("KOSK_LIB_PATH") and not hasattr(lib, "kosk_set_contexts")):
        sig.update(bound)
    # dense wire format (kosk-dense-v1); optional under the same rule (and only then)
    dense = {
        "kosk_dense_proof_bytes": (sz, [C.c_int]),
        "kosk_proof_dense_pack": (C.c_int, [C.c_int, vp, vp]),
        "kosk_proof_dense_unpack": (C.c_int, [C.c_int, vp, vp]),
        "kosk_fetch_proofs_dense": (C.c_int, [vp, C.c_int, vp]),
        "kosk_stage_verifier_inputs_dense": (C.c_int, [vp, C.c_int, vp, vp]),
        "kosk_verifiable_keygen_batch_dense": (C.c_int, [vp, C.c_int, vp, sz, vp, vp, vp]),
        "kosk_verifiable_keygen_seeded_batch_dense": (C.c_int, [vp, C.c_int, vp, sz, vp, vp, vp]),
        "kosk_verify_batch_dense": (C.c_int, [vp, C.c_int, vp, vp, vp]),
        "kosk_dense_fill_device": (C.c_int, [vp, C.c_int, vp, sz, vp]),
    }
    if not (os.environ.get("KOSK_LIB_PATH") and not hasattr(lib, "kosk_dense_proof_bytes")):
        sig.update(dense)
    # KEM key pairs and key checks; optional under the same rule (and only then)
    keypair = {
        "kosk_kem_keypair_batch": (C.c_int, [vp, C.c_int, vp, vp, vp]),
        "kosk_kem_check_pk": (C.c_int, [vp, C.c_int, vp, vp]),
        "kosk_kem_check_sk": (C.c_int, [vp, C.c_int, vp, vp]),
    }
    if not (os.environ.get("KOSK_LIB_PATH") and not hasattr(lib, "kosk_kem_keypair_batch")):
        sig.update(keypair)
    # randomness derived from the key (kosk-keyseed-v1); optional under the same rule (and only then)
    keyseed = {
        "kosk_keyseed_value": (C.c_int, [C.c_int, vp, vp, vp, vp]),
        "kosk_keyseed_device": (C.c_int, [vp, C.c_int, vp, vp, sz, vp, sz, vp]),
        "kosk_stage_prover_keys_derived": (C.c_int, [vp, C.c_int, vp, vp, sz, vp]),
        "kosk_prove_keys_derived_batch": (C.c_int, [vp, C.c_int, vp, vp, sz, vp, vp]),
    }
    if not (os.environ.get("KOSK_LIB_PATH") and not hasattr(lib, "kosk_keyseed_value")):
        sig.update(keyseed)
    # erasing secrets and the audit scan; optional under the same rule (and only then)
    wipe = {
        "kosk_wipe_secrets": (C.c_int, [vp]),
        "kosk_set_wipe": (C.c_int, [vp, C.c_int]),
        "kosk_secret_scan": (C.c_int, [vp, vp, sz, C.POINTER(C.c_long)]),
        "kosk_wipe_device": (C.c_int, [vp, C.c_int, vp, vp]),
        "kosk_wipe_timing": (C.c_int, [vp, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    }
    if not (os.environ.get("KOSK_LIB_PATH") and not hasattr(lib, "kosk_wipe_secrets")):
        sig.update(wipe)
    # KEM with one resident key; optional under the same rule (and only then)
    onekey = {
        "kosk_kem_key_set": (C.c_int, [vp, vp, vp]),
        "kosk_kem_key_state": (C.c_int, [vp]),
        "kosk_kem_key_clear": (C.c_int, [vp]),
        "kosk_kem_enc_key": (C.c_int, [vp, C.c_int, vp, vp, vp]),
        "kosk_kem_dec_key": (C.c_int, [vp, C.c_int, vp, vp]),
    }
    if not (os.environ.get("KOSK_LIB_PATH") and not hasattr(lib, "kosk_kem_key_set")):
        sig.update(onekey)
    # tests: the prover at forced opened lists; optional under the same rule (and only then)
    forced = {
        "kosk_force_opened_candidates": (C.c_int, [vp, C.c_int, vp]),
        "kosk_opened_tables": (C.c_int, [vp, vp, vp, C.c_int]),
    }
    if not (os.environ.get("KOSK_LIB_PATH") and not hasattr(lib, "kosk_opened_tables")):
        sig.update(forced)
    # transcoding between the wire formats; optional under the same rule (and only then)
    transcode = {
        "kosk_format_bytes": (sz, [C.c_int, C.c_int]),
        "kosk_transcode_batch": (C.c_int, [vp, C.c_int, C.c_int, vp, C.c_int, vp, vp]),
        "kosk_dense_check_device": (C.c_int, [vp, C.c_int, vp, sz, vp]),
    }
    if not (os.environ.get("KOSK_LIB_PATH") and not hasattr(lib, "kosk_transcode_batch")):
        sig.update(transcode)
    # dense wire format kosk-dense-v2 and the calls that take the packed format as an argument; optional under the same rule (and only then)
    dense2 = {
        "kosk_dense2_proof_bytes": (sz, [C.c_int]),
        "kosk_proof_dense2_pack": (C.c_int, [C.c_int, vp, vp]),
        "kosk_proof_dense2_unpack": (C.c_int, [C.c_int, vp, vp]),
        "kosk_dense2_fill_device": (C.c_int, [vp, C.c_int, vp, sz, vp]),
        "kosk_dense2_check_device": (C.c_int, [vp, C.c_int, vp, sz, vp]),
        "kosk_verifiable_keygen_batch_fmt": (C.c_int, [vp, C.c_int, C.c_int, vp, sz, vp, vp, vp]),
        "kosk_verifiable_keygen_seeded_batch_fmt": (C.c_int, [vp, C.c_int, C.c_int, vp, sz, vp, vp, vp]),
        "kosk_verify_batch_fmt": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, vp]),
        "kosk_fetch_proofs_fmt": (C.c_int, [vp, C.c_int, C.c_int, vp]),
        "kosk_stage_verifier_inputs_fmt": (C.c_int, [vp, C.c_int, C.c_int, vp, vp]),
    }
    if not (os.environ.get("KOSK_LIB_PATH") and not hasattr(lib, "kosk_dense2_proof_bytes")):
        sig.update(dense2)
    # the offline bank; optional under the same rule (and only then)
    bank = {
        "kosk_bank_entry_bytes": (sz, [C.c_int]),
        "kosk_tape_section": (C.c_int, [C.c_int, C.c_int, C.POINTER(sz), C.POINTER(sz)]),
        "kosk_bank_reserve": (C.c_int, [vp, C.c_int]),
        "kosk_bank_level": (C.c_int, [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
        "kosk_bank_fill": (C.c_int, [vp, C.c_int, vp, sz, vp, sz]),
        "kosk_stage_prover_keys_banked": (C.c_int, [vp, C.c_int, vp, vp, sz, vp, sz, vp]),
        "kosk_prove_keys_banked_batch": (C.c_int, [vp, C.c_int, vp, vp, sz, vp, sz, vp, vp]),
        "kosk_verifiable_keygen_banked_batch": (C.c_int, [vp, C.c_int, vp, sz, vp, sz, vp, vp, vp]),
        "kosk_bank_timing": (C.c_int, [vp, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                       C.POINTER(sz)]),
    }
    if not (os.environ.get("KOSK_LIB_PATH") and not hasattr(lib, "kosk_bank_reserve")):
        sig.update(bank)
    # the verified-key registry; optional under the same rule (and only then)
    ip = C.POINTER(C.c_int)
    registry = {
        "kosk_registry_slot_bytes": (sz, [C.c_int]),
        "kosk_registry_reserve": (C.c_int, [vp, C.c_int]),
        "kosk_registry_level": (C.c_int, [vp, ip, ip]),
        "kosk_registry_admit_verified": (C.c_int, [vp, C.c_int, vp, vp]),
        "kosk_registry_admit": (C.c_int, [vp, C.c_int, vp, vp, vp]),
        "kosk_registry_evict": (C.c_int, [vp, C.c_int, vp]),
        "kosk_registry_read": (C.c_int, [vp, C.c_int, vp, vp, vp, vp]),
        "kosk_kem_enc_slots": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, vp]),
    }
    if not (os.environ.get("KOSK_LIB_PATH") and not hasattr(lib, "kosk_registry_reserve")):
        sig.update(registry)
    # the registry by fingerprint; optional under the same rule (and only then)
    peers = {
        "kosk_registry_index_entries": (sz, [C.c_int]),
        "kosk_registry_index_home": (C.c_int, [C.c_int, vp]),
        "kosk_registry_find": (C.c_int, [vp, C.c_int, vp, vp]),
        "kosk_registry_enrol_verified": (C.c_int, [vp, C.c_int, vp, vp]),
        "kosk_registry_enrol": (C.c_int, [vp, C.c_int, vp, vp, vp, vp]),
        "kosk_kem_enc_peers": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, vp]),
    }
    if not (os.environ.get("KOSK_LIB_PATH") and not hasattr(lib, "kosk_registry_find")):
        sig.update(peers)
    # the registry tree, kosk-regtree-v1; optional under the same rule (and only then)
    tree = {
        "kosk_registry_tree_depth": (C.c_int, [C.c_int]),
        "kosk_registry_tree_bytes": (sz, [C.c_int]),
        "kosk_regtree_leaf": (C.c_int, [C.c_int, vp, vp]),
        "kosk_regtree_node": (C.c_int, [vp, vp, vp]),
        "kosk_regtree_root_from_path": (C.c_int, [C.c_int, C.c_int, C.c_int32, vp, vp, vp]),
        "kosk_registry_root": (C.c_int, [vp, vp, ip, ip]),
        "kosk_registry_prove_slots": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, vp]),
        "kosk_registry_prove_peers": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, vp]),
    }
    if not (os.environ.get("KOSK_LIB_PATH") and not hasattr(lib, "kosk_registry_root")):
        sig.update(tree)
    # the sorted tree, kosk-regsort-v1; optional under the same rule (and only then)
    sorted_tree = {
        "kosk_regsort_proof_bytes": (sz, [C.c_int]),
        "kosk_regsort_leaf": (C.c_int, [C.c_int, vp, C.c_int32, vp]),
        "kosk_regsort_node": (C.c_int, [vp, vp, vp]),
        "kosk_regsort_root_from_path": (C.c_int, [C.c_int, C.c_int, C.c_int32, vp, C.c_int32, vp, vp]),
        "kosk_regsort_check_proof": (C.c_int, [C.c_int, C.c_int, vp, vp, vp]),
        "kosk_registry_sorted_root": (C.c_int, [vp, vp, ip, ip]),
        "kosk_registry_prove_absent": (C.c_int, [vp, C.c_int, vp, vp, vp, vp]),
        "kosk_regsort_order_device": (C.c_int, [vp, C.c_int, vp, vp, vp]),
    }
    if not (os.environ.get("KOSK_LIB_PATH") and not hasattr(lib, "kosk_registry_sorted_root")):
        sig.update(sorted_tree)
    # the registry history, kosk-reghist-v1; optional under the same rule (and only then)
    history = {
        "kosk_reghist_depth": (C.c_int, [C.c_int]),
        "kosk_reghist_path_bytes": (sz, [C.c_int]),
        "kosk_reghist_consistency_bytes": (sz, [C.c_int]),
        "kosk_reghist_leaf": (C.c_int, [C.c_int, vp, vp]),
        "kosk_reghist_node": (C.c_int, [vp, vp, vp]),
        "kosk_reghist_empty_root": (C.c_int, [C.c_int, vp]),
        "kosk_reghist_root_from_path": (C.c_int, [C.c_int, C.c_int, vp, vp, vp]),
        "kosk_reghist_check_consistency": (C.c_int, [C.c_int, C.c_int, vp, vp, vp]),
        "kosk_registry_history_reserve": (C.c_int, [vp, C.c_int]),
        "kosk_registry_history_level": (C.c_int, [vp, ip, ip]),
        "kosk_registry_history_head": (C.c_int, [vp, C.c_int, vp, ip]),
        "kosk_registry_history_checkpoint": (C.c_int, [vp, ip]),
        "kosk_registry_history_read": (C.c_int, [vp, C.c_int, C.c_int, vp]),
        "kosk_registry_history_prove_events": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, vp, vp]),
        "kosk_registry_history_prove_consistency": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, vp]),
    }
    if not (os.environ.get("KOSK_LIB_PATH") and not hasattr(lib, "kosk_registry_history_reserve")):
        sig.update(history)
    # the registry monitor; optional under the same rule (and only then)
    monitor = {
        "kosk_monitor_reserve": (C.c_int, [vp, C.c_int, C.c_int]),
        "kosk_monitor_level": (C.c_int, [vp, ip, ip, ip, ip, ip]),
        "kosk_monitor_feed": (C.c_int, [vp, C.c_int, vp, ip, ip]),
        "kosk_monitor_head": (C.c_int, [vp, C.c_int, vp, ip]),
        "kosk_monitor_roots": (C.c_int, [vp, vp, vp]),
        "kosk_monitor_read": (C.c_int, [vp, C.c_int, vp, vp, vp]),
    }
    if not (os.environ.get("KOSK_LIB_PATH") and not hasattr(lib, "kosk_monitor_reserve")):
        sig.update(monitor)
    # the relying party; optional under the same rule (and only then)
    relying = {
        "kosk_regtree_check_paths": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp]),
        "kosk_regsort_check_proofs": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, vp, vp]),
        "kosk_kem_enc_proven": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp, vp]),
    }
    if not (os.environ.get("KOSK_LIB_PATH") and not hasattr(lib, "kosk_regtree_check_paths")):
        sig.update(relying)
    # signed heads, kosk-headsig-v1; optional under the same rule (and only then)
    headsig = {
        "kosk_headsig_sig_bytes": (sz, [C.c_int]),
        "kosk_headsig_statement": (C.c_int, [C.c_int, vp, C.c_int, vp]),
        "kosk_headsig_verify": (C.c_int, [vp, C.c_int, vp, C.c_int, vp]),
        "kosk_headsig_public_from_seed": (C.c_int, [C.c_int, vp, vp, vp]),
        "kosk_registry_signer_reserve": (C.c_int, [vp, C.c_int, vp, vp, vp]),
        "kosk_registry_signer_level": (C.c_int, [vp, ip, ip]),
        "kosk_registry_history_sign_head": (C.c_int, [vp, C.c_int, vp, vp, ip]),
        "kosk_headsig_verify_heads": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, vp]),
    }
    if not (os.environ.get("KOSK_LIB_PATH") and not hasattr(lib, "kosk_headsig_verify")):
        sig.update(headsig)
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)  # AttributeError if the header and the library ever disagree
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()
EXPORTS = ["kosk_pk_bytes", "kosk_sk_bytes", "kosk_proof_bytes", "kosk_tape_bytes", "kosk_proof_field", "kosk_create",
           "kosk_destroy", "kosk_last_error", "kosk_set_randombytes", "kosk_verifiable_keygen_batch", "kosk_verify_batch",
           "kosk_verify_fail_masks", "kosk_randomness_bytes", "kosk_range_proof_bytes", "kosk_mlwe_inst_bytes",
           "kosk_prepare_randomness", "kosk_prepare_range_proof", "kosk_prove_prepared", "kosk_verify_inst", "kosk_compact_proof_bytes",
           "kosk_proof_compress", "kosk_proof_decompress", "kosk_fetch_proofs_compact", "kosk_stage_verifier_inputs_compact", "kosk_stage_prover_inputs", "kosk_prove_resident", "kosk_fetch_proofs",
           "kosk_stage_verifier_inputs", "kosk_verify_resident", "kosk_verifiable_keygen_resident", "kosk_verify_resident_pk",
           "kosk_resident_digests", "kosk_set_round_hook", "kosk_phase_seconds", "kosk_path_count", "kosk_host_threads", "kosk_sha3_256_batch_pair", "kosk_verifiable_keygen_batch_compact", "kosk_verify_batch_compact", "kosk_host_alloc", "kosk_host_free", "kosk_sha3_256_batch",
           "kosk_shake256_batch", "kosk_commit_hash_lanes", "kosk_ntt256_batch", "kosk_lagrange_expand",
           "kosk_recon_secrets", "kosk_profile_enable", "kosk_profile_read", "kosk_profile_read_units", "kosk_combine_stats", "kosk_stream_timer_start", "kosk_stream_timer_stop", "kosk_device_synchronize", "kosk_streams", "kosk_resident_proofs", "kosk_keygen", "kosk_fs_alpha",
           "kosk_fs_opened", "kosk_host_sha3_256", "kosk_host_shake256", "kosk_host_sha3_256_multi", "kosk_lagrange_table",
           "kosk_options_init", "kosk_create_ex", "kosk_sha3_256_batch_wave", "kosk_fs_alpha_device", "kosk_fs_opened_device",
           "kosk_tape_from_seed", "kosk_set_entropy", "kosk_tape_expand_device", "kosk_verifiable_keygen_seeded_batch",
           "kosk_verifiable_keygen_seeded_batch_compact", "kosk_verifiable_keygen_seeded_resident", "kosk_stage_prover_inputs_seeded",
           "kosk_ct_bytes", "kosk_kem_enc_batch", "kosk_kem_dec_batch", "kosk_kem_enc_verified",
           "kosk_witness_from_sk", "kosk_stage_prover_keys", "kosk_stage_prover_keys_seeded", "kosk_prove_keys_batch",
           "kosk_prove_keys_seeded_batch",
           "kosk_bind_value", "kosk_bind_device", "kosk_fs_alpha_bound", "kosk_fs_opened_bound", "kosk_fs_alpha_bound_device",
           "kosk_fs_opened_bound_device", "kosk_set_contexts",
           "kosk_dense_proof_bytes", "kosk_proof_dense_pack", "kosk_proof_dense_unpack", "kosk_fetch_proofs_dense",
           "kosk_stage_verifier_inputs_dense", "kosk_verifiable_keygen_batch_dense", "kosk_verifiable_keygen_seeded_batch_dense",
           "kosk_verify_batch_dense", "kosk_dense_fill_device",
           "kosk_kem_keypair_batch", "kosk_kem_check_pk", "kosk_kem_check_sk",
           "kosk_keyseed_value", "kosk_keyseed_device", "kosk_stage_prover_keys_derived", "kosk_prove_keys_derived_batch",
           "kosk_wipe_secrets", "kosk_set_wipe", "kosk_secret_scan", "kosk_wipe_device", "kosk_wipe_timing",
           "kosk_kem_key_set", "kosk_kem_key_state", "kosk_kem_key_clear", "kosk_kem_enc_key", "kosk_kem_dec_key",
           "kosk_force_opened_candidates", "kosk_opened_tables",
           "kosk_format_bytes", "kosk_transcode_batch", "kosk_dense_check_device",
           "kosk_dense2_proof_bytes", "kosk_proof_dense2_pack", "kosk_proof_dense2_unpack", "kosk_dense2_fill_device", "kosk_dense2_check_device",
           "kosk_verifiable_keygen_batch_fmt", "kosk_verifiable_keygen_seeded_batch_fmt", "kosk_verify_batch_fmt", "kosk_fetch_proofs_fmt",
           "kosk_stage_verifier_inputs_fmt",
           "kosk_bank_entry_bytes", "kosk_tape_section", "kosk_bank_reserve", "kosk_bank_level", "kosk_bank_fill", "kosk_stage_prover_keys_banked",
           "kosk_prove_keys_banked_batch", "kosk_verifiable_keygen_banked_batch", "kosk_bank_timing",
           "kosk_registry_slot_bytes", "kosk_registry_reserve", "kosk_registry_level", "kosk_registry_admit_verified", "kosk_registry_admit",
           "kosk_registry_evict", "kosk_registry_read", "kosk_kem_enc_slots",
           "kosk_registry_index_entries", "kosk_registry_index_home", "kosk_registry_find", "kosk_registry_enrol_verified",
           "kosk_registry_enrol", "kosk_kem_enc_peers",
           "kosk_registry_tree_depth", "kosk_registry_tree_bytes", "kosk_regtree_leaf", "kosk_regtree_node", "kosk_regtree_root_from_path",
           "kosk_registry_root", "kosk_registry_prove_slots", "kosk_registry_prove_peers",
           "kosk_regsort_proof_bytes", "kosk_regsort_leaf", "kosk_regsort_node", "kosk_regsort_root_from_path", "kosk_regsort_check_proof",
           "kosk_registry_sorted_root", "kosk_registry_prove_absent", "kosk_regsort_order_device",
           "kosk_reghist_depth", "kosk_reghist_path_bytes", "kosk_reghist_consistency_bytes", "kosk_reghist_leaf", "kosk_reghist_node",
           "kosk_reghist_empty_root", "kosk_reghist_root_from_path", "kosk_reghist_check_consistency",
           "kosk_registry_history_reserve", "kosk_registry_history_level", "kosk_registry_history_head", "kosk_registry_history_checkpoint",
           "kosk_registry_history_read", "kosk_registry_history_prove_events", "kosk_registry_history_prove_consistency",
           "kosk_monitor_reserve", "kosk_monitor_level", "kosk_monitor_feed", "kosk_monitor_head", "kosk_monitor_roots", "kosk_monitor_read",
           "kosk_regtree_check_paths", "kosk_regsort_check_proofs", "kosk_kem_enc_proven",
           "kosk_headsig_sig_bytes", "kosk_headsig_statement", "kosk_headsig_verify", "kosk_headsig_public_from_seed",
           "kosk_registry_signer_reserve", "kosk_registry_signer_level", "kosk_registry_history_sign_head", "kosk_headsig_verify_heads"]
HAS_KEM = hasattr(lib, "kosk_kem_enc_batch")  # False only for an older library named by KOSK_LIB_PATH


class KoskOptions(C.Structure):
    """kosk_options of include/kosk_mi355x.h (per-handle configuration, round 6); build with options(**fields)"""
    _fields_ = [("size", C.c_uint32), ("streams", C.c_int32), ("combine", C.c_int32), ("combine_wait_us", C.c_int32),
                ("combine_idle_us", C.c_int32), ("combine_prewake_us", C.c_int32), ("strict_encoding", C.c_int32), ("fs_mode", C.c_int32),
                ("host_threads", C.c_int32), ("blocking_sync", C.c_int32), ("hooks_unmerged", C.c_int32), ("reserved", C.c_int32 * 6)]


FS_HOST, FS_DEVICE = 0, 1
ENTROPY_TAPE, ENTROPY_SEED = 0, 1  # kosk_set_entropy
WIPE_OFF, WIPE_CALL = 0, 1  # kosk_set_wipe
SEED_BYTES = 32
SS_BYTES = 32  # KOSK_SS_BYTES
KEYPAIR_COIN_BYTES = 64  # d || z of crypto_kem_keypair_derand
KEYCHK_HASH, KEYCHK_PK_RANGE, KEYCHK_S_RANGE = 1, 2, 4  # KOSK_KEYCHK_*
KEM_KEY_NONE, KEM_KEY_PK, KEM_KEY_SK = 0, 1, 2  # KOSK_KEM_KEY_*
FMT_IMAGE, FMT_COMPACT, FMT_DENSE = 0, 1, 2  # KOSK_FMT_*
FMT_DENSE2 = 4  # KOSK_FMT_DENSE2 (kosk-dense-v2); 3 is not a format


def options(**fields):
    o = KoskOptions()
    lib.kosk_options_init(C.byref(o))
    for k_, v_ in fields.items():
        if k_ not in dict(KoskOptions._fields_) or k_ in ("size", "reserved"):
            raise KoskError("unknown option " + k_)
        setattr(o, k_, int(v_))
    return o


def pk_bytes(k): return lib.kosk_pk_bytes(k)
def sk_bytes(k): return lib.kosk_sk_bytes(k)
def proof_bytes(k): return lib.kosk_proof_bytes(k)
def tape_bytes(k): return lib.kosk_tape_bytes(k)
def ct_bytes(k): return lib.kosk_ct_bytes(k)
def dense_proof_bytes(k): return lib.kosk_dense_proof_bytes(k)
def dense2_proof_bytes(k): return lib.kosk_dense2_proof_bytes(k)
def format_bytes(k, fmt): return lib.kosk_format_bytes(k, fmt)
def bank_entry_bytes(k): return lib.kosk_bank_entry_bytes(k)
def registry_slot_bytes(k): return lib.kosk_registry_slot_bytes(k)
def registry_index_entries(capacity): return lib.kosk_registry_index_entries(capacity)


ENROL_REJECTED, ENROL_ADMITTED, ENROL_DUPLICATE = 0, 1, 2  # KOSK_ENROL_*


def registry_index_home(capacity, h):
    """kosk_registry_index_home: the home entry of fingerprint h (32 bytes) in the index of a registry of `capacity` slots; -1 for capacity < 1"""
    h = bytes(h)
    if len(h) != 32:
        raise KoskError("a fingerprint has 32 bytes")
    return lib.kosk_registry_index_home(capacity, C.c_char_p(h))


# the registry tree, kosk-regtree-v1: the host functions, no handle and no GPU
REGTREE_TIER_LEVELS = 10  # KOSK_REGTREE_TIER_LEVELS


def registry_tree_depth(capacity): return lib.kosk_registry_tree_depth(capacity)
def registry_tree_bytes(capacity): return lib.kosk_registry_tree_bytes(capacity)


def _digest(what, b):
    b = bytes(b)
    if len(b) != 32:
        raise KoskError("%s has 32 bytes" % what)
    return b


def regtree_leaf(k, h=None):
    """kosk_regtree_leaf: the leaf of an occupied slot whose stored fingerprint is h, or (h None) of an empty slot"""
    out = C.create_string_buffer(32)
    if lib.kosk_regtree_leaf(k, None if h is None else C.c_char_p(_digest("a fingerprint", h)), out):
        raise KoskError("regtree_leaf: kyber_k outside 2..4")
    return out.raw


def regtree_node(left, right):
    """kosk_regtree_node: the inner node over two 32-byte children"""
    out = C.create_string_buffer(32)
    if lib.kosk_regtree_node(C.c_char_p(_digest("a node", left)), C.c_char_p(_digest("a node", right)), out):
        raise KoskError("regtree_node failed")
    return out.raw


def regtree_root_from_path(k, depth, slot, h, path):
    """kosk_regtree_root_from_path: the root that slot, its fingerprint h (None: the slot is empty) and path (depth x 32 bytes, or a list
    of depth 32-byte records) imply; compare it with the published root"""
    if not isinstance(path, (bytes, bytearray)):
        path = b"".join(path)
    path = bytes(path)
    if depth < 0 or len(path) != 32 * depth:
        raise KoskError("a path of depth %d has %d bytes" % (depth, 32 * max(depth, 0)))
    out = C.create_string_buffer(32)
    if lib.kosk_regtree_root_from_path(k, depth, slot, None if h is None else C.c_char_p(_digest("a fingerprint", h)),
                                       C.c_char_p(path) if depth else None, out):
        raise KoskError("regtree_root_from_path: bad kyber_k, depth or slot")
    return out.raw


# the sorted tree, kosk-regsort-v1: the host functions, no handle and no GPU
REGSORT_NEITHER, REGSORT_ABSENT, REGSORT_PRESENT = 0, 1, 2  # kosk_regsort_check_proof


def regsort_proof_bytes(depth): return lib.kosk_regsort_proof_bytes(depth)


def regsort_leaf(k, h=None, slot=0):
    """kosk_regsort_leaf: the key leaf S(h, slot), or (h None) the padding leaf Z"""
    out = C.create_string_buffer(32)
    if lib.kosk_regsort_leaf(k, None if h is None else C.c_char_p(_digest("a fingerprint", h)), slot, out):
        raise KoskError("regsort_leaf: kyber_k outside 2..4, or a key leaf with slot < 0")
    return out.raw


def regsort_node(left, right):
    """kosk_regsort_node: the inner node over two 32-byte children"""
    out = C.create_string_buffer(32)
    if lib.kosk_regsort_node(C.c_char_p(_digest("a node", left)), C.c_char_p(_digest("a node", right)), out):
        raise KoskError("regsort_node failed")
    return out.raw


def regsort_root_from_path(k, depth, pos, h, slot, path):
    """kosk_regsort_root_from_path: the root that position pos, its entry (h, slot) (h None: padding) and path (depth x 32 bytes, or a list
    of depth 32-byte records) imply"""
    if not isinstance(path, (bytes, bytearray)):
        path = b"".join(path)
    path = bytes(path)
    if depth < 0 or len(path) != 32 * depth:
        raise KoskError("a path of depth %d has %d bytes" % (depth, 32 * max(depth, 0)))
    out = C.create_string_buffer(32)
    if lib.kosk_regsort_root_from_path(k, depth, pos, None if h is None else C.c_char_p(_digest("a fingerprint", h)), slot,
                                       C.c_char_p(path) if depth else None, out):
        raise KoskError("regsort_root_from_path: bad kyber_k, depth, position or slot")
    return out.raw


def regsort_check_proof(k, depth, x, record, root):
    """kosk_regsort_check_proof: what record proves about fingerprint x under root -- REGSORT_PRESENT, REGSORT_ABSENT or REGSORT_NEITHER"""
    record = bytes(record)
    if depth < 0 or depth > 31 or len(record) != regsort_proof_bytes(depth):
        raise KoskError("a proof record of depth %d has %d bytes" % (depth, regsort_proof_bytes(depth) if 0 <= depth <= 31 else 0))
    rc = lib.kosk_regsort_check_proof(k, depth, C.c_char_p(_digest("a fingerprint", x)), C.c_char_p(record), C.c_char_p(_digest("a root", root)))
    if rc < 0:
        raise KoskError("regsort_check_proof: bad kyber_k or depth")
    return rc


# the registry history, kosk-reghist-v1: the host functions, no handle and no GPU
REGHIST_ADMIT, REGHIST_EVICT, REGHIST_CHECKPOINT = 1, 2, 3  # KOSK_REGHIST_*
REGHIST_EVENT_BYTES = 80  # KOSK_REGHIST_EVENT_BYTES
REGHIST_TIER_LEVELS = 10  # KOSK_REGHIST_TIER_LEVELS
# KOSK_MONITOR_*: why kosk_monitor_feed rejected a log
MONITOR_OK, MONITOR_BAD_RECORD, MONITOR_BAD_SLOT, MONITOR_ADMIT_OCCUPIED, MONITOR_EVICT_EMPTY = 0, 1, 2, 3, 4
MONITOR_EVICT_MISMATCH, MONITOR_CP_USED, MONITOR_CP_CAPACITY, MONITOR_CP_SLOT_ROOT, MONITOR_CP_SORTED_ROOT = 5, 6, 7, 8, 9


def reghist_depth(size): return lib.kosk_reghist_depth(size)
def reghist_path_bytes(size): return lib.kosk_reghist_path_bytes(size)
def reghist_consistency_bytes(size): return lib.kosk_reghist_consistency_bytes(size)


def reghist_event(op, a, b=0, x=bytes(32), y=bytes(32)):
    """the 80-byte stored event record: ops 1 / 2 (a = slot, x = the fingerprint), op 3 (a = used, b = capacity, x / y = the two roots)"""
    import struct
    return struct.pack("<4I", op, a, b, 0) + _digest("x", x) + _digest("y", y)


def reghist_leaf(k, event):
    """kosk_reghist_leaf: the leaf hash of a stored event record (80 bytes)"""
    event = bytes(event)
    if len(event) != REGHIST_EVENT_BYTES:
        raise KoskError("an event record has %d bytes" % REGHIST_EVENT_BYTES)
    out = C.create_string_buffer(32)
    if lib.kosk_reghist_leaf(k, C.c_char_p(event), out):
        raise KoskError("reghist_leaf: kyber_k outside 2..4, op outside 1..3 or a non-zero reserved field")
    return out.raw


def reghist_node(left, right):
    """kosk_reghist_node: the inner node over two 32-byte children"""
    out = C.create_string_buffer(32)
    if lib.kosk_reghist_node(C.c_char_p(_digest("a node", left)), C.c_char_p(_digest("a node", right)), out):
        raise KoskError("reghist_node failed")
    return out.raw


def reghist_empty_root(k):
    """kosk_reghist_empty_root: O, the root of the history without events"""
    out = C.create_string_buffer(32)
    if lib.kosk_reghist_empty_root(k, out):
        raise KoskError("reghist_empty_root: kyber_k outside 2..4")
    return out.raw


def reghist_root_from_path(index, size, leaf, record):
    """kosk_reghist_root_from_path: the root that leaf `index` of a history of `size` events and its inclusion record imply, or None where
    the record is malformed; compare it with the published head"""
    record = bytes(record)
    if len(record) != reghist_path_bytes(size):
        raise KoskError("an inclusion record at size %d has %d bytes" % (size, reghist_path_bytes(size)))
    out = C.create_string_buffer(32)
    if lib.kosk_reghist_root_from_path(index, size, C.c_char_p(_digest("a leaf", leaf)), C.c_char_p(record), out):
        return None
    return out.raw


def reghist_check_consistency(old_size, size, root_old, root_new, record):
    """kosk_reghist_check_consistency: True iff record shows that the history of `size` events under root_new extends the one of old_size
    events under root_old"""
    record = bytes(record)
    if len(record) != reghist_consistency_bytes(size):
        raise KoskError("a consistency record at size %d has %d bytes" % (size, reghist_consistency_bytes(size)))
    rc = lib.kosk_reghist_check_consistency(old_size, size, None if root_old is None else C.c_char_p(_digest("a root", root_old)),
                                            C.c_char_p(_digest("a root", root_new)), C.c_char_p(record))
    if rc < 0:
        raise KoskError("reghist_check_consistency: a negative size, old_size > size or size < 1")
    return bool(rc)


HEADSIG_PUB_BYTES = 52  # KOSK_HEADSIG_PUB_BYTES
HEADSIG_ITEMS_PER_BLOCK = 7  # KOSK_HEADSIG_ITEMS_PER_BLOCK


def headsig_sig_bytes(height):
    """kosk_headsig_sig_bytes: 1136 + 32 height, 0 for a height outside 1..24"""
    return lib.kosk_headsig_sig_bytes(height)


def headsig_statement(k, root, size):
    """kosk_headsig_statement: the 56 bytes a head signature signs"""
    out = C.create_string_buffer(56)
    if lib.kosk_headsig_statement(k, C.c_char_p(_digest("a root", root)), size, out):
        raise KoskError("headsig_statement: kyber_k outside 2..4 or size < 0")
    return out.raw


def _headsig_height(pub):
    pub = bytes(pub)
    if len(pub) != HEADSIG_PUB_BYTES:
        raise KoskError("a head-signature public key has %d bytes" % HEADSIG_PUB_BYTES)
    return pub, int.from_bytes(pub[:4], "little")


def headsig_verify(pub, k, root, size, sig):
    """kosk_headsig_verify: True iff sig is the signature of the head (root, size) of a Kyber-k registry under pub"""
    pub, h = _headsig_height(pub)
    sig = bytes(sig)
    if not headsig_sig_bytes(h) or len(sig) != headsig_sig_bytes(h):
        raise KoskError("a signature under this public key has %d bytes" % headsig_sig_bytes(h))
    rc = lib.kosk_headsig_verify(C.c_char_p(pub), k, C.c_char_p(_digest("a root", root)), size, C.c_char_p(sig))
    if rc < 0:
        raise KoskError("headsig_verify: kyber_k outside 2..4, size < 0 or a height outside 1..24")
    return bool(rc)


def headsig_public_from_seed(height, seed, key_id):
    """kosk_headsig_public_from_seed: the public key of (height, seed, id) on one host thread: 2^height x 8714 permutations"""
    seed, key_id = bytes(seed), bytes(key_id)
    if len(seed) != 32 or len(key_id) != 16:
        raise KoskError("a seed has 32 bytes and a key identifier 16")
    out = C.create_string_buffer(HEADSIG_PUB_BYTES)
    if lib.kosk_headsig_public_from_seed(height, C.c_char_p(seed), C.c_char_p(key_id), out):
        raise KoskError("headsig_public_from_seed: height outside 1..24")
    return out.raw


TAPE_SEC_KEYSEED, TAPE_SEC_OFFLINE, TAPE_SEC_ONLINE = 0, 1, 2  # kosk_tape_section


def tape_section(k, section):
    """kosk_tape_section -> (offset, size) of section 0 key seed / 1 offline / 2 online of a tape"""
    off, size = C.c_size_t(), C.c_size_t()
    if lib.kosk_tape_section(k, section, C.byref(off), C.byref(size)):
        raise KoskError("tape_section: bad kyber_k or section")
    return off.value, size.value


def tape_splice(k, offline_tape, online_tape, seed_tape=None):
    """the spliced tape of INTEGRATION.md 14: key seed (of seed_tape, default online_tape) || offline section of offline_tape || online
    section of online_tape"""
    (o0, s0), (o1, s1), (o2, s2) = (tape_section(k, i) for i in range(3))
    head = online_tape if seed_tape is None else seed_tape
    return bytes(head[o0:o0 + s0]) + bytes(offline_tape[o1:o1 + s1]) + bytes(online_tape[o2:o2 + s2])


def proof_dense2_pack(k, pi):
    """host codec of kosk-dense-v2 (kosk_proof_dense2_pack) -> (return code, record): 0, -1 a stored value >= 4096, -2 a malformed I or
    a dropped row that is not the refill; the record is only meaningful for 0"""
    if len(pi) != proof_bytes(k):
        raise KoskError("proof_dense2_pack: an image of kosk_proof_bytes")
    out = C.create_string_buffer(dense2_proof_bytes(k))
    rc = lib.kosk_proof_dense2_pack(k, C.c_char_p(bytes(pi)), out)
    return rc, out.raw


def proof_dense2_unpack(k, rec):
    """kosk_proof_dense2_unpack -> (status, image): status 1 = malformed opened list (the dropped rows are zero)"""
    if len(rec) != dense2_proof_bytes(k):
        raise KoskError("proof_dense2_unpack: a record of kosk_dense2_proof_bytes")
    out = C.create_string_buffer(proof_bytes(k))
    rc = lib.kosk_proof_dense2_unpack(k, C.c_char_p(bytes(rec)), out)
    return rc, out.raw


def dense_pack(k, pi):
    """host codec of kosk-dense-v1 (kosk_proof_dense_pack) -> (return code, record): 0, -1 a stored value >= 4096, -2 a malformed I or
    a dropped row that is not the refill; the record is only meaningful for 0"""
    if len(pi) != proof_bytes(k):
        raise KoskError("dense_pack: an image of kosk_proof_bytes")
    out = C.create_string_buffer(dense_proof_bytes(k))
    rc = lib.kosk_proof_dense_pack(k, C.c_char_p(bytes(pi)), out)
    return rc, out.raw


def dense_unpack(k, rec):
    """kosk_proof_dense_unpack -> (status, image): status 1 = malformed opened list (the dropped rows are zero)"""
    if len(rec) != dense_proof_bytes(k):
        raise KoskError("dense_unpack: a record of kosk_dense_proof_bytes")
    out = C.create_string_buffer(proof_bytes(k))
    rc = lib.kosk_proof_dense_unpack(k, C.c_char_p(bytes(rec)), out)
    return rc, out.raw


CONTEXT_BYTES = 32


def bind_value(k, pk, context):
    """B of format kosk-bind-v1 for one public key and one 32-byte context, on the host (kosk_bind_value)"""
    pk, context = bytes(pk), bytes(context)
    if len(pk) != pk_bytes(k) or len(context) != CONTEXT_BYTES:
        raise KoskError("bind_value: a public key of kosk_pk_bytes and a context of %d bytes" % CONTEXT_BYTES)
    out = C.create_string_buffer(32)
    if lib.kosk_bind_value(k, C.c_char_p(pk), C.c_char_p(context), out):
        raise KoskError("kosk_bind_value: kyber_k outside 2..4")
    return out.raw


SALT_BYTES = 32


def keyseed_value(k, sk, context=None, salt=None):
    """the seed of format kosk-keyseed-v1 for one secret-key record, on the host (kosk_keyseed_value).  context None: unbound;
    salt None: the deterministic form.  The seed is as secret as the key."""
    sk = bytes(sk)
    if len(sk) != sk_bytes(k):
        raise KoskError("keyseed_value: a secret key of kosk_sk_bytes")
    if context is not None and len(context) != CONTEXT_BYTES:
        raise KoskError("a context has %d bytes" % CONTEXT_BYTES)
    if salt is not None and len(salt) != SALT_BYTES:
        raise KoskError("a salt has %d bytes" % SALT_BYTES)
    out = C.create_string_buffer(SEED_BYTES)
    cp = None if context is None else C.c_char_p(bytes(context))
    sp = None if salt is None else C.c_char_p(bytes(salt))
    if lib.kosk_keyseed_value(k, C.c_char_p(sk), cp, sp, out):
        raise KoskError("kosk_keyseed_value: kyber_k outside 2..4")
    return out.raw


SEL_STRIDE = 1312  # entries of a row of the opened-list tables as the handles lay them out (>= 1304)


def opened_tables(cand, sel_stride=SEL_STRIDE, fill=0):
    """tests (kosk_opened_tables): the host's round-2 function behind the PRF on 150 candidates, no handle -> (sel, rest), two rows of
    sel_stride u16 that held `fill` everywhere before the call: sel = I, the window boundaries at 160, the opened parties ascending at
    192 and their positions in I at 352; rest = the ascending complement"""
    cand = [int(c) for c in cand]
    if len(cand) != 150 or any(not 0 <= c < 65536 for c in cand):
        raise KoskError("opened_tables: 150 candidates")
    rows = max(int(sel_stride), 1)
    sel, rest = (C.c_uint16 * rows)(*([fill] * rows)), (C.c_uint16 * rows)(*([fill] * rows))
    if lib.kosk_opened_tables((C.c_uint16 * 150)(*cand), sel, rest, sel_stride):
        raise KoskError("kosk_opened_tables: an entry >= 1454, or sel_stride below a row of the tables")
    return list(sel), list(rest)


def tape_from_seed(k, seed):
    """the randomness tape of one 32-byte seed (format kosk-seedtape-v1, kosk_tape_from_seed)"""
    seed = bytes(seed)
    if len(seed) != SEED_BYTES:
        raise KoskError("a seed has %d bytes" % SEED_BYTES)
    out = C.create_string_buffer(tape_bytes(k) or 1)
    if lib.kosk_tape_from_seed(k, C.c_char_p(seed), out):
        raise KoskError("kosk_tape_from_seed: kyber_k outside 2..4")
    return out.raw


def proof_field(k, idx):
    off, size = C.c_size_t(), C.c_size_t()
    if lib.kosk_proof_field(k, idx, C.byref(off), C.byref(size)):
        raise KoskError("bad field")
    return off.value, size.value


def _buf(b):
    """bytes-like -> (ctypes pointer value, keepalive)"""
    if isinstance(b, (bytes, bytearray)):
        arr = (C.c_uint8 * len(b)).from_buffer_copy(b) if isinstance(b, bytes) else (C.c_uint8 * len(b)).from_buffer(b)
        return C.cast(arr, C.c_void_p), arr
    raise TypeError(type(b))


def _cut(buf, size, n):
    """n records of `size` bytes out of a ctypes buffer (ONE copy of the buffer: .raw copies all of it every time it is read)"""
    raw = buf.raw
    return [raw[i * size:(i + 1) * size] for i in range(n)]


def host_keygen(k, seed64):
    """kyber_keygen (kosk.cpp:4-70) on the host; returns pk, sk, A, s, e, t (lists of int)."""
    import numpy as np
    pk = C.create_string_buffer(pk_bytes(k)); sk = C.create_string_buffer(sk_bytes(k))
    A = np.zeros(k * k * 256, np.int16); s = np.zeros(k * 256, np.int16); e = np.zeros(k * 256, np.int16); t = np.zeros(k * 256, np.int16)
    r = lib.kosk_keygen(k, C.c_char_p(bytes(seed64)), pk, sk, A.ctypes.data, s.ctypes.data, e.ctypes.data, t.ctypes.data)
    if r:
        raise KoskError("kosk_keygen failed")
    return pk.raw, sk.raw, A, s, e, t


def host_sha3_256(data):
    out = C.create_string_buffer(32)
    lib.kosk_host_sha3_256(out, C.c_char_p(bytes(data)), len(data))
    return out.raw


def host_shake256(data, outlen):
    out = C.create_string_buffer(outlen)
    lib.kosk_host_shake256(out, outlen, C.c_char_p(bytes(data)), len(data))
    return out.raw


class DeviceView:
    """A window on library-owned HBM for torch (torch.as_tensor(view, device="cuda") is zero-copy): uint8, C-contiguous."""

    def __init__(self, ptr, shape):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "|u1", "data": (int(ptr), False), "version": 2, "strides": None}


class Kosk:
    """One library context = one GPU, one parameter set, up to max_batch proofs in flight.

    Mirrors the reference's top-level API (kosk.hpp):
      verifiable_keygen(tapes) -> (pk, sk, pi) lists      kyber_verifiable_keygen
      verify(pi, pk) -> list[bool]                         kyber_kosk_verify
    """

    def __init__(self, kyber_k=2, max_batch=1, device=0, entropy=None, **opts):
        """opts: fields of kosk_options (streams, combine, strict_encoding, fs_mode, host_threads, blocking_sync, ...): the handle is
        then created with kosk_create_ex; without any, with kosk_create (library defaults; no KOSK_* variable stands in for an option).
        entropy: ENTROPY_TAPE / ENTROPY_SEED, handed to set_entropy() once the handle exists (a setter, not an options field)"""
        self.k = kyber_k
        self.max_batch = max_batch
        self._h = C.c_void_p()
        if opts:
            self._opts = options(**opts)
            rc = lib.kosk_create_ex(C.byref(self._h), device, kyber_k, max_batch, C.byref(self._opts))
        else:
            rc = lib.kosk_create(C.byref(self._h), device, kyber_k, max_batch)
        if rc:
            raise KoskError("kosk_create: " + lib.kosk_last_error(None).decode())
        self.pk_bytes, self.sk_bytes = pk_bytes(kyber_k), sk_bytes(kyber_k)
        self.proof_bytes, self.tape_bytes = proof_bytes(kyber_k), tape_bytes(kyber_k)
        self._cb = None
        self._hook = None
        self._pk = self._sk = None
        if entropy is not None:
            try:
                self.set_entropy(entropy)
            except KoskError:
                self.close()
                raise

    def close(self):
        if self._h:
            lib.kosk_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, r, what):
        if r:
            raise KoskError(what + ": " + lib.kosk_last_error(self._h).decode())

    @property
    def handle(self):
        return self._h

    def set_randombytes(self, fn):
        """fn(nbytes) -> bytes, called in the reference's randombytes order."""
        if fn is None:
            self._cb = None
            self._chk(lib.kosk_set_randombytes(self._h, None, None), "set_randombytes")
            return
        CB = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_uint8), C.c_size_t)

        def tramp(_user, out, n):
            data = fn(n)
            C.memmove(out, data, n)
        self._cb = CB(tramp)
        self._chk(lib.kosk_set_randombytes(self._h, C.cast(self._cb, C.c_void_p), None), "set_randombytes")

    def set_entropy(self, mode):
        """what a call without tapes draws: ENTROPY_TAPE (default) the reference's sequence, a whole tape per proof; ENTROPY_SEED one
        32-byte seed per proof, expanded on the device (kosk_set_entropy)"""
        self._chk(lib.kosk_set_entropy(self._h, int(mode)), "set_entropy")

    def wipe_secrets(self):
        """zero every secret buffer of the handle now, HBM and page-locked staging; public resident state survives (kosk_wipe_secrets)"""
        self._chk(lib.kosk_wipe_secrets(self._h), "wipe_secrets")

    def set_wipe(self, mode):
        """WIPE_OFF (default), or WIPE_CALL: every entry point that brings secrets onto the handle ends with the wipe (kosk_set_wipe)"""
        self._chk(lib.kosk_set_wipe(self._h, int(mode)), "set_wipe")

    def secret_scan(self, needle):
        """the audit: at how many byte positions of ANY buffer the handle owns, HBM or page-locked, do these 16..64 bytes occur"""
        needle = bytes(needle)
        hits = C.c_long()
        if lib.kosk_secret_scan(self._h, C.c_char_p(needle), len(needle), C.byref(hits)):
            raise KoskError("secret_scan: " + (lib.kosk_last_error(self._h).decode() or "NULL argument or a needle outside 16..64 bytes"))
        return hits.value

    def wipe_device(self, d_ptrs, sizes):
        """kernel level: k_wipe on the caller's device memory, region i = [d_ptrs[i], d_ptrs[i] + sizes[i]) (int pointers)"""
        n = len(d_ptrs)
        ptrs = (C.c_void_p * max(n, 1))(*d_ptrs)
        lens = (C.c_size_t * max(n, 1))(*sizes)
        self._chk(lib.kosk_wipe_device(self._h, n, ptrs, lens), "wipe_device")

    def wipe_timing(self, reps=20):
        """diagnostic (kosk_wipe_timing): (ms per k_wipe launch over the secret HBM regions, ms of the runtime's fills of the same regions,
        bytes, regions)"""
        a, b, n, r = C.c_double(), C.c_double(), C.c_size_t(), C.c_int()
        self._chk(lib.kosk_wipe_timing(self._h, reps, C.byref(a), C.byref(b), C.byref(n), C.byref(r)), "wipe_timing")
        return a.value, b.value, n.value, r.value

    def set_contexts(self, contexts, n=None, stride=None):
        """arm the handle (kosk_set_contexts): from now on position b of every proving / verifying call uses context b.
        contexts: list of 32-byte bytes, or an int DEVICE pointer (with n, and stride if not 32)"""
        if isinstance(contexts, int):
            if n is None:
                raise KoskError("a device context pointer needs n")
            self._chk(lib.kosk_set_contexts(self._h, n, C.c_void_p(contexts), CONTEXT_BYTES if stride is None else stride), "set_contexts")
            return
        for c_ in contexts:
            if len(c_) != CONTEXT_BYTES:
                raise KoskError("a context has %d bytes" % CONTEXT_BYTES)
        st = CONTEXT_BYTES if stride is None else stride
        n = len(contexts) if n is None else n
        blob = b"".join(bytes(c_) + bytes(max(st - CONTEXT_BYTES, 0)) for c_ in contexts)
        self._chk(lib.kosk_set_contexts(self._h, n, C.c_char_p(blob), st), "set_contexts")

    def clear_contexts(self):
        """disarm the handle: it behaves exactly as one that was never armed"""
        self._chk(lib.kosk_set_contexts(self._h, 0, None, 0), "clear_contexts")

    def force_opened_candidates(self, lists, n=None):
        """tests (kosk_force_opened_candidates): lists = a list of lists of 150 candidates below 1454, proof b of every proving call on
        this handle then takes lists[b] where it would read its candidates from the PRF output; None clears.  n: the count handed to
        the library, if not len(lists)"""
        if lists is None:
            self._chk(lib.kosk_force_opened_candidates(self._h, 0, None), "force_opened_candidates")
            return
        flat = [int(c) for row in lists for c in row]
        if any(len(row) != 150 for row in lists) or any(not 0 <= c < 65536 for c in flat):
            raise KoskError("force_opened_candidates: lists of 150 candidates")
        arr = (C.c_uint16 * max(len(flat), 1))(*flat)
        self._chk(lib.kosk_force_opened_candidates(self._h, len(lists) if n is None else n, arr), "force_opened_candidates")

    def bind_device(self, n, pk, contexts, d_out, context_stride=CONTEXT_BYTES):
        """B for n proofs into device memory d_out (int pointer).  pk / contexts: bytes (host) or int device pointers"""
        a = C.c_void_p(pk) if isinstance(pk, int) else C.c_char_p(bytes(pk))
        b = C.c_void_p(contexts) if isinstance(contexts, int) else C.c_char_p(bytes(contexts))
        self._chk(lib.kosk_bind_device(self._h, n, a, b, context_stride, d_out), "bind_device")

    def keyseed_device(self, n, sk, d_seeds, contexts=None, context_stride=CONTEXT_BYTES, salts=None, salt_stride=SALT_BYTES):
        """n seeds of format kosk-keyseed-v1 into device memory d_seeds (int pointer, 8-byte aligned; kosk_keyseed_device).
        sk / contexts / salts: bytes (host) or int device pointers; contexts None: unbound, salts None: none"""
        def arg(v):
            return None if v is None else C.c_void_p(v) if isinstance(v, int) else C.c_char_p(bytes(v))
        self._chk(lib.kosk_keyseed_device(self._h, n, arg(sk), arg(contexts), context_stride, arg(salts), salt_stride, d_seeds), "keyseed_device")

    def _salt_arg(self, salts, n, salt_stride):
        """salts of the derived calls: None (deterministic), a list of 32-byte bytes, an int DEVICE pointer (salt_stride apart), or True
        (one os.urandom draw per proof, made here) -> (pointer, stride, keepalive)"""
        if salts is None:
            return None, 0, None
        if isinstance(salts, bool):
            if not salts:
                return None, 0, None
            salts = [os.urandom(SALT_BYTES) for _ in range(n)]
        if isinstance(salts, int):
            return C.c_void_p(salts), SALT_BYTES if salt_stride is None else salt_stride, None
        if len(salts) != n:
            raise KoskError("salts for %d proofs, secret keys for %d" % (len(salts), n))
        for s_ in salts:
            if len(s_) != SALT_BYTES:
                raise KoskError("a salt has %d bytes" % SALT_BYTES)
        blob = b"".join(bytes(s_) for s_ in salts)
        return C.c_char_p(blob), SALT_BYTES, blob

    def _seed_arg(self, seeds, n, seed_stride):
        """seeds: list of 32-byte bytes, an int DEVICE pointer (with n and seed_stride), or True (the library draws one 32-byte seed
        per proof through the callback / OS entropy; with n) -> (pointer, stride, n, keepalive)"""
        if seeds is True:
            if n is None:
                raise KoskError("seeds=True needs n")
            return None, SEED_BYTES, n, None
        if isinstance(seeds, int):
            if n is None:
                raise KoskError("a device seed pointer needs n")
            return C.c_void_p(seeds), SEED_BYTES if seed_stride is None else seed_stride, n, None
        for s_ in seeds:
            if len(s_) != SEED_BYTES:
                raise KoskError("a seed has %d bytes" % SEED_BYTES)
        blob = b"".join(bytes(s_) for s_ in seeds)
        return C.c_char_p(blob), SEED_BYTES, len(seeds), blob

    def tape_expand_device(self, seeds, d_tapes, tape_stride, n=None, seed_stride=None):
        """n tapes into DEVICE memory at d_tapes (int pointer), tape_stride apart, from seeds (list of bytes or int device pointer)"""
        sp, ss, n, _keep = self._seed_arg(seeds, n, seed_stride)
        self._chk(lib.kosk_tape_expand_device(self._h, n, sp, ss, d_tapes, tape_stride), "tape_expand_device")

    # ---- the wire formats (FMT_IMAGE / FMT_COMPACT / FMT_DENSE / FMT_DENSE2): one body per operation, the library's functions by format ----
    # format -> (suffix of the public names, size function, then the library's keygen, seeded keygen, verify, fetch and stage functions)
    _FMT = {fmt: (sfx, size) + tuple(name + sfx for name in ("kosk_verifiable_keygen_batch", "kosk_verifiable_keygen_seeded_batch", "kosk_verify_batch",
                                                              "kosk_fetch_proofs", "kosk_stage_verifier_inputs"))
            for fmt, sfx, size in ((FMT_IMAGE, "", "kosk_proof_bytes"), (FMT_COMPACT, "_compact", "kosk_compact_proof_bytes"),
                                   (FMT_DENSE, "_dense", "kosk_dense_proof_bytes"))}
    # kosk-dense-v2 has no names of its own in the library: the _fmt calls, with the format right behind the handle
    _FMT[FMT_DENSE2] = ("_dense2", "kosk_dense2_proof_bytes") + tuple(name + "_fmt" for name in _FMT[FMT_IMAGE][2:])
    _KEYGEN, _KEYGEN_SEEDED, _VERIFY, _FETCH, _STAGE = 2, 3, 4, 5, 6

    def _fmt(self, fmt, op):
        """(suffix, record size, the library's function for `op`) of a format"""
        row = self._FMT[fmt]
        fn = getattr(lib, row[op])
        if row[op].endswith("_fmt"):
            by_fmt = fn
            fn = lambda h, *args: by_fmt(h, fmt, *args)
        return row[0], getattr(lib, row[1])(self.k), fn

    def _keygen(self, fmt, tapes, n, seeds, seed_stride):
        if seeds is not None:
            tp, stride, n, _keep = self._seed_arg(seeds, n, seed_stride)
        elif tapes is not None:
            n, stride = len(tapes), self.tape_bytes
            if any(len(t) < stride for t in tapes):
                raise KoskError("tape shorter than kosk_tape_bytes")
            tp = C.c_char_p(b"".join(t[:stride] for t in tapes))
        else:
            n, stride, tp = 1 if n is None else n, 0, None
        sfx, size, fn = self._fmt(fmt, self._KEYGEN if seeds is None else self._KEYGEN_SEEDED)
        pk = C.create_string_buffer(self.pk_bytes * n); sk = C.create_string_buffer(self.sk_bytes * n)
        out = C.create_string_buffer(size * n)
        self._chk(fn(self._h, n, tp, stride, pk, sk, out), "verifiable_keygen" + sfx)
        return _cut(pk, self.pk_bytes, n), _cut(sk, self.sk_bytes, n), _cut(out, size, n)

    def _verify(self, fmt, recs, pks):
        sfx, _size, fn = self._fmt(fmt, self._VERIFY)
        n = len(recs)
        ok = C.create_string_buffer(n)
        self._chk(fn(self._h, n, C.c_char_p(b"".join(recs)), C.c_char_p(b"".join(pks)), ok), "verify" + sfx)
        return [b == 1 for b in ok.raw]

    def _fetch(self, fmt, n):
        sfx, size, fn = self._fmt(fmt, self._FETCH)
        out = C.create_string_buffer(size * n)
        self._chk(fn(self._h, n, out), "fetch_proofs" + sfx)
        return _cut(out, size, n)

    def _stage(self, fmt, recs, pks):
        sfx, _size, fn = self._fmt(fmt, self._STAGE)
        self._chk(fn(self._h, len(recs), b"".join(recs), b"".join(pks)), "stage_verifier_inputs" + sfx)

    def verifiable_keygen(self, tapes=None, n=None, seeds=None, seed_stride=None):
        """tapes: list of bytes (one randomness tape per instance) or None (callback / OS entropy).
        seeds (instead of tapes): seeded proving, see _seed_arg."""
        return self._keygen(FMT_IMAGE, tapes, n, seeds, seed_stride)

    def verifiable_keygen_compact(self, tapes=None, n=None, seeds=None, seed_stride=None):
        """verifiable_keygen with the proofs in the compact wire format (kosk_verifiable_keygen_[seeded_]batch_compact)"""
        return self._keygen(FMT_COMPACT, tapes, n, seeds, seed_stride)

    def verifiable_keygen_dense(self, tapes=None, n=None, seeds=None, seed_stride=None):
        """verifiable_keygen with the proofs in the dense wire format kosk-dense-v1 (kosk_verifiable_keygen_[seeded_]batch_dense)"""
        return self._keygen(FMT_DENSE, tapes, n, seeds, seed_stride)

    def verifiable_keygen_dense2(self, tapes=None, n=None, seeds=None, seed_stride=None):
        """verifiable_keygen with the proofs in the dense wire format kosk-dense-v2 (kosk_verifiable_keygen_[seeded_]batch_fmt)"""
        return self._keygen(FMT_DENSE2, tapes, n, seeds, seed_stride)

    def verify(self, pis, pks): return self._verify(FMT_IMAGE, pis, pks)
    def verify_dense(self, recs, pks): return self._verify(FMT_DENSE, recs, pks)
    def verify_dense2(self, recs, pks): return self._verify(FMT_DENSE2, recs, pks)
    def fetch_proofs_dense2(self, n): return self._fetch(FMT_DENSE2, n)
    def stage_verifier_inputs_dense2(self, recs, pks): self._stage(FMT_DENSE2, recs, pks)
    def fetch_proofs(self, n): return self._fetch(FMT_IMAGE, n)
    def fetch_proofs_compact(self, n): return self._fetch(FMT_COMPACT, n)
    def fetch_proofs_dense(self, n): return self._fetch(FMT_DENSE, n)

    def stage_verifier_inputs(self, pis, pks):
        """proof images and public keys into HBM for verify_resident (kosk_stage_verifier_inputs)"""
        self._stage(FMT_IMAGE, pis, pks)

    def stage_verifier_inputs_compact(self, blobs, pks): self._stage(FMT_COMPACT, blobs, pks)
    def stage_verifier_inputs_dense(self, recs, pks): self._stage(FMT_DENSE, recs, pks)

    def fail_masks(self, n):
        m = (C.c_uint32 * n)()
        self._chk(lib.kosk_verify_fail_masks(self._h, m, n), "fail_masks")
        return list(m)

    def dense_fill_device(self, n, d_images, image_stride, d_status):
        """kernel level: refill rows 407..1303 of the seven low-degree fields of n images in HBM, in place (int device pointers)"""
        self._chk(lib.kosk_dense_fill_device(self._h, n, d_images, image_stride, d_status), "dense_fill_device")

    def dense_check_device(self, n, d_images, image_stride, d_status):
        """kernel level: the codeword check on n images in HBM, read only (int device pointers); d_status[b] 0, 1 malformed I, 2 a row
        407..1303 of a listed field that is not the refill of rows 0..406"""
        self._chk(lib.kosk_dense_check_device(self._h, n, d_images, image_stride, d_status), "dense_check_device")

    def dense2_fill_device(self, n, d_images, image_stride, d_status):
        """kernel level: refill the dropped rows of kosk-dense-v2 (407.. of five fields, 151.. of the eta fields, 557.. of the u fields) of n
        images in HBM, in place (int device pointers)"""
        self._chk(lib.kosk_dense2_fill_device(self._h, n, d_images, image_stride, d_status), "dense2_fill_device")

    def dense2_check_device(self, n, d_images, image_stride, d_status):
        """kernel level: the codeword check of kosk-dense-v2 on n images in HBM, read only (int device pointers); d_status[b] 0, 1, 2"""
        self._chk(lib.kosk_dense2_check_device(self._h, n, d_images, image_stride, d_status), "dense2_check_device")

    def transcode(self, records, from_fmt, to_fmt, n=None, out=None):
        """kosk_transcode_batch: records of format from_fmt into format to_fmt (FMT_IMAGE / FMT_COMPACT / FMT_DENSE) -> (statuses, records).
        records: a list of bytes; or an int pointer (host or device memory, any alignment) to n consecutive records, with out an int
        pointer to room for n records of to_fmt -- then (statuses, None).  A record with a negative status is all zero."""
        ib, ob = lib.kosk_format_bytes(self.k, from_fmt), lib.kosk_format_bytes(self.k, to_fmt)
        if isinstance(records, int):
            if n is None or out is None:
                raise KoskError("transcode: a pointer needs n and out")
            st = (C.c_int32 * n)()
            self._chk(lib.kosk_transcode_batch(self._h, n, from_fmt, records, to_fmt, out, st), "transcode")
            return list(st), None
        n = len(records)
        if any(len(r) != ib for r in records):
            raise KoskError("transcode: records of kosk_format_bytes(k, from_fmt)")
        st = (C.c_int32 * max(n, 1))()
        buf = C.create_string_buffer(max(ob * n, 1))
        self._chk(lib.kosk_transcode_batch(self._h, n, from_fmt, C.c_char_p(b"".join(records)), to_fmt, buf, st), "transcode")
        return list(st)[:n], _cut(buf, ob, n)

    # second-level entry points (reference structs as bytes; see include/kosk_mi355x.h)
    def prepare_randomness(self, tapes=None, n=None):
        n = len(tapes) if tapes is not None else n
        size = lib.kosk_randomness_bytes(self.k)
        out = C.create_string_buffer(size * n)
        blob = b"".join(tapes) if tapes is not None else None
        self._chk(lib.kosk_prepare_randomness(self._h, n, blob, len(tapes[0]) if tapes is not None else 0, out), "prepare_randomness")
        return [out.raw[i * size:(i + 1) * size] for i in range(n)]

    def prepare_range_proof(self, tapes=None, n=None):
        n = len(tapes) if tapes is not None else n
        size = lib.kosk_range_proof_bytes(self.k)
        out = C.create_string_buffer(size * n)
        blob = b"".join(tapes) if tapes is not None else None
        self._chk(lib.kosk_prepare_range_proof(self._h, n, blob, len(tapes[0]) if tapes is not None else 0, out), "prepare_range_proof")
        return [out.raw[i * size:(i + 1) * size] for i in range(n)]

    def prove_prepared(self, insts, rands, ranges, tapes=None):
        n = len(insts)
        pi = C.create_string_buffer(self.proof_bytes * n)
        blob = b"".join(tapes) if tapes is not None else None
        self._chk(lib.kosk_prove_prepared(self._h, n, b"".join(insts), b"".join(rands), b"".join(ranges), blob,
                                          len(tapes[0]) if tapes is not None else 0, pi), "prove_prepared")
        return [pi.raw[i * self.proof_bytes:(i + 1) * self.proof_bytes] for i in range(n)]

    def verify_inst(self, proofs, insts):
        n = len(proofs)
        ok = (C.c_uint8 * n)()
        self._chk(lib.kosk_verify_inst(self._h, n, b"".join(proofs), b"".join(insts), ok), "verify_inst")
        return [bool(x) for x in ok]

    # resident split (bench)
    def stage_prover_inputs(self, tapes=None, n=None, seeds=None, seed_stride=None):
        if seeds is not None:
            sp, ss, n, _keep = self._seed_arg(seeds, n, seed_stride)
            self._pk = C.create_string_buffer(self.pk_bytes * n); self._sk = C.create_string_buffer(self.sk_bytes * n)
            self._chk(lib.kosk_stage_prover_inputs_seeded(self._h, n, sp, ss, self._pk, self._sk), "stage_prover_inputs")
            return n
        if tapes is not None:
            n = len(tapes)
        blob = b"".join(t[:self.tape_bytes] for t in tapes) if tapes is not None else None  # None: callback / OS entropy, with n
        self._pk = C.create_string_buffer(self.pk_bytes * n); self._sk = C.create_string_buffer(self.sk_bytes * n)
        self._chk(lib.kosk_stage_prover_inputs(self._h, n, C.c_char_p(blob) if blob is not None else None, self.tape_bytes, self._pk, self._sk), "stage_prover_inputs")
        return n

    def prove_resident(self, n):
        self._chk(lib.kosk_prove_resident(self._h, n), "prove_resident")

    def verify_resident(self, n):
        ok = C.create_string_buffer(n)
        self._chk(lib.kosk_verify_resident(self._h, n, ok), "verify_resident")
        return [b == 1 for b in ok.raw]

    def verifiable_keygen_resident(self, tapes=None, n=None, tape_stride=None, seeds=None, seed_stride=None):
        """kyber_verifiable_keygen as one resident call: key generation + prove, pk/sk returned, proofs stay in HBM.
        tapes: list of bytes, or an int DEVICE pointer (with n and tape_stride), or None (callback / OS entropy, with n).
        seeds (instead of tapes): seeded proving, see _seed_arg."""
        if seeds is not None:
            sp, ss, n, _keep = self._seed_arg(seeds, n, seed_stride)
            if getattr(self, "_pk", None) is None or len(self._pk) != self.pk_bytes * n:
                self._pk = C.create_string_buffer(self.pk_bytes * n); self._sk = C.create_string_buffer(self.sk_bytes * n)
            self._chk(lib.kosk_verifiable_keygen_seeded_resident(self._h, n, sp, ss, self._pk, self._sk), "verifiable_keygen_resident")
            return n
        if isinstance(tapes, int):
            tp, stride = C.c_void_p(tapes), tape_stride
        elif tapes is None:
            tp, stride = None, 0
        else:
            n = len(tapes)
            blob = b"".join(t[:self.tape_bytes] for t in tapes)
            tp, stride = C.c_char_p(blob), self.tape_bytes
        if getattr(self, "_pk", None) is None or len(self._pk) != self.pk_bytes * n:
            self._pk = C.create_string_buffer(self.pk_bytes * n); self._sk = C.create_string_buffer(self.sk_bytes * n)
        self._chk(lib.kosk_verifiable_keygen_resident(self._h, n, tp, stride, self._pk, self._sk), "verifiable_keygen_resident")
        return n

    def keys(self, n):
        """pk, sk lists of the last stage_prover_inputs / verifiable_keygen_resident"""
        return ([self._pk.raw[i * self.pk_bytes:(i + 1) * self.pk_bytes] for i in range(n)],
                [self._sk.raw[i * self.sk_bytes:(i + 1) * self.sk_bytes] for i in range(n)])

    def verify_resident_pk(self, n, pks=None):
        """kyber_kosk_verify on the resident proofs, pk decoding (polyvec_frombytes + gen_matrix) included; pks None = the
        pk bytes the key generation left in HBM"""
        ok = C.create_string_buffer(n)
        self._chk(lib.kosk_verify_resident_pk(self._h, n, C.c_char_p(b"".join(pks)) if pks is not None else None, ok), "verify_resident_pk")
        return [b == 1 for b in ok.raw]

    def resident_digests(self, rnd, n):
        """DeviceView of the round's digest table [n][1454][32] (round 0 Tcomm, 1 view commitments)"""
        d, stride = C.c_void_p(), C.c_size_t()
        self._chk(lib.kosk_resident_digests(self._h, rnd, C.byref(d), C.byref(stride)), "resident_digests")
        assert stride.value == 1454 * 32
        return DeviceView(d.value, (n, 1454, 32))

    def set_round_hook(self, fn):
        """fn(role, round, device_ptr, nbytes) on the calling thread when a round's digest table is complete in HBM"""
        if fn is None:
            self._hook = None
            self._chk(lib.kosk_set_round_hook(self._h, None, None), "set_round_hook")
            return
        CB = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t)
        self._hook = CB(lambda _u, role, rnd, ptr, nbytes: fn(role, rnd, ptr, nbytes))
        self._chk(lib.kosk_set_round_hook(self._h, C.cast(self._hook, C.c_void_p), None), "set_round_hook")

    def phase_seconds(self):
        out = (C.c_double * 16)()
        lib.kosk_phase_seconds(self._h, out, 16)
        return list(out)

    PROFILE_IDS = ["hash_tcomm", "hash_view", "gemm_expand1", "gemm_expand2", "lincomb", "ntt_f", "assemble",
                   "v_hash_tcomm", "v_hash_view", "v_interp_build", "v_gemm_interp", "v_gemm_expand", "v_gemm_recon", "v_lincomb",
                   "fs_alpha", "fs_opened", "v_fs_alpha", "v_fs_opened"]

    def profile_enable(self, on=True):
        self._chk(lib.kosk_profile_enable(self._h, int(on)), "profile_enable")

    def profile_read(self):
        """{name: (total_ms, launches)} since profile_enable()"""
        out = {}
        for i, name in enumerate(self.PROFILE_IDS):
            ms, cnt = C.c_double(), C.c_long()
            lib.kosk_profile_read(self._h, i, C.byref(ms), C.byref(cnt))
            out[name] = (ms.value, cnt.value)
        return out

    def profile_read_units(self):
        """{name: (total_ms, launches, proofs served by those launches)}: a merged run of a cohort (KOSK_COMBINE) serves several
        callers' batches per launch and is timed on the handle that led it"""
        out = {}
        for i, name in enumerate(self.PROFILE_IDS):
            ms, cnt, units = C.c_double(), C.c_long(), C.c_long()
            lib.kosk_profile_read_units(self._h, i, C.byref(ms), C.byref(cnt), C.byref(units))
            out[name] = (ms.value, cnt.value, units.value)
        return out

    def combine_stats(self):
        """(resident calls of this handle served through the combiner, sum over them of the members their run served)"""
        a, b = C.c_long(), C.c_long()
        self._chk(lib.kosk_combine_stats(self._h, C.byref(a), C.byref(b)), "combine_stats")
        return a.value, b.value

    def _records(self, what, x, n, size):
        """list of `size`-byte records or an int DEVICE pointer (with n) -> (pointer, n, keepalive)"""
        if isinstance(x, int):
            if n is None:
                raise KoskError("a device pointer for %s needs n" % what)
            return C.c_void_p(x), n, None
        for r_ in x:
            if len(r_) != size:
                raise KoskError("a %s record has %d bytes" % (what, size))
        blob = b"".join(bytes(r_) for r_ in x)
        return C.c_char_p(blob), len(x), blob

    def _kem_out(self, out, n, sizes):
        """out: None (host buffers, returned as lists of bytes) or a tuple of int DEVICE pointers, one per output"""
        if out is not None:
            if len(out) != len(sizes):
                raise KoskError("out needs %d device pointers" % len(sizes))
            return [C.c_void_p(int(p_)) for p_ in out], None
        bufs = [C.create_string_buffer(s_ * n) for s_ in sizes]
        return bufs, bufs

    def kem_enc(self, pks, coins=None, n=None, out=None):
        """crypto_kem_enc_derand for n public keys (kosk_kem_enc_batch).  pks / coins: lists of bytes or int DEVICE pointers (with n);
        coins=None: one 32-byte draw per item through the randombytes callback / OS entropy.  Returns (cts, sss) as lists of bytes, or,
        with out=(d_ct, d_ss) int device pointers, writes there and returns out."""
        pp, n, _k1 = self._records("pk", pks, n, self.pk_bytes)
        cp, _k2 = None, None
        if coins is not None:
            cp, nc, _k2 = self._records("coins", coins, n, 32)
            if nc != n:
                raise KoskError("coins for %d items, public keys for %d" % (nc, n))
        ctb = ct_bytes(self.k)
        bufs, host = self._kem_out(out, n, (ctb, SS_BYTES))
        self._chk(lib.kosk_kem_enc_batch(self._h, n, pp, cp, bufs[0], bufs[1]), "kem_enc")
        if host is None:
            return out
        return _cut(bufs[0], ctb, n), _cut(bufs[1], SS_BYTES, n)

    def kem_dec(self, cts, sks, n=None, out=None):
        """crypto_kem_dec for n (ciphertext, secret key) pairs (kosk_kem_dec_batch); inputs as in kem_enc.  Returns the list of shared
        secrets, or, with out = an int device pointer, writes there and returns it."""
        ctb = ct_bytes(self.k)
        cp, n, _k1 = self._records("ct", cts, n, ctb)
        sp, ns, _k2 = self._records("sk", sks, n, self.sk_bytes)
        if ns != n:
            raise KoskError("secret keys for %d items, ciphertexts for %d" % (ns, n))
        bufs, host = self._kem_out(None if out is None else (out,), n, (SS_BYTES,))
        self._chk(lib.kosk_kem_dec_batch(self._h, n, cp, sp, bufs[0]), "kem_dec")
        if host is None:
            return out
        return _cut(bufs[0], SS_BYTES, n)

    def kem_keypair(self, coins=None, n=None, out=None):
        """crypto_kem_keypair_derand for n items (kosk_kem_keypair_batch).  coins: a list of 64-byte values (d || z) or an int DEVICE
        pointer (with n); None: one 64-byte draw per item through the randombytes callback / OS entropy (with n, default 1).  Returns
        (pks, sks) as lists of bytes, or, with out=(d_pk, d_sk) int device pointers, writes there and returns out."""
        cp, _k = None, None
        if coins is not None:
            cp, n, _k = self._records("coins", coins, n, KEYPAIR_COIN_BYTES)
        elif n is None:
            n = 1
        bufs, host = self._kem_out(out, n, (self.pk_bytes, self.sk_bytes))
        self._chk(lib.kosk_kem_keypair_batch(self._h, n, cp, bufs[0], bufs[1]), "kem_keypair")
        if host is None:
            return out
        return _cut(bufs[0], self.pk_bytes, n), _cut(bufs[1], self.sk_bytes, n)

    def _kem_check(self, fn, what, recs, n, size):
        rp, n, _k = self._records(what, recs, n, size)
        flags = C.create_string_buffer(max(n, 1))
        self._chk(fn(self._h, n, rp, flags), "kem_check_" + what)
        return list(flags.raw[:n])

    def kem_check_pk(self, pks, n=None):
        """kosk_kem_check_pk: per public key 0 or KEYCHK_PK_RANGE (a 12-bit field >= q, FIPS 203 7.2).  pks: list of bytes or an int
        DEVICE pointer (with n)"""
        return self._kem_check(lib.kosk_kem_check_pk, "pk", pks, n, self.pk_bytes)

    def kem_check_sk(self, sks, n=None):
        """kosk_kem_check_sk: per secret key the OR of KEYCHK_HASH (FIPS 203 7.3), KEYCHK_PK_RANGE and KEYCHK_S_RANGE; 0 = passes"""
        return self._kem_check(lib.kosk_kem_check_sk, "sk", sks, n, self.sk_bytes)

    def kem_enc_verified(self, n, coins=None):
        """kosk_kem_enc_verified: encapsulate to the public keys the last completed verify call left in HBM, where its verify bit is 1.
        Returns (cts, sss, done); ct and ss of a rejected position are zero-filled."""
        cp, _k = None, None
        if coins is not None:
            cp, nc, _k = self._records("coins", coins, n, 32)
            if nc != n:
                raise KoskError("coins for %d items, n = %d" % (nc, n))
        ctb = ct_bytes(self.k)
        ct = C.create_string_buffer(ctb * n); ss = C.create_string_buffer(SS_BYTES * n); done = C.create_string_buffer(n)
        self._chk(lib.kosk_kem_enc_verified(self._h, n, cp, ct, ss, done), "kem_enc_verified")
        return _cut(ct, ctb, n), _cut(ss, SS_BYTES, n), [bool(x) for x in done.raw[:n]]

    # one resident key
    def kem_key_set(self, pk=None, sk=None):
        """kosk_kem_key_set: load ONE record into the handle's key slot, exactly one of pk / sk (bytes, or an int DEVICE pointer);
        replaces the slot"""
        if (pk is None) == (sk is None):
            raise KoskError("kem_key_set: exactly one of pk / sk")
        rec, size, what = (pk, self.pk_bytes, "pk") if sk is None else (sk, self.sk_bytes, "sk")
        ptr, _n, _k = self._records(what, rec if isinstance(rec, int) else [rec], 1, size)
        self._chk(lib.kosk_kem_key_set(self._h, ptr if sk is None else None, None if sk is None else ptr), "kem_key_set")

    def kem_key_state(self):
        """KEM_KEY_NONE / KEM_KEY_PK / KEM_KEY_SK (kosk_kem_key_state)"""
        return lib.kosk_kem_key_state(self._h)

    def kem_key_clear(self):
        """wipe and empty the key slot (kosk_kem_key_clear)"""
        self._chk(lib.kosk_kem_key_clear(self._h), "kem_key_clear")

    def kem_enc_key(self, n=None, coins=None, out=None):
        """kosk_kem_enc_key: n encapsulations to the loaded key; coins / out as in kem_enc (coins=None: n draws, n defaults to 1)"""
        cp, _k = None, None
        if coins is not None:
            cp, n, _k = self._records("coins", coins, n, 32)
        elif n is None:
            n = 1
        ctb = ct_bytes(self.k)
        bufs, host = self._kem_out(out, n, (ctb, SS_BYTES))
        self._chk(lib.kosk_kem_enc_key(self._h, n, cp, bufs[0], bufs[1]), "kem_enc_key")
        if host is None:
            return out
        return _cut(bufs[0], ctb, n), _cut(bufs[1], SS_BYTES, n)

    def kem_dec_key(self, cts, n=None, out=None):
        """kosk_kem_dec_key: decapsulate n ciphertexts with the loaded secret key; cts / out as in kem_dec"""
        ctb = ct_bytes(self.k)
        cp, n, _k = self._records("ct", cts, n, ctb)
        bufs, host = self._kem_out(None if out is None else (out,), n, (SS_BYTES,))
        self._chk(lib.kosk_kem_dec_key(self._h, n, cp, bufs[0]), "kem_dec_key")
        if host is None:
            return out
        return _cut(bufs[0], SS_BYTES, n)

    # the verified-key registry
    @staticmethod
    def _slots(slots):
        """a list of slot ids -> (int32 array in host memory, n)"""
        arr = (C.c_int32 * max(len(slots), 1))(*[int(s_) for s_ in slots])
        return arr, len(slots)

    def registry_reserve(self, capacity):
        """kosk_registry_reserve: exactly `capacity` empty slots in HBM (0 frees); only while no slot is occupied"""
        self._chk(lib.kosk_registry_reserve(self._h, capacity), "registry_reserve")

    def registry_level(self):
        """kosk_registry_level -> (used, capacity)"""
        u, c_ = C.c_int(), C.c_int()
        self._chk(lib.kosk_registry_level(self._h, C.byref(u), C.byref(c_)), "registry_level")
        return u.value, c_.value

    def registry_admit_verified(self, slots):
        """kosk_registry_admit_verified: key b of the last completed verify call into slots[b] where its verify bit is 1; returns those bits"""
        sp, n = self._slots(slots)
        done = C.create_string_buffer(max(n, 1))
        self._chk(lib.kosk_registry_admit_verified(self._h, n, sp, done), "registry_admit_verified")
        return [bool(x) for x in done.raw[:n]]

    def registry_admit(self, pks, slots, accept=None, n=None):
        """kosk_registry_admit: the CALLER vouches for these keys (no proof was seen).  pks: a list of bytes or an int DEVICE pointer (with n);
        accept: None for all, or one truth value per key (0: the slot is left alone)"""
        pp, n, _k = self._records("pk", pks, n, self.pk_bytes)
        sp, ns = self._slots(slots)
        if ns != n or (accept is not None and len(accept) != n):
            raise KoskError("registry_admit: %d keys need %d slots and accept bytes" % (n, n))
        ap = None if accept is None else C.c_char_p(bytes(1 if a_ else 0 for a_ in accept))
        self._chk(lib.kosk_registry_admit(self._h, n, pp, ap, sp), "registry_admit")

    def registry_evict(self, slots):
        """kosk_registry_evict: zero the named slots' records and flags"""
        sp, n = self._slots(slots)
        self._chk(lib.kosk_registry_evict(self._h, n, sp), "registry_evict")

    def registry_read(self, slots):
        """kosk_registry_read -> (states, pks, hs): occupancy, the pk bytes and SHA3-256 of them per named slot (zeros for an empty one)"""
        sp, n = self._slots(slots)
        state = C.create_string_buffer(max(n, 1))
        pk = C.create_string_buffer(self.pk_bytes * max(n, 1)); h = C.create_string_buffer(32 * max(n, 1))
        self._chk(lib.kosk_registry_read(self._h, n, sp, state, pk, h), "registry_read")
        return list(state.raw[:n]), _cut(pk, self.pk_bytes, n), _cut(h, 32, n)

    def kem_enc_slots(self, slots, coins=None, out=None):
        """kosk_kem_enc_slots: item b to the key in slots[b]; coins / out as in kem_enc, with out=(d_ct, d_ss, d_done).  Returns (cts, sss,
        done); ct and ss of an empty slot are zero-filled"""
        sp, n = self._slots(slots)
        cp, _k = None, None
        if coins is not None:
            cp, nc, _k = self._records("coins", coins, n, 32)
            if nc != n:
                raise KoskError("coins for %d items, slots for %d" % (nc, n))
        ctb = ct_bytes(self.k)
        bufs, host = self._kem_out(out, n, (ctb, SS_BYTES, 1))
        self._chk(lib.kosk_kem_enc_slots(self._h, n, sp, cp, bufs[0], bufs[1], bufs[2]), "kem_enc_slots")
        if host is None:
            return out
        return _cut(bufs[0], ctb, n), _cut(bufs[1], SS_BYTES, n), [bool(x) for x in bufs[2].raw[:n]]

    # the registry by fingerprint
    def registry_find(self, hs, n=None, out=None):
        """kosk_registry_find: per fingerprint SHA3-256(pk) the lowest occupied slot that holds the key, or -1.  hs: a list of 32-byte
        strings or an int DEVICE pointer (with n); out: None (a list of ints is returned) or an int DEVICE pointer to n int32"""
        hp, n, _k = self._records("fingerprint", hs, n, 32)
        if out is not None:
            self._chk(lib.kosk_registry_find(self._h, n, hp, C.c_void_p(int(out))), "registry_find")
            return out
        slots = (C.c_int32 * max(n, 1))()
        self._chk(lib.kosk_registry_find(self._h, n, hp, slots), "registry_find")
        return list(slots[:n])

    def registry_enrol(self, pks, accept=None, n=None):
        """kosk_registry_enrol: kosk_registry_admit with the slots picked by the library and duplicates refused -> (slots, status), status
        ENROL_REJECTED / ENROL_ADMITTED / ENROL_DUPLICATE per key.  pks / accept as in registry_admit"""
        pp, n, _k = self._records("pk", pks, n, self.pk_bytes)
        if accept is not None and len(accept) != n:
            raise KoskError("registry_enrol: %d keys need %d accept bytes" % (n, n))
        ap = None if accept is None else C.c_char_p(bytes(1 if a_ else 0 for a_ in accept))
        slots = (C.c_int32 * max(n, 1))(); status = C.create_string_buffer(max(n, 1))
        self._chk(lib.kosk_registry_enrol(self._h, n, pp, ap, slots, status), "registry_enrol")
        return list(slots[:n]), list(status.raw[:n])

    def registry_enrol_verified(self, n):
        """kosk_registry_enrol_verified: the first n keys of the last completed verify call, where its verify bit is 1 -> (slots, status)"""
        slots = (C.c_int32 * max(n, 1))(); status = C.create_string_buffer(max(n, 1))
        self._chk(lib.kosk_registry_enrol_verified(self._h, n, slots, status), "registry_enrol_verified")
        return list(slots[:n]), list(status.raw[:n])

    def kem_enc_peers(self, hs, coins=None, out=None, n=None):
        """kosk_kem_enc_peers: item b to the registry's key with fingerprint hs[b] (a list of 32-byte strings, or an int DEVICE pointer
        with n); coins / out as in kem_enc_slots.  Returns (cts, sss, done); ct and ss of a fingerprint that is not found are zero-filled"""
        hp, n, _k1 = self._records("fingerprint", hs, n, 32)
        cp, _k2 = None, None
        if coins is not None:
            cp, nc, _k2 = self._records("coins", coins, n, 32)
            if nc != n:
                raise KoskError("coins for %d items, fingerprints for %d" % (nc, n))
        ctb = ct_bytes(self.k)
        bufs, host = self._kem_out(out, n, (ctb, SS_BYTES, 1))
        self._chk(lib.kosk_kem_enc_peers(self._h, n, hp, cp, bufs[0], bufs[1], bufs[2]), "kem_enc_peers")
        if host is None:
            return out
        return _cut(bufs[0], ctb, n), _cut(bufs[1], SS_BYTES, n), [bool(x) for x in bufs[2].raw[:n]]

    # the registry tree, kosk-regtree-v1
    def registry_root(self, out=None):
        """kosk_registry_root -> (root, used, capacity); out: an int DEVICE pointer to 32 bytes, returned in place of the root"""
        u, c_ = C.c_int(), C.c_int()
        buf = C.create_string_buffer(32) if out is None else C.c_void_p(int(out))
        self._chk(lib.kosk_registry_root(self._h, buf, C.byref(u), C.byref(c_)), "registry_root")
        return (buf.raw if out is None else out), u.value, c_.value

    def registry_prove_slots(self, slots, out=None):
        """kosk_registry_prove_slots -> (states, hs, paths, root): occupancy, the stored fingerprint (zeros for an empty slot) and the
        inclusion path (a bytes of depth x 32) per named slot, and the root they belong to.  out=(d_h, d_paths, d_root): int DEVICE
        pointers (any of them None); (states, out) is returned"""
        sp, n = self._slots(slots)
        d = registry_tree_depth(self.registry_level()[1])
        state = C.create_string_buffer(max(n, 1))
        if out is not None:
            ptr = [None if p is None else C.c_void_p(int(p)) for p in out]
            self._chk(lib.kosk_registry_prove_slots(self._h, n, sp, state, ptr[0], ptr[1], ptr[2]), "registry_prove_slots")
            return list(state.raw[:n]), out
        h = C.create_string_buffer(32 * max(n, 1)); paths = C.create_string_buffer(max(32 * max(d, 0) * n, 1)); root = C.create_string_buffer(32)
        self._chk(lib.kosk_registry_prove_slots(self._h, n, sp, state, h, paths, root), "registry_prove_slots")
        return list(state.raw[:n]), _cut(h, 32, n), [paths.raw[32 * d * b:32 * d * (b + 1)] for b in range(n)], root.raw

    def registry_prove_peers(self, hs, n=None, out=None):
        """kosk_registry_prove_peers -> (slots, paths, done, root): per fingerprint the lowest occupied slot that holds it (or -1), its
        inclusion path (zeros for a miss) and whether it was found.  hs: a list of 32-byte strings or an int DEVICE pointer (with n);
        out=(d_slots, d_paths, d_done, d_root): int DEVICE pointers (d_root may be None), returned as they are"""
        hp, n, _k = self._records("fingerprint", hs, n, 32)
        d = registry_tree_depth(self.registry_level()[1])
        if out is not None:
            ptr = [None if p is None else C.c_void_p(int(p)) for p in out]
            self._chk(lib.kosk_registry_prove_peers(self._h, n, hp, ptr[0], ptr[1], ptr[2], ptr[3]), "registry_prove_peers")
            return out
        slots = (C.c_int32 * max(n, 1))(); done = C.create_string_buffer(max(n, 1))
        paths = C.create_string_buffer(max(32 * max(d, 0) * n, 1)); root = C.create_string_buffer(32)
        self._chk(lib.kosk_registry_prove_peers(self._h, n, hp, slots, paths, done, root), "registry_prove_peers")
        return list(slots[:n]), [paths.raw[32 * d * b:32 * d * (b + 1)] for b in range(n)], [bool(x) for x in done.raw[:n]], root.raw

    # the sorted tree, kosk-regsort-v1
    def registry_sorted_root(self, out=None):
        """kosk_registry_sorted_root -> (root, used, capacity); out: an int DEVICE pointer to 32 bytes, returned in place of the root"""
        u, c_ = C.c_int(), C.c_int()
        buf = C.create_string_buffer(32) if out is None else C.c_void_p(int(out))
        self._chk(lib.kosk_registry_sorted_root(self._h, buf, C.byref(u), C.byref(c_)), "registry_sorted_root")
        return (buf.raw if out is None else out), u.value, c_.value

    def registry_prove_absent(self, hs, n=None, out=None):
        """kosk_registry_prove_absent -> (kinds, records, root): per fingerprint REGSORT_ABSENT or REGSORT_PRESENT and the proof record
        (kosk_regsort_check_proof reads it).  hs: a list of 32-byte strings or an int DEVICE pointer (with n); out=(d_kind, d_records,
        d_root): int DEVICE pointers (d_root may be None), returned as they are"""
        hp, n, _k = self._records("fingerprint", hs, n, 32)
        rec = regsort_proof_bytes(registry_tree_depth(self.registry_level()[1]))
        if out is not None:
            ptr = [None if p is None else C.c_void_p(int(p)) for p in out]
            self._chk(lib.kosk_registry_prove_absent(self._h, n, hp, ptr[0], ptr[1], ptr[2]), "registry_prove_absent")
            return out
        kind = C.create_string_buffer(max(n, 1)); records = C.create_string_buffer(max(rec * n, 1)); root = C.create_string_buffer(32)
        self._chk(lib.kosk_registry_prove_absent(self._h, n, hp, kind, records, root), "registry_prove_absent")
        return list(kind.raw[:n]), [records.raw[rec * b:rec * (b + 1)] for b in range(n)], root.raw

    def regsort_order(self, n, d_h, d_flag, d_order):
        """kosk_regsort_order_device: the sort kernels alone on n caller-made fingerprints (d_h, n x 32 bytes) and flags (d_flag, n bytes) in
        DEVICE memory; d_order (n int32, DEVICE memory) = the index of the i-th entry in (fingerprint, index) order, -1 behind the entries"""
        self._chk(lib.kosk_regsort_order_device(self._h, n, C.c_void_p(int(d_h)), C.c_void_p(int(d_flag)), C.c_void_p(int(d_order))), "regsort_order")
        return d_order

    # the registry history, kosk-reghist-v1
    def registry_history_reserve(self, max_events):
        """kosk_registry_history_reserve: an append-only history of up to max_events events on an EMPTY registry; 0 frees"""
        self._chk(lib.kosk_registry_history_reserve(self._h, max_events), "registry_history_reserve")

    def registry_history_level(self):
        """kosk_registry_history_level -> (size, max_events)"""
        s_, m = C.c_int(), C.c_int()
        self._chk(lib.kosk_registry_history_level(self._h, C.byref(s_), C.byref(m)), "registry_history_level")
        return s_.value, m.value

    def registry_history_head(self, size=-1, out=None):
        """kosk_registry_history_head -> (root, size): the root over the first `size` events (< 0: all); out: an int DEVICE pointer to 32
        bytes, returned in place of the root"""
        n = C.c_int()
        buf = C.create_string_buffer(32) if out is None else C.c_void_p(int(out))
        self._chk(lib.kosk_registry_history_head(self._h, size, buf, C.byref(n)), "registry_history_head")
        return (buf.raw if out is None else out), n.value

    def registry_history_checkpoint(self):
        """kosk_registry_history_checkpoint -> the index of the appended op-3 event, which binds both state roots, used and capacity"""
        i = C.c_int()
        self._chk(lib.kosk_registry_history_checkpoint(self._h, C.byref(i)), "registry_history_checkpoint")
        return i.value

    def registry_history_read(self, first=0, n=None, out=None):
        """kosk_registry_history_read -> the raw 80-byte records of events first .. first + n - 1 (n None: up to the current size); out: an
        int DEVICE pointer, returned as it is"""
        if n is None:
            n = self.registry_history_level()[0] - first
        if n == 0 and out is None:
            return []
        buf = C.create_string_buffer(max(REGHIST_EVENT_BYTES * n, 1)) if out is None else C.c_void_p(int(out))
        self._chk(lib.kosk_registry_history_read(self._h, first, n, buf), "registry_history_read")
        return _cut(buf, REGHIST_EVENT_BYTES, n) if out is None else out

    def _history_size(self, size):
        return self.registry_history_level()[0] if size < 0 else size

    def registry_history_prove_events(self, indices, size=-1, out=None):
        """kosk_registry_history_prove_events -> (leaves, records, root): per event index its leaf hash and inclusion record at `size`
        (< 0: the current size), and the head at that size.  out=(d_leaves, d_records, d_root): int DEVICE pointers (d_leaves and d_root
        may be None), returned as they are"""
        n = len(indices)
        ip_ = (C.c_int32 * max(n, 1))(*indices)
        if out is not None:
            ptr = [None if p is None else C.c_void_p(int(p)) for p in out]
            self._chk(lib.kosk_registry_history_prove_events(self._h, size, n, ip_, ptr[0], ptr[1], ptr[2]), "registry_history_prove_events")
            return out
        rec = reghist_path_bytes(self._history_size(size))
        leaves = C.create_string_buffer(32 * max(n, 1)); records = C.create_string_buffer(max(rec * n, 1)); root = C.create_string_buffer(32)
        self._chk(lib.kosk_registry_history_prove_events(self._h, size, n, ip_, leaves, records, root), "registry_history_prove_events")
        return _cut(leaves, 32, n), [records.raw[rec * b:rec * (b + 1)] for b in range(n)], root.raw

    def registry_history_prove_consistency(self, old_sizes, size=-1, out=None):
        """kosk_registry_history_prove_consistency -> (records, root): per old size the consistency record to `size` (< 0: the current
        size), and the head at that size.  out=(d_records, d_root): int DEVICE pointers (d_root may be None), returned as they are"""
        n = len(old_sizes)
        op_ = (C.c_int32 * max(n, 1))(*old_sizes)
        if out is not None:
            ptr = [None if p is None else C.c_void_p(int(p)) for p in out]
            self._chk(lib.kosk_registry_history_prove_consistency(self._h, size, n, op_, ptr[0], ptr[1]), "registry_history_prove_consistency")
            return out
        rec = reghist_consistency_bytes(self._history_size(size))
        records = C.create_string_buffer(max(rec * n, 1)); root = C.create_string_buffer(32)
        self._chk(lib.kosk_registry_history_prove_consistency(self._h, size, n, op_, records, root), "registry_history_prove_consistency")
        return [records.raw[rec * b:rec * (b + 1)] for b in range(n)], root.raw

    # the registry monitor
    def monitor_reserve(self, capacity, max_events):
        """kosk_monitor_reserve: a fresh, empty replay of up to max_events events onto a table of `capacity` slots; (0, 0) frees"""
        self._chk(lib.kosk_monitor_reserve(self._h, capacity, max_events), "monitor_reserve")

    def monitor_level(self):
        """kosk_monitor_level -> (size, max_events, used, capacity, failed)"""
        v = [C.c_int() for _ in range(5)]
        self._chk(lib.kosk_monitor_level(self._h, *[C.byref(x) for x in v]), "monitor_level")
        return v[0].value, v[1].value, v[2].value, v[3].value, bool(v[4].value)

    def monitor_feed(self, events, n=None):
        """kosk_monitor_feed -> (ok, bad_index, reason): the next events of the log, a list of 80-byte records, one bytes object, or an int
        DEVICE pointer (with n).  ok False: the log is invalid at bad_index for MONITOR_<reason>; (True, -1, MONITOR_OK) otherwise"""
        if isinstance(events, (bytes, bytearray)):
            if len(events) % REGHIST_EVENT_BYTES:
                raise KoskError("an event record has %d bytes" % REGHIST_EVENT_BYTES)
            blob = bytes(events)
            ep, n = C.c_char_p(blob), len(blob) // REGHIST_EVENT_BYTES
        else:
            ep, n, _k = self._records("event", events, n, REGHIST_EVENT_BYTES)
        i, why = C.c_int(), C.c_int()
        r = lib.kosk_monitor_feed(self._h, n, ep, C.byref(i), C.byref(why))
        if r < 0:
            self._chk(r, "monitor_feed")
        return r == 1, i.value, why.value

    def monitor_head(self, size=-1, out=None):
        """kosk_monitor_head -> (root, size): the history root over the first `size` events fed (< 0: all); out: an int DEVICE pointer to 32
        bytes, returned in place of the root"""
        n = C.c_int()
        buf = C.create_string_buffer(32) if out is None else C.c_void_p(int(out))
        self._chk(lib.kosk_monitor_head(self._h, size, buf, C.byref(n)), "monitor_head")
        return (buf.raw if out is None else out), n.value

    def monitor_roots(self, out=None):
        """kosk_monitor_roots -> (slot_root, sorted_root) of the replayed table; out=(d_slot_root, d_sorted_root): int DEVICE pointers
        (either may be None), returned as they are"""
        if out is not None:
            ptr = [None if p is None else C.c_void_p(int(p)) for p in out]
            self._chk(lib.kosk_monitor_roots(self._h, ptr[0], ptr[1]), "monitor_roots")
            return out
        a, b = C.create_string_buffer(32), C.create_string_buffer(32)
        self._chk(lib.kosk_monitor_roots(self._h, a, b), "monitor_roots")
        return a.raw, b.raw

    def monitor_read(self, slots, out=None):
        """kosk_monitor_read -> (states, hs): occupancy and the fingerprint per named slot of the replayed table (zeros for an empty one);
        out: an int DEVICE pointer to n x 32 bytes, returned in place of hs"""
        sp, n = self._slots(slots)
        state = C.create_string_buffer(max(n, 1))
        h = C.create_string_buffer(32 * max(n, 1)) if out is None else C.c_void_p(int(out))
        self._chk(lib.kosk_monitor_read(self._h, n, sp, state, h), "monitor_read")
        return list(state.raw[:n]), (_cut(h, 32, n) if out is None else out)

    # the relying party: no registry on the handle
    @staticmethod
    def _peer_slots(slots, n):
        """a list of slot ids (any int32, they are peer data) or an int pointer (with n) -> (pointer, n, keepalive)"""
        if isinstance(slots, int):
            if n is None:
                raise KoskError("a pointer for slots needs n")
            return C.c_void_p(slots), n, None
        arr = (C.c_int32 * max(len(slots), 1))(*[int(s_) for s_ in slots])
        return arr, len(slots), arr

    @staticmethod
    def _peer_root(root):
        """32 bytes, or an int pointer -> (pointer, keepalive)"""
        if isinstance(root, int):
            return C.c_void_p(root), None
        root = _digest("a root", root)
        return C.c_char_p(root), root

    def regtree_check_paths(self, depth, slots, hs, paths, root, states=None, out=None, n=None):
        """kosk_regtree_check_paths -> [ok]: item b is 1 iff (slots[b], hs[b] or "empty" where states[b] == 0, paths[b]) walks to root.
        slots: a list of ints; hs: a list of 32-byte strings, or None where every state is 0; paths: a list of depth x 32-byte strings
        (None where depth == 0); states: None (all occupied) or one truth value per item.  Each of them may instead be an int pointer
        to host or DEVICE memory (with n).  out: an int pointer to n bytes, returned as it is"""
        sp, n, _k0 = self._peer_slots(slots, n)
        hp, _k1 = None, None
        if hs is not None:
            hp, nh, _k1 = self._records("fingerprint", hs, n, 32)
            if nh != n:
                raise KoskError("regtree_check_paths: %d slots, %d fingerprints" % (n, nh))
        pp, _k2 = None, None
        if paths is not None:
            pp, np_, _k2 = self._records("path", paths, n, 32 * depth)
            if np_ != n:
                raise KoskError("regtree_check_paths: %d slots, %d paths" % (n, np_))
        stp, _k3 = None, None
        if states is not None:
            if isinstance(states, int):
                stp = C.c_void_p(states)
            else:
                if len(states) != n:
                    raise KoskError("regtree_check_paths: %d slots, %d states" % (n, len(states)))
                _k3 = bytes(1 if s_ else 0 for s_ in states)
                stp = C.c_char_p(_k3)
        rp, _k4 = self._peer_root(root)
        ok = C.create_string_buffer(max(n, 1)) if out is None else C.c_void_p(int(out))
        self._chk(lib.kosk_regtree_check_paths(self._h, n, depth, sp, stp, hp, pp, rp, ok), "regtree_check_paths")
        return list(ok.raw[:n]) if out is None else out

    def regsort_check_proofs(self, depth, xs, records, root, out=None, n=None):
        """kosk_regsort_check_proofs -> [verdict]: per item what records[b] proves about xs[b] under root: REGSORT_NEITHER, REGSORT_ABSENT
        or REGSORT_PRESENT.  xs: a list of 32-byte strings; records: a list of regsort_proof_bytes(depth)-byte strings; either may be an
        int pointer to host or DEVICE memory (with n).  out: an int pointer to n bytes, returned as it is"""
        xp, n, _k0 = self._records("fingerprint", xs, n, 32)
        cp, nr, _k1 = self._records("proof record", records, n, regsort_proof_bytes(depth))
        if nr != n:
            raise KoskError("regsort_check_proofs: %d fingerprints, %d records" % (n, nr))
        rp, _k2 = self._peer_root(root)
        v = C.create_string_buffer(max(n, 1)) if out is None else C.c_void_p(int(out))
        self._chk(lib.kosk_regsort_check_proofs(self._h, n, depth, xp, cp, rp, v), "regsort_check_proofs")
        return list(v.raw[:n]) if out is None else out

    def kem_enc_proven(self, depth, pks, slots, paths, root, coins=None, out=None, n=None):
        """kosk_kem_enc_proven: encapsulate to pks[b] iff (slots[b], SHA3-256(pks[b]), paths[b]) walks to root; the check and the mask stay
        on the device.  Inputs as in regtree_check_paths / kem_enc.  Returns (cts, sss, done); ct and ss of an item whose path fails are
        zero-filled.  out=(d_ct, d_ss, d_done): int DEVICE pointers, returned as they are"""
        pp, n, _k0 = self._records("pk", pks, n, self.pk_bytes)
        sp, ns, _k1 = self._peer_slots(slots, n)
        if ns != n:
            raise KoskError("kem_enc_proven: %d public keys, %d slots" % (n, ns))
        tp, _k2 = None, None
        if paths is not None:
            tp, np_, _k2 = self._records("path", paths, n, 32 * depth)
            if np_ != n:
                raise KoskError("kem_enc_proven: %d public keys, %d paths" % (n, np_))
        cp, _k3 = None, None
        if coins is not None:
            cp, nc, _k3 = self._records("coins", coins, n, 32)
            if nc != n:
                raise KoskError("coins for %d items, public keys for %d" % (nc, n))
        rp, _k4 = self._peer_root(root)
        ctb = ct_bytes(self.k)
        bufs, host = self._kem_out(out, n, (ctb, SS_BYTES, 1))
        self._chk(lib.kosk_kem_enc_proven(self._h, n, depth, pp, sp, tp, rp, cp, bufs[0], bufs[1], bufs[2]), "kem_enc_proven")
        if host is None:
            return out
        return _cut(bufs[0], ctb, n), _cut(bufs[1], SS_BYTES, n), [bool(x) for x in bufs[2].raw[:n]]

    # signed heads, kosk-headsig-v1
    def registry_signer_reserve(self, height, seed=None, key_id=None, out=None):
        """kosk_registry_signer_reserve -> the 52-byte public key: builds the 2^height one-time keys and their tree in HBM on a handle with a
        history; height 0 frees (and returns None).  seed (32 bytes) and key_id (16 bytes) may be int pointers to host or DEVICE memory;
        out: an int DEVICE pointer to 52 bytes, returned in place of the key"""
        if height == 0:
            self._chk(lib.kosk_registry_signer_reserve(self._h, 0, None, None, None), "registry_signer_reserve")
            return None
        sp = C.c_void_p(seed) if isinstance(seed, int) else C.c_char_p(bytes(seed))
        ip_ = C.c_void_p(key_id) if isinstance(key_id, int) else C.c_char_p(bytes(key_id))
        if not isinstance(seed, int) and len(bytes(seed)) != 32 or not isinstance(key_id, int) and len(bytes(key_id)) != 16:
            raise KoskError("a seed has 32 bytes and a key identifier 16")
        buf = C.create_string_buffer(HEADSIG_PUB_BYTES) if out is None else C.c_void_p(int(out))
        self._chk(lib.kosk_registry_signer_reserve(self._h, height, sp, ip_, buf), "registry_signer_reserve")
        return buf.raw if out is None else out

    def registry_signer_level(self):
        """kosk_registry_signer_level -> (height, has_seed); height 0: no signer"""
        h, s_ = C.c_int(), C.c_int()
        self._chk(lib.kosk_registry_signer_level(self._h, C.byref(h), C.byref(s_)), "registry_signer_level")
        return h.value, bool(s_.value)

    def registry_history_sign_head(self, size=-1, out=None):
        """kosk_registry_history_sign_head -> (sig, root, size): the head over the first `size` events (< 0: all) signed with leaf `size`.
        out=(d_sig, d_root): int DEVICE pointers, returned in place of the bytes"""
        h = self.registry_signer_level()[0]
        n = C.c_int()
        if out is None:
            sig, root = C.create_string_buffer(max(headsig_sig_bytes(h), 1)), C.create_string_buffer(32)
        else:
            sig, root = C.c_void_p(int(out[0])), C.c_void_p(int(out[1]))
        self._chk(lib.kosk_registry_history_sign_head(self._h, size, sig, root, C.byref(n)), "registry_history_sign_head")
        if out is None:
            return sig.raw[:headsig_sig_bytes(h)], root.raw, n.value
        return out[0], out[1], n.value

    def headsig_verify_heads(self, pub, roots, sizes, sigs, out=None, n=None):
        """kosk_headsig_verify_heads -> [ok]: item b is 1 iff headsig_verify(pub, k, roots[b], sizes[b], sigs[b]).  roots, sizes and sigs
        are lists or int pointers to host or DEVICE memory (with n); out: an int pointer to n bytes, returned as it is"""
        pub, h = _headsig_height(pub)
        rp, n, _k0 = self._records("root", roots, n, 32)
        zp, ns, _k1 = self._peer_slots(sizes, n)
        gp, ng, _k2 = self._records("signature", sigs, n, headsig_sig_bytes(h))
        if ns != n or ng != n:
            raise KoskError("headsig_verify_heads: %d roots, %d sizes, %d signatures" % (n, ns, ng))
        ok = C.create_string_buffer(max(n, 1)) if out is None else C.c_void_p(int(out))
        self._chk(lib.kosk_headsig_verify_heads(self._h, n, C.c_char_p(pub), rp, zp, gp, ok), "headsig_verify_heads")
        return list(ok.raw[:n]) if out is None else out

    # proofs for keys that already exist
    def witness_from_sk(self, sks, n=None):
        """kosk_witness_from_sk: the prover's witness of n secret keys (list of bytes, or an int DEVICE pointer with n), left resident.
        Returns (se, ok): se an int16 ndarray [n, 2K, 256], s then e per key, all zero where ok is False."""
        import numpy as np
        sp, n, _keep = self._records("sk", sks, n, self.sk_bytes)
        se = np.zeros((n, 2 * self.k, 256), np.int16)
        ok = C.create_string_buffer(n)
        self._chk(lib.kosk_witness_from_sk(self._h, n, sp, se.ctypes.data, ok), "witness_from_sk")
        return se, [b == 1 for b in ok.raw[:n]]

    def _key_rand(self, tapes, seeds, n, seed_stride):
        """the randomness arguments of the *_keys calls -> (seeded, pointer, stride, keepalive)"""
        if seeds is not None:
            sp, ss, ns, keep = self._seed_arg(seeds, n, seed_stride)
            if ns != n:
                raise KoskError("seeds for %d proofs, secret keys for %d" % (ns, n))
            return True, sp, ss, keep
        if tapes is None:
            return False, None, 0, None
        if isinstance(tapes, int):
            return False, C.c_void_p(tapes), self.tape_bytes, None
        if len(tapes) != n:
            raise KoskError("tapes for %d proofs, secret keys for %d" % (len(tapes), n))
        for t in tapes:
            if len(t) < self.tape_bytes:
                raise KoskError("tape shorter than kosk_tape_bytes")
        blob = b"".join(t[:self.tape_bytes] for t in tapes)
        return False, C.c_char_p(blob), self.tape_bytes, blob

    def stage_prover_keys(self, sks, tapes=None, seeds=None, n=None, seed_stride=None, derived=False, salts=None, salt_stride=None):
        """kosk_stage_prover_keys[_seeded|_derived]: witness and randomness of n existing keys resident for prove_resident(n).  tapes: list
        of bytes, an int DEVICE pointer (kosk_tape_bytes apart) or None; seeds: see _seed_arg; neither: the handle's entropy mode.
        derived=True (kosk-keyseed-v1): the randomness is derived from the keys on the device; salts: see _salt_arg.
        Returns ok (list of bool)."""
        sp, n, _k1 = self._records("sk", sks, n, self.sk_bytes)
        if derived or salts is not None:
            if tapes is not None or seeds is not None:
                raise KoskError("derived=True takes neither tapes nor seeds")
            rp, stride, _k2 = self._salt_arg(salts, n, salt_stride)
            ok = C.create_string_buffer(n)
            self._chk(lib.kosk_stage_prover_keys_derived(self._h, n, sp, rp, stride, ok), "stage_prover_keys")
            return [b == 1 for b in ok.raw[:n]]
        seeded, rp, stride, _k2 = self._key_rand(tapes, seeds, n, seed_stride)
        ok = C.create_string_buffer(n)
        fn = lib.kosk_stage_prover_keys_seeded if seeded else lib.kosk_stage_prover_keys
        self._chk(fn(self._h, n, sp, rp, stride, ok), "stage_prover_keys")
        return [b == 1 for b in ok.raw[:n]]

    def prove_keys(self, sks, tapes=None, seeds=None, n=None, seed_stride=None, derived=False, salts=None, salt_stride=None):
        """kosk_prove_keys[_seeded|_derived]_batch: one proof per existing key, any n.  derived / salts: as stage_prover_keys.
        Returns (proofs, ok); the image of a key with ok False is all zero."""
        sp, n, _k1 = self._records("sk", sks, n, self.sk_bytes)
        if derived or salts is not None:
            if tapes is not None or seeds is not None:
                raise KoskError("derived=True takes neither tapes nor seeds")
            rp, stride, _k2 = self._salt_arg(salts, n, salt_stride)
            ok = C.create_string_buffer(n)
            pi = C.create_string_buffer(self.proof_bytes * n)
            self._chk(lib.kosk_prove_keys_derived_batch(self._h, n, sp, rp, stride, pi, ok), "prove_keys")
            return _cut(pi, self.proof_bytes, n), [b == 1 for b in ok.raw[:n]]
        seeded, rp, stride, _k2 = self._key_rand(tapes, seeds, n, seed_stride)
        ok = C.create_string_buffer(n)
        pi = C.create_string_buffer(self.proof_bytes * n)
        fn = lib.kosk_prove_keys_seeded_batch if seeded else lib.kosk_prove_keys_batch
        self._chk(fn(self._h, n, sp, rp, stride, pi, ok), "prove_keys")
        return _cut(pi, self.proof_bytes, n), [b == 1 for b in ok.raw[:n]]

    # the offline bank
    def bank_reserve(self, capacity):
        self._chk(lib.kosk_bank_reserve(self._h, int(capacity)), "bank_reserve")

    def bank_level(self):
        """kosk_bank_level -> (ready, capacity)"""
        r, c_ = C.c_int(), C.c_int()
        self._chk(lib.kosk_bank_level(self._h, C.byref(r), C.byref(c_)), "bank_level")
        return r.value, c_.value

    def _bank_rand(self, tapes, seeds, n, seed_stride):
        """the randomness arguments of the bank calls -> (tapes pointer, tape stride, seeds pointer, seed stride, keepalive)"""
        seeded, rp, stride, keep = self._key_rand(tapes, seeds, n, seed_stride)
        return (None, 0, rp, stride, keep) if seeded else (rp, stride, None, 0, keep)

    def bank_fill(self, n=None, tapes=None, seeds=None, seed_stride=None):
        """kosk_bank_fill: n entries from tapes (list of bytes, or an int DEVICE pointer with n), seeds (see _seed_arg) or, with neither,
        the handle's entropy mode"""
        if n is None:
            n = len(tapes if tapes is not None else seeds)
        tp, ts, sp, ss, _keep = self._bank_rand(tapes, seeds, n, seed_stride)
        self._chk(lib.kosk_bank_fill(self._h, n, tp, ts, sp, ss), "bank_fill")

    def stage_prover_keys_banked(self, sks, tapes=None, seeds=None, n=None, seed_stride=None):
        """kosk_stage_prover_keys_banked: as stage_prover_keys, on the n oldest bank entries; then prove_resident(n).  Returns ok"""
        kp, n, _k1 = self._records("sk", sks, n, self.sk_bytes)
        tp, ts, sp, ss, _keep = self._bank_rand(tapes, seeds, n, seed_stride)
        ok = C.create_string_buffer(n)
        self._chk(lib.kosk_stage_prover_keys_banked(self._h, n, kp, tp, ts, sp, ss, ok), "stage_prover_keys_banked")
        return [b == 1 for b in ok.raw[:n]]

    def prove_keys_banked(self, sks, tapes=None, seeds=None, n=None, seed_stride=None):
        """kosk_prove_keys_banked_batch: as prove_keys, on the n oldest bank entries.  Returns (proofs, ok)"""
        kp, n, _k1 = self._records("sk", sks, n, self.sk_bytes)
        tp, ts, sp, ss, _keep = self._bank_rand(tapes, seeds, n, seed_stride)
        ok = C.create_string_buffer(n)
        pi = C.create_string_buffer(self.proof_bytes * n)
        self._chk(lib.kosk_prove_keys_banked_batch(self._h, n, kp, tp, ts, sp, ss, pi, ok), "prove_keys_banked")
        return _cut(pi, self.proof_bytes, n), [b == 1 for b in ok.raw[:n]]

    def verifiable_keygen_banked(self, n=None, tapes=None, seeds=None, seed_stride=None):
        """kosk_verifiable_keygen_banked_batch: as verifiable_keygen, on the n oldest bank entries.  Returns (pks, sks, proofs)"""
        if n is None:
            n = len(tapes if tapes is not None else seeds)
        tp, ts, sp, ss, _keep = self._bank_rand(tapes, seeds, n, seed_stride)
        pk = C.create_string_buffer(self.pk_bytes * n)
        sk = C.create_string_buffer(self.sk_bytes * n)
        pi = C.create_string_buffer(self.proof_bytes * n)
        self._chk(lib.kosk_verifiable_keygen_banked_batch(self._h, n, tp, ts, sp, ss, pk, sk, pi), "verifiable_keygen_banked")
        return _cut(pk, self.pk_bytes, n), _cut(sk, self.sk_bytes, n), _cut(pi, self.proof_bytes, n)

    def bank_timing(self, n, reps=20):
        """kosk_bank_timing -> dict(put_ms, take_ms, copy_ms, copy_fill_ms, bytes)"""
        v = [C.c_double() for _ in range(4)]
        nb = C.c_size_t()
        self._chk(lib.kosk_bank_timing(self._h, n, reps, *[C.byref(x) for x in v], C.byref(nb)), "bank_timing")
        return dict(put_ms=v[0].value, take_ms=v[1].value, copy_ms=v[2].value, copy_fill_ms=v[3].value, bytes=nb.value)

    PATH_IDS = ["hash_dma", "hash_plain", "table_gemm", "limb_gemm", "copy_direct", "copy_staged", "graph_replay", "digest_copy", "small_copy_kernel",
                "fs_device", "fs_host", "tape_expand", "kem_enc", "kem_dec"]

    # ids behind PATH_IDS (that list is what path_counts() walks and stays as it is)
    PATH_DENSE_FILL = 14
    PATH_KEM_KEYPAIR = 15
    PATH_KEM_CHECK = 16
    PATH_KEYSEED = 17
    PATH_WIPE = 18
    PATH_KEM_KEY_SETUP = 19
    PATH_KEM_ENC_KEY = 20
    PATH_KEM_DEC_KEY = 21
    PATH_DENSE_CHECK = 22
    PATH_DENSE2_FILL = 23
    PATH_DENSE2_CHECK = 24
    PATH_BANK_PUT = 25
    PATH_BANK_TAKE = 26
    PATH_REGISTRY_ADMIT = 27
    PATH_KEM_ENC_SLOTS = 28
    PATH_REGISTRY_INDEX = 29
    PATH_REGISTRY_FIND = 30
    PATH_KEM_ENC_PEERS = 31
    PATH_REGISTRY_TREE = 32
    PATH_REGISTRY_SUBTREES = 33
    PATH_REGISTRY_PATH = 34
    PATH_REGSORT_SORT = 35
    PATH_REGSORT_TREE = 36
    PATH_REGSORT_PROVE = 37
    PATH_REGHIST_APPEND = 38
    PATH_REGHIST_GROUPS = 39
    PATH_REGHIST_FRONTIER = 40
    PATH_REGHIST_PROVE = 41
    PATH_MONITOR_KEYS = 42
    PATH_MONITOR_APPLY = 43
    PATH_MONITOR_LEAVES = 44
    PATH_MONITOR_CHECK = 45
    PATH_REGTREE_CHECK = 46  # launches of k_regtree_check (kosk_regtree_check_paths, kosk_kem_enc_proven)
    PATH_REGSORT_CHECK = 47  # launches of k_regsort_check
    PATH_KEM_ENC_PROVEN = 48  # encapsulation launches of kosk_kem_enc_proven
    PATH_HEADSIG_LEAVES = 49  # launches of k_headsig_leaves (kosk_registry_signer_reserve)
    PATH_HEADSIG_TREE = 50  # launches of k_headsig_tree, one per tier
    PATH_HEADSIG_SIGN = 51  # launches of k_headsig_sign
    PATH_HEADSIG_VERIFY = 52  # launches of k_headsig_verify, one per launch group

    def path_count(self, path_id):
        """one counter of kosk_path_count by number, e.g. PATH_DENSE_FILL: refills of the dense wire format"""
        v = C.c_long()
        self._chk(lib.kosk_path_count(self._h, int(path_id), C.byref(v)), "path_count")
        return v.value

    def path_counts(self):
        """{name: launches / copies} of the alternative kernel and copy paths on this handle since it was created"""
        out = {}
        for i, name in enumerate(self.PATH_IDS if HAS_KEM else self.PATH_IDS[:12]):
            v = C.c_long()
            self._chk(lib.kosk_path_count(self._h, i, C.byref(v)), "path_count")
            out[name] = v.value
        return out

    @property
    def host_threads(self):
        return lib.kosk_host_threads(self._h)

    def timer_start(self):
        self._chk(lib.kosk_stream_timer_start(self._h), "timer_start")

    def timer_stop_ms(self):
        ms = C.c_double()
        self._chk(lib.kosk_stream_timer_stop(self._h, C.byref(ms)), "timer_stop")
        return ms.value

    @property
    def streams(self):
        return lib.kosk_streams(self._h)

    def synchronize(self):
        self._chk(lib.kosk_device_synchronize(self._h), "synchronize")

    # kernel-level (device pointers as ints, e.g. torch tensor .data_ptr())
    def sha3_256_batch(self, d_in, in_stride, inlen, d_out, n):
        self._chk(lib.kosk_sha3_256_batch(self._h, d_in, in_stride, inlen, d_out, n), "sha3_256_batch")

    def sha3_256_batch_pair(self, d_in, in_stride, inlen, d_out, n):
        self._chk(lib.kosk_sha3_256_batch_pair(self._h, d_in, in_stride, inlen, d_out, n), "sha3_256_batch_pair")

    def sha3_256_batch_wave(self, d_in, in_stride, inlen, d_out, n):
        self._chk(lib.kosk_sha3_256_batch_wave(self._h, d_in, in_stride, inlen, d_out, n), "sha3_256_batch_wave")

    def fs_alpha_device(self, d_tables, table_stride, n, d_alpha, d_h1=None):
        self._chk(lib.kosk_fs_alpha_device(self._h, d_tables, table_stride, n, d_alpha, d_h1), "fs_alpha_device")

    def fs_opened_device(self, d_tables, table_stride, n, d_sel, d_rest, sel_stride, d_ch=None):
        self._chk(lib.kosk_fs_opened_device(self._h, d_tables, table_stride, n, d_sel, d_rest, sel_stride, d_ch), "fs_opened_device")

    def fs_alpha_bound_device(self, d_tables, table_stride, n, d_bind, d_alpha, d_h1=None):
        self._chk(lib.kosk_fs_alpha_bound_device(self._h, d_tables, table_stride, n, d_bind, d_alpha, d_h1), "fs_alpha_bound_device")

    def fs_opened_bound_device(self, d_tables, table_stride, n, d_bind, d_sel, d_rest, sel_stride, d_ch=None):
        self._chk(lib.kosk_fs_opened_bound_device(self._h, d_tables, table_stride, n, d_bind, d_sel, d_rest, sel_stride, d_ch), "fs_opened_bound_device")

    def shake256_batch(self, d_in, in_stride, inlen, d_out, outlen, n):
        self._chk(lib.kosk_shake256_batch(self._h, d_in, in_stride, inlen, d_out, outlen, n), "shake256_batch")

    def commit_hash_lanes(self, d_rows, row_stride, n_lanes, d_prefix, with_prefix, d_out):
        self._chk(lib.kosk_commit_hash_lanes(self._h, d_rows, row_stride, n_lanes, d_prefix, int(with_prefix), d_out), "commit_hash_lanes")

    def ntt256_batch(self, d_in, d_out, n):
        self._chk(lib.kosk_ntt256_batch(self._h, d_in, d_out, n), "ntt256_batch")

    def lagrange_expand(self, d_y407, d_shares, n):
        self._chk(lib.kosk_lagrange_expand(self._h, d_y407, d_shares, n), "lagrange_expand")

    def recon_secrets(self, d_shares, d_secrets, n, two_d=False):
        self._chk(lib.kosk_recon_secrets(self._h, d_shares, d_secrets, n, int(two_d)), "recon_secrets")
