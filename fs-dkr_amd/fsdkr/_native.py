"""ctypes binding of libfsdkr.so (include/fsdkr/fsdkr.h).

The product path is the HIP library: loading fails loudly if it is missing,
and there is no CPU fallback anywhere in this package."""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# FSDKR_LIB: alternative build of the same library (A/B timing tools only)
LIB_PATH = os.environ.get("FSDKR_LIB") or os.path.join(_HERE, "libfsdkr.so")

FSDKR_OK = 0
FSDKR_E_ARG = -1
FSDKR_E_HIP = -2
FSDKR_E_OOM = -3
FSDKR_E_UNSUPPORTED = -4
FSDKR_CFG_TIMING = 1
# algorithm switches (parity tests, A/B runs; results identical under each)
FSDKR_CFG_FB_BGMW = 2    # fixed-base exponentiations by BGMW windows only
FSDKR_CFG_FB_COMB = 4    # a Lim-Lee comb wherever one fits
FSDKR_CFG_INV_EACH = 8   # one inverse per element (no simultaneous inversion)
FSDKR_CFG_GA_FULLWIDTH = 16   # GA's head as a generic 4096-bit chain (not half-width N-adic)
FSDKR_CFG_GA_TAIL_FULLWIDTH = 32   # the N-adic head's tail at full width over its own tables

u32p = ctypes.POINTER(ctypes.c_uint32)


class FsdkrError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"fsdkr error {code}: {msg}")
        self.code = code


class _Cfg(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int32), ("flags", ctypes.c_uint32)]


class CollectBatchC(ctypes.Structure):
    """struct fsdkr_collect_batch (include/fsdkr/fsdkr.h)."""
    _fields_ = [(f, ctypes.c_uint32) for f in ("n_refresh", "n_join", "t", "m_security", "key_bits", "nl",
                                               "s1l", "s3l", "el", "zl", "yl")] + \
               [(f, u32p) for f in ("party_index", "msg_lens", "recv_n", "recv_ntilde", "recv_h1", "recv_h2",
                                    "enc", "commit", "pdl_z", "pdl_u3", "pdl_s2", "pdl_u1", "pdl_u2", "pdl_s1",
                                    "pdl_s3", "rp_z", "rp_s", "rp_e", "rp_s1", "rp_s2", "vss", "ped_S", "ped_T",
                                    "ped_N", "ped_A", "ped_Z", "ck_n", "ck_sigma", "dlog_N", "dlog_g", "dlog_ni",
                                    "dlog_x1", "dlog_x2", "dlog_y1", "dlog_y2")] + [("n_recv", ctypes.c_uint32)] + \
               [("vss_len", u32p), ("range_lens", u32p), ("ckl", ctypes.c_uint32), ("recv_avail", ctypes.c_uint32),
                ("ped_lens", u32p), ("ck_lens", u32p), ("pdl_s3_neg", ctypes.POINTER(ctypes.c_uint8)),
                ("neg_bits", ctypes.POINTER(ctypes.c_uint8)), ("ped_a_neg", ctypes.POINTER(ctypes.c_uint8))]


u8p = ctypes.POINTER(ctypes.c_uint8)


class VerdictsC(ctypes.Structure):
    _fields_ = [(f, u8p) for f in ("feldman", "pdl", "range", "ped", "ck", "dlog")] + \
               [(f, ctypes.c_uint32) for f in ("cap_pairs", "cap_msgs", "cap_joins")]


class BobBatchC(ctypes.Structure):
    """struct fsdkr_bob_batch (include/fsdkr/fsdkr.h)."""
    _fields_ = [(f, ctypes.c_uint32) for f in ("count", "n_keys", "nl", "el", "s1l", "s2l", "t1l", "t2l")] + \
               [(f, u32p) for f in ("N", "Ntilde", "h1", "h2", "key_idx", "a_enc", "mta", "z", "t", "s", "e",
                                    "s1", "s2", "t1", "t2", "X", "u")]


class AliceBatchC(ctypes.Structure):
    """struct fsdkr_alice_batch (include/fsdkr/fsdkr.h)."""
    _fields_ = [(f, ctypes.c_uint32) for f in ("count", "n_keys", "nl", "el", "s1l", "s2l")] + \
               [(f, u32p) for f in ("N", "Ntilde", "h1", "h2", "key_idx", "cipher", "z", "s", "e", "s1", "s2")]


class BobProveC(ctypes.Structure):
    """struct fsdkr_bob_prove_batch (include/fsdkr/fsdkr.h)."""
    SECRET = ("b", "beta_prim", "r", "alpha", "beta", "gamma", "gamma_mod_n", "ro", "ro_prim", "sigma", "tau")
    _fields_ = [(f, ctypes.c_uint32) for f in ("count", "n_keys", "nl")] + \
               [(f, u32p) for f in ("N", "Ntilde", "h1", "h2", "key_idx", "a_enc", "mta") + SECRET]


class BobProofsC(ctypes.Structure):
    """struct fsdkr_bob_proofs."""
    _fields_ = [(f, u32p) for f in ("z", "t", "s", "e", "s1", "s2", "t1", "t2")]


class AliceProveC(ctypes.Structure):
    """struct fsdkr_alice_prove_batch."""
    SECRET = ("a", "r", "alpha", "beta", "gamma", "ro")
    _fields_ = [(f, ctypes.c_uint32) for f in ("count", "n_keys", "nl")] + \
               [(f, u32p) for f in ("N", "Ntilde", "h1", "h2", "key_idx", "cipher") + SECRET]


class AliceProofsC(ctypes.Structure):
    """struct fsdkr_alice_proofs."""
    _fields_ = [(f, u32p) for f in ("z", "s", "e", "s1", "s2")]


def bob_prove_widths(nl):
    """Limbs of every row of fsdkr_bob_prove in the width class nl: the inputs, then
    the outputs (limbs(e x + y) = max(xl + 8, yl) + 1)."""
    return ({"b": 8, "beta_prim": nl, "r": nl, "alpha": 24, "beta": nl, "gamma": nl + 16, "gamma_mod_n": nl,
             "ro": nl + 8, "ro_prim": nl + 24, "sigma": nl + 8, "tau": nl + 24},
            {"z": nl, "t": nl, "s": nl, "e": 8, "s1": 25, "s2": nl + 25, "t1": nl + 17, "t2": nl + 25})


def alice_prove_widths(nl):
    """Limbs of every row of fsdkr_alice_prove in the width class nl."""
    return ({"a": 24, "r": nl, "alpha": 24, "beta": nl, "gamma": nl + 24, "ro": nl + 8},
            {"z": nl, "s": nl, "e": 8, "s1": 33, "s2": nl + 25})


class RecoverJobC(ctypes.Structure):
    _fields_ = [("nl", ctypes.c_uint32), ("t_vss", ctypes.c_uint32), ("t_key", ctypes.c_uint32),
                ("n_new", ctypes.c_uint32), ("old_index", u32p), ("cts", u32p), ("p", u32p), ("q", u32p),
                ("points", u32p), ("flags", ctypes.c_uint32)]


class RecoveredC(ctypes.Structure):
    _fields_ = [("share", ctypes.c_uint32 * 8), ("y", ctypes.c_uint32 * 16), ("pk_vec", u32p),
                ("status", ctypes.c_int32)]


def _struct_dtype(cls):
    """numpy structured dtype with the exact layout of a ctypes Structure (pointers as u8)."""
    names, formats, offsets = [], [], []
    for name, typ in cls._fields_:
        names.append(name)
        formats.append(np.uint64 if ctypes.sizeof(typ) == 8 else np.uint32)
        offsets.append(getattr(cls, name).offset)
    return np.dtype({"names": names, "formats": formats, "offsets": offsets, "itemsize": ctypes.sizeof(cls)})


_RECOVER_DT = _struct_dtype(RecoverJobC)
_RECOVERED_DT = np.dtype({"names": ["pk_vec", "status"], "formats": [np.uint64, np.int32],
                          "offsets": [RecoveredC.pk_vec.offset, RecoveredC.status.offset],
                          "itemsize": ctypes.sizeof(RecoveredC)})
RECOVER_OK, RECOVER_PANIC_LI, RECOVER_PANIC_DECRYPT = 0, 1, 2
RECOVER_NO_DECRYPT = 1   # fsdkr_recover_job.flags
DRAW_BITS_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32),
                                ctypes.c_uint32)


class ErrorC(ctypes.Structure):
    _fields_ = [("variant", ctypes.c_int32), ("panic", ctypes.c_int32), ("f", ctypes.c_uint32 * 4),
                ("keys_applied", ctypes.c_uint32)]


_lib = None


def lib():
    """Load libfsdkr.so.  Raises (never falls back) if the HIP library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} missing: run __graft_entry__.build() (no CPU fallback exists)")
    L = ctypes.CDLL(LIB_PATH)
    vp = ctypes.c_void_p
    L.fsdkr_ctx_create.argtypes = [ctypes.POINTER(_Cfg), ctypes.POINTER(vp)]
    L.fsdkr_ctx_create.restype = ctypes.c_int
    L.fsdkr_collect_recover.argtypes = [vp, ctypes.POINTER(RecoverJobC), ctypes.c_uint32,
                                        ctypes.POINTER(RecoveredC)]
    L.fsdkr_collect_recover.restype = ctypes.c_int
    L.fsdkr_collect_recover_launch.argtypes = [vp, ctypes.POINTER(RecoverJobC), ctypes.c_uint32]
    L.fsdkr_collect_recover_launch.restype = ctypes.c_int
    L.fsdkr_collect_recover_finish.argtypes = [vp, ctypes.POINTER(RecoveredC)]
    L.fsdkr_collect_recover_finish.restype = ctypes.c_int
    L.fsdkr_sample_primes.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                      DRAW_BITS_FN, vp, u32p, ctypes.c_uint32]
    L.fsdkr_sample_primes.restype = ctypes.c_int
    L.fsdkr_ctx_destroy.argtypes = [vp]
    L.fsdkr_ctx_destroy.restype = None
    L.fsdkr_last_error.argtypes = [vp]
    L.fsdkr_last_error.restype = ctypes.c_char_p
    L.fsdkr_device_available.argtypes = []
    L.fsdkr_device_available.restype = ctypes.c_int
    L.fsdkr_modexp_batch.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, u32p, u32p, ctypes.c_uint32, u32p, u32p,
                                     ctypes.c_uint32, u32p]
    L.fsdkr_modexp_batch.restype = ctypes.c_int
    L.fsdkr_modexp_batch_ct.argtypes = L.fsdkr_modexp_batch.argtypes
    L.fsdkr_modexp_joint_batch.argtypes = [vp, ctypes.c_uint32, u32p, u32p, u32p, u32p, u32p, u32p, ctypes.c_uint32,
                                           ctypes.c_uint32, u32p]
    L.fsdkr_modexp_joint_batch.restype = ctypes.c_int
    L.fsdkr_modexp_nadic_batch.argtypes = L.fsdkr_modexp_joint_batch.argtypes
    L.fsdkr_modexp_nadic_batch.restype = ctypes.c_int
    L.fsdkr_modexp_joint3_batch.argtypes = [vp, ctypes.c_uint32, u32p, u32p, u32p, ctypes.c_uint32, u32p, u32p, u32p,
                                            u32p, u32p, ctypes.c_uint32, ctypes.c_uint32, u32p]
    L.fsdkr_modexp_joint3_batch.restype = ctypes.c_int
    L.fsdkr_modexp_joint3_batch_k.argtypes = [vp, ctypes.c_uint32] + L.fsdkr_modexp_joint3_batch.argtypes[1:]
    L.fsdkr_modexp_joint3_batch_k.restype = ctypes.c_int
    L.fsdkr_bob_verify.argtypes = [vp, ctypes.POINTER(BobBatchC), u8p]
    L.fsdkr_bob_verify.restype = ctypes.c_int
    L.fsdkr_bob_verify_unfused.argtypes = L.fsdkr_bob_verify.argtypes
    L.fsdkr_bob_verify_unfused.restype = ctypes.c_int
    L.fsdkr_modexp_batch_ct.restype = ctypes.c_int
    L.fsdkr_mta_respond.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, u32p, u32p, u32p, u32p, u32p, u32p,
                                    ctypes.c_uint32, u32p]
    L.fsdkr_mta_respond.restype = ctypes.c_int
    L.fsdkr_mta_respond_unfused.argtypes = L.fsdkr_mta_respond.argtypes
    L.fsdkr_mta_respond_unfused.restype = ctypes.c_int
    L.fsdkr_bob_commit_v.argtypes = L.fsdkr_mta_respond.argtypes
    L.fsdkr_bob_commit_v.restype = ctypes.c_int
    L.fsdkr_bob_commit_v_unfused.argtypes = L.fsdkr_mta_respond.argtypes
    L.fsdkr_bob_commit_v_unfused.restype = ctypes.c_int
    L.fsdkr_alice_verify.argtypes = [vp, ctypes.POINTER(AliceBatchC), u8p]
    L.fsdkr_alice_verify.restype = ctypes.c_int
    L.fsdkr_pedersen_commit_ct.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, u32p, ctypes.c_uint32, u32p,
                                           ctypes.c_uint32, u32p, u32p, u32p, u32p, ctypes.c_uint32, u32p]
    L.fsdkr_pedersen_commit_ct.restype = ctypes.c_int
    L.fsdkr_modexp_batch_device.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, vp, vp, ctypes.c_uint32,
                                            ctypes.c_uint32, vp, vp, ctypes.c_uint32, vp]
    L.fsdkr_modexp_batch_device.restype = ctypes.c_int
    L.fsdkr_modexp_keyed_device.argtypes = L.fsdkr_modexp_batch_device.argtypes
    L.fsdkr_modexp_keyed_device.restype = ctypes.c_int
    L.fsdkr_kernel_time.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_double),
                                    ctypes.POINTER(ctypes.c_uint32)]
    L.fsdkr_kernel_time.restype = ctypes.c_int
    L.fsdkr_kernel_time_reset.argtypes = [vp]
    L.fsdkr_kernel_time_reset.restype = None
    L.fsdkr_verify_collect.argtypes = [vp, ctypes.POINTER(CollectBatchC), ctypes.POINTER(VerdictsC)]
    L.fsdkr_verify_collect.restype = ctypes.c_int
    L.fsdkr_collect_prepare.argtypes = [vp, ctypes.POINTER(CollectBatchC)]
    L.fsdkr_collect_prepare.restype = ctypes.c_int
    L.fsdkr_collect_run.argtypes = [vp, ctypes.POINTER(VerdictsC)]
    L.fsdkr_collect_run.restype = ctypes.c_int
    L.fsdkr_collect_launch.argtypes = [vp]
    L.fsdkr_collect_launch.restype = ctypes.c_int
    L.fsdkr_collect_prestart.argtypes = [vp, ctypes.POINTER(CollectBatchC)]
    L.fsdkr_collect_prestart.restype = ctypes.c_int
    L.fsdkr_collect_last_span_ms.argtypes = [vp]
    L.fsdkr_collect_last_span_ms.restype = ctypes.c_double
    L.fsdkr_collect_reuse_mask.argtypes = [vp]
    L.fsdkr_collect_reuse_mask.restype = ctypes.c_uint32
    L.fsdkr_collect_finish.argtypes = [vp, ctypes.POINTER(VerdictsC)]
    L.fsdkr_collect_finish.restype = ctypes.c_int
    L.fsdkr_collect_prepare_multi.argtypes = [vp, ctypes.POINTER(CollectBatchC), ctypes.c_uint32]
    L.fsdkr_collect_prepare_multi.restype = ctypes.c_int
    L.fsdkr_collect_prestart_multi.argtypes = [vp, ctypes.POINTER(CollectBatchC), ctypes.c_uint32]
    L.fsdkr_collect_prestart_multi.restype = ctypes.c_int
    L.fsdkr_collect_prestart_rp.argtypes = [vp, ctypes.POINTER(CollectBatchC), ctypes.c_uint32]
    L.fsdkr_collect_prestart_rp.restype = ctypes.c_int
    L.fsdkr_collect_finish_multi.argtypes = [vp, ctypes.POINTER(VerdictsC), ctypes.c_uint32]
    L.fsdkr_collect_finish_multi.restype = ctypes.c_int
    L.fsdkr_verify_collect_multi.argtypes = [vp, ctypes.POINTER(CollectBatchC), ctypes.c_uint32,
                                             ctypes.POINTER(VerdictsC)]
    L.fsdkr_verify_collect_multi.restype = ctypes.c_int
    L.fsdkr_paillier_decrypt_multi.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, u32p, u32p, u32p, u32p,
                                               ctypes.c_uint32, u32p]
    L.fsdkr_paillier_decrypt_multi.restype = ctypes.c_int
    L.fsdkr_collect_first_error.argtypes = [ctypes.POINTER(CollectBatchC), ctypes.POINTER(VerdictsC),
                                            ctypes.POINTER(ErrorC)]
    L.fsdkr_collect_first_error.restype = ctypes.c_int
    L.fsdkr_paillier_decrypt.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, u32p, u32p, u32p, u32p]
    L.fsdkr_paillier_decrypt.restype = ctypes.c_int
    L.fsdkr_paillier_encrypt.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, u32p, ctypes.c_uint32, u32p, u32p,
                                         u32p, ctypes.c_uint32, u32p]
    L.fsdkr_paillier_encrypt.restype = ctypes.c_int
    L.fsdkr_ctx_set_modexp_group.argtypes = [vp, ctypes.c_uint32]
    L.fsdkr_ctx_set_modexp_group.restype = ctypes.c_int
    L.fsdkr_ctx_set_timing.argtypes = [vp, ctypes.c_int]
    L.fsdkr_ctx_set_cu_split.argtypes = [vp, ctypes.c_uint32]
    L.fsdkr_ctx_set_cu_split.restype = ctypes.c_int
    L.fsdkr_ctx_set_timing.restype = ctypes.c_int
    L.fsdkr_ctx_set_flags.argtypes = [vp, ctypes.c_uint32]
    L.fsdkr_ctx_set_flags.restype = ctypes.c_int
    L.fsdkr_mod_inverse.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, u32p, u32p, u32p, u32p]
    L.fsdkr_mod_inverse.restype = ctypes.c_int
    L.fsdkr_mod_inverse_grouped.argtypes = L.fsdkr_mod_inverse.argtypes
    L.fsdkr_mod_inverse_grouped.restype = ctypes.c_int
    L.fsdkr_miller_rabin.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, u32p, u32p, u32p]
    L.fsdkr_miller_rabin.restype = ctypes.c_int
    L.fsdkr_ec_msm.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, u32p, u32p, u32p]
    L.fsdkr_ec_msm.restype = ctypes.c_int
    L.fsdkr_ec_msm_ct.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, u32p, u32p, u32p]
    L.fsdkr_ec_msm_ct.restype = ctypes.c_int
    L.fsdkr_ec_mul_g_ct.argtypes = [vp, ctypes.c_uint32, u32p, u32p]
    L.fsdkr_ec_mul_g_ct.restype = ctypes.c_int
    L.fsdkr_fixed_base_modexp.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, u32p, u32p, u32p, ctypes.c_uint32,
                                          ctypes.c_uint32, u32p, u32p, ctypes.c_uint32, u32p]
    L.fsdkr_fixed_base_modexp.restype = ctypes.c_int
    L.fsdkr_feldman_check.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, u32p, u32p, u8p]
    L.fsdkr_feldman_check.restype = ctypes.c_int
    L.fsdkr_pdl_u1_check.argtypes = [vp, ctypes.c_uint32, u32p, ctypes.c_uint32, u32p, u32p, u32p, u8p]
    L.fsdkr_pdl_u1_check.restype = ctypes.c_int
    L.fsdkr_ring_pedersen_verify.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                             u32p, u32p, u32p, u32p, u32p, u8p]
    L.fsdkr_ring_pedersen_verify.restype = ctypes.c_int
    L.fsdkr_bob_prove.argtypes = [vp, ctypes.POINTER(BobProveC), ctypes.POINTER(BobProofsC)]
    L.fsdkr_bob_prove.restype = ctypes.c_int
    L.fsdkr_alice_prove.argtypes = [vp, ctypes.POINTER(AliceProveC), ctypes.POINTER(AliceProofsC)]
    L.fsdkr_alice_prove.restype = ctypes.c_int
    L.fsdkr_resp_ct.argtypes = [vp, ctypes.c_uint32, u32p, u32p, ctypes.c_uint32, u32p, ctypes.c_uint32, u32p]
    L.fsdkr_resp_ct.restype = ctypes.c_int
    L.fsdkr_eq_check.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, u32p, ctypes.c_uint32, u32p, ctypes.c_uint32,
                                 u32p, ctypes.c_uint32, u32p, ctypes.c_uint32, u32p, u32p, u32p, u32p,
                                 ctypes.c_uint32, u32p, u8p]
    L.fsdkr_eq_check.restype = ctypes.c_int
    L.fsdkr_prod3.argtypes = [vp, ctypes.c_uint32, ctypes.c_uint32, u32p, ctypes.c_uint32, u32p, ctypes.c_uint32,
                              u32p, ctypes.c_uint32, u32p, ctypes.c_uint32, u32p, u32p]
    L.fsdkr_prod3.restype = ctypes.c_int
    L.fsdkr_pow2_check.argtypes = [vp, ctypes.c_uint32] + [u32p, ctypes.c_uint32] * 6 + [u32p, u32p, u32p, u32p,
                                                                                          ctypes.c_uint32, u8p]
    L.fsdkr_pow2_check.restype = ctypes.c_int
    _lib = L
    return L


def _ptr(a):
    return a.ctypes.data_as(u32p)


def ints_to_limbs(values, limbs):
    """list of non-negative ints -> (len, limbs) uint32 little-endian array
    (csrc/pack.c digit re-slicing); ValueError if a value is negative or too wide."""
    from . import _pack
    out = np.empty((len(values), limbs), dtype=np.uint32)
    try:
        _pack.pack(values, None, out, limbs)
    except OverflowError:
        raise ValueError(f"a value does not fit {limbs} limbs") from None
    return out


def limbs_to_ints(arr):
    arr = np.ascontiguousarray(arr, dtype=np.uint32)
    b = arr.tobytes()
    n = arr.shape[1] * 4
    return [int.from_bytes(b[i * n:(i + 1) * n], "little") for i in range(arr.shape[0])]


class Context:
    """Owns one fsdkr_ctx (HIP stream + device buffers)."""

    def __init__(self, device=-1, timing=False):
        L = lib()
        cfg = _Cfg(device, FSDKR_CFG_TIMING if timing else 0)
        h = ctypes.c_void_p()
        rc = L.fsdkr_ctx_create(ctypes.byref(cfg), ctypes.byref(h))
        if rc != FSDKR_OK:
            raise FsdkrError(rc, "fsdkr_ctx_create failed (no HIP device?)")
        self._h = h
        self._lib = L
        self._flags = cfg.flags

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            self._lib.fsdkr_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc):
        if rc != FSDKR_OK:
            raise FsdkrError(rc, self._lib.fsdkr_last_error(self._h).decode())

    def kernel_time(self, name):
        ms = ctypes.c_double()
        n = ctypes.c_uint32()
        self.check(self._lib.fsdkr_kernel_time(self._h, name.encode(), ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def kernel_time_reset(self):
        self._lib.fsdkr_kernel_time_reset(self._h)

    def modexp_batch(self, bases, exps, mods, mod_idx, mod_limbs, secret=False):
        """[base_i ^ exp_i mod mods[mod_idx_i]] computed on the GPU.  secret=True:
        regular-access kernel (fsdkr_modexp_batch_ct) for secret exponents."""
        count = len(bases)
        if count == 0:
            return []
        emax = max(1, max(e.bit_length() for e in exps))
        exp_limbs = (emax + 31) // 32
        B = ints_to_limbs(bases, mod_limbs)
        E = ints_to_limbs(exps, exp_limbs)
        Mo = ints_to_limbs(mods, mod_limbs)
        I = np.ascontiguousarray(np.asarray(mod_idx, dtype=np.uint32))
        O = np.zeros((count, mod_limbs), dtype=np.uint32)
        fn = self._lib.fsdkr_modexp_batch_ct if secret else self._lib.fsdkr_modexp_batch
        self.check(fn(self._h, mod_limbs, count, _ptr(B), _ptr(E), exp_limbs, _ptr(I), _ptr(Mo), len(mods), _ptr(O)))
        return limbs_to_ints(O)

    def modexp_joint_batch(self, bases, bases2, exps2, mods, mod_exps, mod_idx):
        """[bases[i] ^ mod_exps[k] * bases2[i] ^ exps2[i] mod mods[k]], k = mod_idx[i],
        4096-bit moduli, exps2 < 2^256, bases2 reduced: collect()'s split GA chains
        (fsdkr_modexp_joint_batch)."""
        count = len(bases)
        if count == 0:
            return []
        exp_limbs = max(1, (max(e.bit_length() for e in mod_exps) + 31) // 32)
        B = ints_to_limbs(bases, 128)
        B2 = ints_to_limbs(bases2, 128)
        E2 = ints_to_limbs(exps2, 8)
        Mo = ints_to_limbs(mods, 128)
        ME = ints_to_limbs(mod_exps, exp_limbs)
        I = np.ascontiguousarray(np.asarray(mod_idx, dtype=np.uint32))
        O = np.zeros((count, 128), dtype=np.uint32)
        self.check(self._lib.fsdkr_modexp_joint_batch(self._h, count, _ptr(B), _ptr(B2), _ptr(E2), _ptr(I), _ptr(Mo),
                                                      _ptr(ME), exp_limbs, len(mods), _ptr(O)))
        return limbs_to_ints(O)

    def modexp_nadic_batch(self, bases, bases2, exps2, nmods, mod_exps, mod_idx):
        """[bases[i] ^ mod_exps[k] * bases2[i] ^ exps2[i] mod nmods[k]^2], k = mod_idx[i], for
        odd nmods and bases below 2^2048: the half-width N-adic head of collect()'s GA
        chains and the tail that takes over from it (fsdkr_modexp_nadic_batch)."""
        count = len(bases)
        if count == 0:
            return []
        exp_limbs = max(1, (max(e.bit_length() for e in mod_exps) + 31) // 32)
        B = ints_to_limbs(bases, 64)
        B2 = ints_to_limbs(bases2, 128)
        E2 = ints_to_limbs(exps2, 8)
        Mo = ints_to_limbs(nmods, 64)
        ME = ints_to_limbs(mod_exps, exp_limbs)
        I = np.ascontiguousarray(np.asarray(mod_idx, dtype=np.uint32))
        O = np.zeros((count, 128), dtype=np.uint32)
        self.check(self._lib.fsdkr_modexp_nadic_batch(self._h, count, _ptr(B), _ptr(B2), _ptr(E2), _ptr(I), _ptr(Mo),
                                                      _ptr(ME), exp_limbs, len(nmods), _ptr(O)))
        return limbs_to_ints(O)

    def modexp_joint3_batch(self, bases, bases2, exps2, bases3, exps3, mods, mod_exps, mod_idx, k32=128):
        """[bases[i] ^ mod_exps[k] * bases2[i] ^ exps2[i] * bases3[i] ^ exps3[i] mod mods[k]],
        k = mod_idx[i], moduli of k32 limbs (128: 4096 bits, 192: 6144 bits), exps2 < 2^768,
        exps3 < 2^256, bases2 / bases3 reduced: the split chain of Bob's range proof
        (fsdkr_modexp_joint3_batch_k).  bases3 = exps3 = None: the two-base tail at the
        same split."""
        count = len(bases)
        if count == 0:
            return []
        exp_limbs = max(1, (max(e.bit_length() for e in mod_exps) + 31) // 32)
        e2l = max(1, (max(e.bit_length() for e in exps2) + 31) // 32)
        B = ints_to_limbs(bases, k32)
        B2 = ints_to_limbs(bases2, k32)
        E2 = ints_to_limbs(exps2, e2l)
        B3 = ints_to_limbs(bases3, k32) if bases3 is not None else None
        E3 = ints_to_limbs(exps3, 8) if exps3 is not None else None
        Mo = ints_to_limbs(mods, k32)
        ME = ints_to_limbs(mod_exps, exp_limbs)
        I = np.ascontiguousarray(np.asarray(mod_idx, dtype=np.uint32))
        O = np.zeros((count, k32), dtype=np.uint32)
        self.check(self._lib.fsdkr_modexp_joint3_batch_k(self._h, k32, count, _ptr(B), _ptr(B2), _ptr(E2), e2l,
                                                         _ptr(B3) if B3 is not None else None,
                                                         _ptr(E3) if E3 is not None else None, _ptr(I), _ptr(Mo),
                                                         _ptr(ME), exp_limbs, len(mods), _ptr(O)))
        return limbs_to_ints(O)

    def bob_verify(self, batch, count, fused=True):
        """fsdkr_bob_verify on a filled BobBatchC -> uint8 verdicts (1 / 0 / 2 = panic)."""
        out = np.zeros(count, dtype=np.uint8)
        fn = self._lib.fsdkr_bob_verify if fused else self._lib.fsdkr_bob_verify_unfused
        self.check(fn(self._h, ctypes.byref(batch), out.ctypes.data_as(u8p)))
        return out

    def alice_verify(self, batch, count):
        """fsdkr_alice_verify on a filled AliceBatchC -> uint8 verdicts (1 / 0); an empty
        batch returns empty without a device call."""
        out = np.zeros(count, dtype=np.uint8)
        if count == 0:
            return out
        self.check(self._lib.fsdkr_alice_verify(self._h, ctypes.byref(batch), out.ctypes.data_as(u8p)))
        return out

    def fixed_base_modexp(self, bases, base_mod_idx, mods, base_idx, exps, mod_limbs):
        """[bases[base_idx[i]] ^ exps[i] mod mods[base_mod_idx[base_idx[i]]]] via the fixed-base engine."""
        count = len(exps)
        if count == 0:
            return []
        exp_limbs = max(1, (max(e.bit_length() for e in exps) + 31) // 32)
        B = ints_to_limbs(bases, mod_limbs)
        Bm = np.ascontiguousarray(np.asarray(base_mod_idx, dtype=np.uint32))
        Mo = ints_to_limbs(mods, mod_limbs)
        Bi = np.ascontiguousarray(np.asarray(base_idx, dtype=np.uint32))
        E = ints_to_limbs(exps, exp_limbs)
        O = np.zeros((count, mod_limbs), dtype=np.uint32)
        self.check(self._lib.fsdkr_fixed_base_modexp(self._h, mod_limbs, len(bases), _ptr(B), _ptr(Bm), _ptr(Mo),
                                                     len(mods), count, _ptr(Bi), _ptr(E), exp_limbs, _ptr(O)))
        return limbs_to_ints(O)

    def set_modexp_group(self, lanes):
        """Force the lanes per modexp instance (0 = automatic)."""
        self.check(self._lib.fsdkr_ctx_set_modexp_group(self._h, lanes))

    def set_cu_split(self, ga_cus):
        """Multi-GPU shards: GA chains on `ga_cus` CUs, everything else on the rest (0 = off)."""
        self.check(self._lib.fsdkr_ctx_set_cu_split(self._h, ga_cus))

    def set_timing(self, on):
        """Per-kernel HIP-event timing on/off (kernel_time needs it on)."""
        self.check(self._lib.fsdkr_ctx_set_timing(self._h, 1 if on else 0))
        self._flags = (self._flags | FSDKR_CFG_TIMING) if on else (self._flags & ~FSDKR_CFG_TIMING)

    def set_flags(self, flags):
        """Replace the fsdkr_cfg flags (FSDKR_CFG_*); returns the previous ones."""
        old = self._flags
        self.check(self._lib.fsdkr_ctx_set_flags(self._h, flags))
        self._flags = flags
        return old

    @property
    def flags(self):
        return self._flags

    def mod_inverse(self, ys, ms, mod_limbs, grouped=False):
        """[(y^-1 mod m or None)] on the GPU (None where gcd(y, m) != 1).
        grouped: fsdkr_mod_inverse_grouped, the simultaneous-inversion kernel at
        every width and for every group size (parity tests)."""
        count = len(ys)
        if count == 0:
            return []
        Y = ints_to_limbs(ys, mod_limbs)
        M = ints_to_limbs(ms, mod_limbs)
        O = np.zeros((count, mod_limbs), dtype=np.uint32)
        U = np.zeros(count, dtype=np.uint32)
        fn = self._lib.fsdkr_mod_inverse_grouped if grouped else self._lib.fsdkr_mod_inverse
        self.check(fn(self._h, mod_limbs, count, _ptr(Y), _ptr(M), _ptr(O), _ptr(U)))
        return [v if u else None for v, u in zip(limbs_to_ints(O), U.tolist())]

    def miller_rabin(self, cands, bases, mod_limbs):
        """[1 if cands[i] is a strong probable prime to base bases[i] else 0] on the GPU."""
        count = len(cands)
        if count == 0:
            return []
        C = ints_to_limbs(cands, mod_limbs)
        B = ints_to_limbs(bases, mod_limbs)
        V = np.zeros(count, dtype=np.uint32)
        self.check(self._lib.fsdkr_miller_rabin(self._h, mod_limbs, count, _ptr(C), _ptr(B), _ptr(V)))
        return V.tolist()

    def sample_primes(self, draw_bits, bits, count, window=0, span=0):
        """fsdkr_sample_primes: `count` primes of `bits` bits by the batched prime
        walk; draw_bits(k) supplies the k-bit random starts (the caller's RNG)."""
        limbs = (bits + 31) // 32
        errs = []

        def cb(_user, nbits, out, nl):
            try:
                v = draw_bits(nbits)
                for k in range(nl):
                    out[k] = (v >> (32 * k)) & 0xFFFFFFFF
                return 0
            except Exception as e:   # re-raised below, after the C call returns
                errs.append(e)
                return 1
        fn = DRAW_BITS_FN(cb)
        O = np.zeros((max(1, count), limbs), dtype=np.uint32)
        rc = self._lib.fsdkr_sample_primes(self._h, bits, count, window, span, fn, None, _ptr(O), limbs)
        if errs:
            raise errs[0]
        self.check(rc)
        return limbs_to_ints(O[:count])

    # ---- collect() verification -------------------------------------------
    def verify_collect(self, batch):
        """Run fsdkr_verify_collect on a fsdkr.batch.CollectBatch; returns a Verdicts."""
        from .batch import Verdicts
        v = Verdicts(batch.R, batch.J, batch.n)
        self.check(self._lib.fsdkr_verify_collect(self._h, ctypes.byref(batch.c), ctypes.byref(v.c)))
        return batch.settle(v)

    def collect_prepare(self, batch):
        """Host pre-pass + one upload of the batch image (device-resident afterwards)."""
        self.check(self._lib.fsdkr_collect_prepare(self._h, ctypes.byref(batch.c)))

    def collect_run(self, batch):
        """Kernel pipeline on the prepared batch; returns Verdicts."""
        from .batch import Verdicts
        v = Verdicts(batch.R, batch.J, batch.n)
        self.check(self._lib.fsdkr_collect_run(self._h, ctypes.byref(v.c)))
        return batch.settle(v)

    def collect_prestart(self, batch):
        """Start the s^N mod N^2 chains of a batch whose GA fields are packed
        (CollectBatch(..., staged=True)); the next prepare of it reuses them."""
        self.check(self._lib.fsdkr_collect_prestart(self._h, ctypes.byref(batch.c)))

    def collect_last_span_ms(self):
        """Device span of the last finished collect() call (HIP events: first
        device work -> the pipeline's last kernel), -1 before any."""
        return float(self._lib.fsdkr_collect_last_span_ms(self._h))

    REUSE = {"ga": 1, "tables": 2, "ck": 4, "tz": 8}

    def collect_reuse(self):
        """Names of the prestarted parts the last prepare reused (fsdkr_collect_reuse_mask)."""
        m = int(self._lib.fsdkr_collect_reuse_mask(self._h))
        return {k for k, bit in self.REUSE.items() if m & bit}

    def collect_launch(self):
        """Enqueue the kernel pipeline of the prepared batch (returns at once)."""
        self.check(self._lib.fsdkr_collect_launch(self._h))

    def collect_finish(self, batch):
        """Wait for the launched pipeline; returns Verdicts."""
        from .batch import Verdicts
        v = Verdicts(batch.R, batch.J, batch.n)
        self.check(self._lib.fsdkr_collect_finish(self._h, ctypes.byref(v.c)))
        return batch.settle(v)

    def collect_prepare_many(self, batches):
        """Prepare many sessions (fsdkr.batch.CollectBatch each) as ONE device image."""
        arr = (CollectBatchC * len(batches))(*[b.c for b in batches])
        self._many = arr   # keep the array alive until finish
        self.check(self._lib.fsdkr_collect_prepare_multi(self._h, arr, len(batches)))

    def collect_prestart_set(self, sset):
        """Start the GA chains of every regular session of a staged SessionSet."""
        arr = sset.prestart_array()
        if arr is not None:
            self._prestart_keep = sset
            self.check(self._lib.fsdkr_collect_prestart_multi(self._h, arr, sset.n_prestart))

    def collect_prestart_rp_set(self, sset):
        """Start the ring-Pedersen T^Z exponents of a SessionSet whose stage 1b
        (SessionSet.stage_z) packed Z, behind the prestarted T tables."""
        arr = sset.prestart_array()
        if arr is not None:
            self.check(self._lib.fsdkr_collect_prestart_rp(self._h, arr, sset.n_prestart))

    def collect_prepare_set(self, sset):
        """Prepare every live session of a fsdkr.batch.SessionSet as ONE device image."""
        self._many = sset   # keep the struct rows alive until finish
        self.check(self._lib.fsdkr_collect_prepare_multi(self._h, sset.c_array, len(sset.live)))

    def collect_finish_set(self, sset):
        """Wait for the launched multi-session pipeline; SetVerdicts of the live sessions."""
        v = sset.verdicts()
        self.check(self._lib.fsdkr_collect_finish_multi(self._h, v.c_array, len(sset.live)))
        return sset.settle(v)

    def collect_finish_many(self, batches):
        """Wait for the launched multi-session pipeline; one Verdicts per session."""
        from .batch import Verdicts
        vs = [Verdicts(b.R, b.J, b.n) for b in batches]
        arr = (VerdictsC * len(vs))(*[v.c for v in vs])
        self.check(self._lib.fsdkr_collect_finish_multi(self._h, arr, len(vs)))
        return [b.settle(v) for b, v in zip(batches, vs)]

    def paillier_decrypt(self, cts, p, q, nl):
        """Decrypt ciphertexts under dk = (p, q) on the GPU (CRT form)."""
        C = ints_to_limbs(cts, 2 * nl)
        Pp = ints_to_limbs([p], nl)
        Qq = ints_to_limbs([q], nl)
        O = np.zeros((len(cts), nl), dtype=np.uint32)
        self.check(self._lib.fsdkr_paillier_decrypt(self._h, nl, len(cts), _ptr(C), _ptr(Pp), _ptr(Qq), _ptr(O)))
        return limbs_to_ints(O)

    def paillier_decrypt_many(self, cts, key_idx, ps, qs, nl):
        """Decrypt cts[k] under key (ps[key_idx[k]], qs[key_idx[k]]) on the GPU."""
        if not cts:
            return []
        C = ints_to_limbs(cts, 2 * nl)
        I = np.ascontiguousarray(np.asarray(key_idx, dtype=np.uint32))
        Pp = ints_to_limbs(ps, nl)
        Qq = ints_to_limbs(qs, nl)
        O = np.zeros((len(cts), nl), dtype=np.uint32)
        self.check(self._lib.fsdkr_paillier_decrypt_multi(self._h, nl, len(cts), _ptr(C), _ptr(I), _ptr(Pp),
                                                          _ptr(Qq), len(ps), _ptr(O)))
        return limbs_to_ints(O)

    def paillier_encrypt(self, ms, rs, ns, n_idx, nl):
        """Job 1: [(1 + m N) r^N mod N^2] for N = ns[n_idx[k]]."""
        ml = max(1, (max(m.bit_length() for m in ms) + 31) // 32)
        Mm = ints_to_limbs(ms, ml)
        Rr = ints_to_limbs(rs, nl)
        Nn = ints_to_limbs(ns, nl)
        I = np.ascontiguousarray(np.asarray(n_idx, dtype=np.uint32))
        O = np.zeros((len(ms), 2 * nl), dtype=np.uint32)
        self.check(self._lib.fsdkr_paillier_encrypt(self._h, nl, len(ms), _ptr(Mm), ml, _ptr(Rr), _ptr(I), _ptr(Nn),
                                                    len(ns), _ptr(O)))
        return limbs_to_ints(O)

    def mta_respond(self, a_encs, bs, beta_prims, rs, ns, n_idx, nl, fused=True):
        """Bob's MtA response [a_enc^b (1 + beta' N) r^N mod N^2] for N = ns[n_idx[k]]
        (range_proofs.rs:688-704; fsdkr_mta_respond).  bs (< 2^256), beta_prims and
        rs (< N) are SECRET and run in regular access; a_encs are reduced mod N^2.
        nl = 64 and nl = 96 are one constant-time chain per response alike.
        fused=False: the separate chains of fsdkr_mta_respond_unfused (A/B timing)."""
        count = len(a_encs)
        if not (len(bs) == len(beta_prims) == len(rs) == len(n_idx) == count):
            raise ValueError("mta_respond: argument lists differ in length")
        A = ints_to_limbs(list(a_encs), 2 * nl) if count else np.zeros((1, 2 * nl), dtype=np.uint32)
        B = ints_to_limbs(list(bs), 8) if count else np.zeros((1, 8), dtype=np.uint32)
        Bp = ints_to_limbs(list(beta_prims), nl) if count else np.zeros((1, nl), dtype=np.uint32)
        Rr = ints_to_limbs(list(rs), nl) if count else np.zeros((1, nl), dtype=np.uint32)
        Nn = ints_to_limbs(list(ns), nl)
        I = np.ascontiguousarray(np.asarray(list(n_idx) or [0], dtype=np.uint32))
        O = np.zeros((max(1, count), 2 * nl), dtype=np.uint32)
        fn = self._lib.fsdkr_mta_respond if fused else self._lib.fsdkr_mta_respond_unfused
        self.check(fn(self._h, nl, count, _ptr(A), _ptr(B), _ptr(Bp), _ptr(Rr), _ptr(I), _ptr(Nn), len(ns), _ptr(O)))
        return limbs_to_ints(O[:count])

    def bob_commit_v(self, a_encs, alphas, gammas, betas, ns, n_idx, nl, fused=True):
        """The commitment v of Bob's range proof [a_enc^alpha (1 + gamma N) beta^N mod N^2]
        for N = ns[n_idx[k]] (range_proofs.rs:283-288; fsdkr_bob_commit_v).  alphas
        (< 2^768, packed to 24 limbs), gammas (reduced below N) and betas (< N) are
        SECRET and run in regular access; a_encs are reduced mod N^2.  ValueError for
        a negative value or one wider than its row.  nl = 64 and nl = 96 are one
        constant-time chain per v alike.
        fused=False: the separate chains of fsdkr_bob_commit_v_unfused (A/B timing)."""
        count = len(a_encs)
        if not (len(alphas) == len(gammas) == len(betas) == len(n_idx) == count):
            raise ValueError("bob_commit_v: argument lists differ in length")
        Al = Ga = Be = None
        try:
            A = ints_to_limbs(list(a_encs), 2 * nl) if count else np.zeros((1, 2 * nl), dtype=np.uint32)
            Al = ints_to_limbs(list(alphas), 24) if count else np.zeros((1, 24), dtype=np.uint32)
            Ga = ints_to_limbs(list(gammas), nl) if count else np.zeros((1, nl), dtype=np.uint32)
            Be = ints_to_limbs(list(betas), nl) if count else np.zeros((1, nl), dtype=np.uint32)
            Nn = ints_to_limbs(list(ns), nl)
            I = np.ascontiguousarray(np.asarray(list(n_idx) or [0], dtype=np.uint32))
            O = np.zeros((max(1, count), 2 * nl), dtype=np.uint32)
            fn = self._lib.fsdkr_bob_commit_v if fused else self._lib.fsdkr_bob_commit_v_unfused
            self.check(fn(self._h, nl, count, _ptr(A), _ptr(Al), _ptr(Ga), _ptr(Be), _ptr(I), _ptr(Nn), len(ns), _ptr(O)))
        finally:
            for S in (Al, Ga, Be):
                if S is not None:
                    S.fill(0)
        return limbs_to_ints(O[:count])

    def pedersen_commit(self, xs, ys, keys, key_idx, nl, xl=None, yl=None):
        """[h1^x h2^y mod N~] for (N~, h1, h2) = keys[key_idx[k]], x = xs[k], y = ys[k]
        (fsdkr_pedersen_commit_ct): xs and ys are SECRET and run through the
        constant-time comb.  xl / yl: limbs of the x / y rows, a PUBLIC bound that
        alone sets the kernel's geometry (default: the widest value given, which
        tells an observer of the launch that width)."""
        count = len(xs)
        if not (len(ys) == len(key_idx) == count):
            raise ValueError("pedersen_commit: argument lists differ in length")
        if count == 0:
            return []
        xl = xl or max(1, (max(v.bit_length() for v in xs) + 31) // 32)
        yl = yl or max(1, (max(v.bit_length() for v in ys) + 31) // 32)
        X, Y = ints_to_limbs(list(xs), xl), ints_to_limbs(list(ys), yl)
        Nt, H1, H2 = (ints_to_limbs([k[c] for k in keys], nl) for c in range(3))
        I = np.ascontiguousarray(np.asarray(key_idx, dtype=np.uint32))
        O = np.zeros((count, nl), dtype=np.uint32)
        try:
            self.check(self._lib.fsdkr_pedersen_commit_ct(self._h, nl, count, _ptr(X), xl, _ptr(Y), yl, _ptr(I), _ptr(Nt),
                                                          _ptr(H1), _ptr(H2), len(keys), _ptr(O)))
        finally:
            X.fill(0)
            Y.fill(0)
        return limbs_to_ints(O)

    def _prove(self, fn, batch_cls, out_cls, widths, keys, key_idx, nl, public, secret):
        """One whole-prover call: `public` / `secret` map field names to lists of ints,
        packed with ints_to_limbs to the fixed widths; the secret staging arrays are
        zeroed whatever happens.  Returns {field: [int]}."""
        win, wout = widths
        count = len(key_idx)
        for name, vals in list(public.items()) + list(secret.items()):
            if len(vals) != count:
                raise ValueError(f"{fn.__name__}: {name} differs in length")
        if count == 0:
            return {f: [] for f in wout}
        b, o = batch_cls(), out_cls()
        b.count, b.n_keys, b.nl = count, len(keys), nl
        keep, staged = [], []
        try:
            for col, name in enumerate(("N", "Ntilde", "h1", "h2")):
                keep.append(ints_to_limbs([k[col] for k in keys], nl))
                setattr(b, name, _ptr(keep[-1]))
            keep.append(np.ascontiguousarray(np.asarray(key_idx, dtype=np.uint32)))
            b.key_idx = _ptr(keep[-1])
            for name, vals in public.items():
                keep.append(ints_to_limbs(list(vals), 2 * nl))
                setattr(b, name, _ptr(keep[-1]))
            for name in batch_cls.SECRET:
                staged.append(ints_to_limbs(list(secret[name]), win[name]))
                setattr(b, name, _ptr(staged[-1]))
            outs = {f: np.zeros((count, w), dtype=np.uint32) for f, w in wout.items()}
            for f, a in outs.items():
                setattr(o, f, _ptr(a))
            self.check(fn(self._h, ctypes.byref(b), ctypes.byref(o)))
        finally:
            for S in staged:
                S.fill(0)
        return {f: limbs_to_ints(a) for f, a in outs.items()}

    def bob_prove(self, keys, key_idx, nl, a_encs, mtas, **secret):
        """BobProof::generate of every proof in ONE device call (fsdkr_bob_prove).  keys:
        [(N, N~, h1, h2)] with h1, h2 < N~; a_encs reduced mod N^2; mtas hashed as given.
        SECRET keyword lists, each a draw or a witness per proof (BobProveC.SECRET): b,
        beta_prim, r, alpha, beta, gamma, gamma_mod_n (= gamma mod N), ro, ro_prim,
        sigma, tau.  ValueError for a negative value or one wider than its row
        (bob_prove_widths).  Returns {z, t, s, e, s1, s2, t1, t2: [int]}."""
        if set(secret) != set(BobProveC.SECRET):
            raise ValueError(f"bob_prove: needs exactly {BobProveC.SECRET}")
        return self._prove(self._lib.fsdkr_bob_prove, BobProveC, BobProofsC, bob_prove_widths(nl), keys, key_idx, nl,
                           {"a_enc": a_encs, "mta": mtas}, secret)

    def alice_prove(self, keys, key_idx, nl, ciphers, **secret):
        """AliceProof::generate of every proof in ONE device call (fsdkr_alice_prove).
        keys as in bob_prove; ciphers hashed as given.  SECRET keyword lists
        (AliceProveC.SECRET): a, r, alpha, beta, gamma, ro.  Returns {z, s, e, s1, s2: [int]}."""
        if set(secret) != set(AliceProveC.SECRET):
            raise ValueError(f"alice_prove: needs exactly {AliceProveC.SECRET}")
        return self._prove(self._lib.fsdkr_alice_prove, AliceProveC, AliceProofsC, alice_prove_widths(nl), keys, key_idx,
                           nl, {"cipher": ciphers}, secret)

    def resp_ct(self, es, xs, ys, xl, yl):
        """[e x + y] as integers through resp_ct_kernel (fsdkr_resp_ct): es public
        (< 2^256), xs / ys SECRET rows of xl / yl limbs (1 .. 128)."""
        count = len(es)
        if not (len(xs) == len(ys) == count):
            raise ValueError("resp_ct: argument lists differ in length")
        if count == 0:
            return []
        X = Y = None
        try:
            E = ints_to_limbs(list(es), 8)
            X, Y = ints_to_limbs(list(xs), xl), ints_to_limbs(list(ys), yl)
            O = np.zeros((count, max(xl + 8, yl) + 1), dtype=np.uint32)
            self.check(self._lib.fsdkr_resp_ct(self._h, count, _ptr(E), _ptr(X), xl, _ptr(Y), yl, _ptr(O)))
        finally:
            for S in (X, Y):
                if S is not None:
                    S.fill(0)
        return limbs_to_ints(O)

    def pdl_u1_check(self, s1s, es, Qs, u1s):
        """[G*(s1 mod q) + Q*(q - e mod q) == u1] per pair (uint8 0/1)."""
        from .batch import pack_points
        sl = max(1, (max(s.bit_length() for s in s1s) + 31) // 32)
        S = ints_to_limbs(s1s, sl)
        E = ints_to_limbs(es, 8)
        Qp, Up = pack_points(Qs), pack_points(u1s)
        out = np.zeros(len(s1s), dtype=np.uint8)
        self.check(self._lib.fsdkr_pdl_u1_check(self._h, len(s1s), _ptr(S), sl, _ptr(E), _ptr(Qp), _ptr(Up),
                                                out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))
        return out

    def eq_check(self, a, b, c, d, mods, mod_idx, mod_limbs, lens=None, sel=None, sel_bits=None, flags=None):
        """[a_i b_i == c_i d'_i (mod mods[mod_idx_i]), and c_i < N where flags_i & 1] as
        uint8 0/1 straight from eq_check_kernel (fsdkr_eq_check).  lens: limbs of the
        a, b, c, d rows (default: mod_limbs each).  sel_i: None (always d_i) or a bit
        index into sel_bits (a list of 32-bit words): d'_i = d_i if the bit is set,
        else 1.  FsdkrError(FSDKR_E_ARG) for a row outside the kernel's precondition
        (a or b, and c or d', below the modulus) or an even modulus."""
        count = len(a)
        if not (len(b) == len(c) == len(d) == len(mod_idx) == count):
            raise ValueError("eq_check: argument lists differ in length")
        out = np.zeros(count, dtype=np.uint8)
        if count == 0:
            return out
        al, bl, cl, dl = lens or (mod_limbs,) * 4
        A, B = ints_to_limbs(list(a), al), ints_to_limbs(list(b), bl)
        Cc, D = ints_to_limbs(list(c), cl), ints_to_limbs(list(d), dl)
        Mo = ints_to_limbs(list(mods), mod_limbs)
        I = np.ascontiguousarray(np.asarray(mod_idx, dtype=np.uint32))
        S = W = F = None
        if sel is not None:
            S = np.ascontiguousarray(np.asarray([0xFFFFFFFF if v is None else v for v in sel], dtype=np.uint32))
            W = np.ascontiguousarray(np.asarray(list(sel_bits or [0]), dtype=np.uint32))
        if flags is not None:
            F = np.ascontiguousarray(np.asarray(flags, dtype=np.uint32))
        if (S is not None and len(S) != count) or (F is not None and len(F) != count):
            raise ValueError("eq_check: sel / flags differ in length from the rows")
        self.check(self._lib.fsdkr_eq_check(self._h, mod_limbs, count, _ptr(A), al, _ptr(B), bl, _ptr(Cc), cl, _ptr(D), dl,
                                            _ptr(S) if S is not None else None, _ptr(W) if W is not None else None,
                                            _ptr(F) if F is not None else None, _ptr(Mo), len(mods), _ptr(I),
                                            out.ctypes.data_as(u8p)))
        return out

    def prod3(self, a, b, c, mods, mod_idx, mod_limbs, lens=None):
        """[a_i b_i c_i mod mods[mod_idx_i]] straight from prod3_kernel (fsdkr_prod3);
        lens: limbs of the a, b, c rows (default: mod_limbs each)."""
        count = len(a)
        if not (len(b) == len(c) == len(mod_idx) == count):
            raise ValueError("prod3: argument lists differ in length")
        if count == 0:
            return []
        al, bl, cl = lens or (mod_limbs,) * 3
        A, B, Cc = ints_to_limbs(list(a), al), ints_to_limbs(list(b), bl), ints_to_limbs(list(c), cl)
        Mo = ints_to_limbs(list(mods), mod_limbs)
        I = np.ascontiguousarray(np.asarray(mod_idx, dtype=np.uint32))
        O = np.zeros((count, mod_limbs), dtype=np.uint32)
        self.check(self._lib.fsdkr_prod3(self._h, mod_limbs, count, _ptr(A), al, _ptr(B), bl, _ptr(Cc), cl, _ptr(Mo),
                                         len(mods), _ptr(I), _ptr(O)))
        return limbs_to_ints(O)

    def pow2_check(self, a, ea, b, eb, c, d, kbits, lens, sel=None, sel_bits=None):
        """[a_i^ea_i b_i^eb_i == c_i d'_i (mod 2^kbits_i)] as uint8 0/1 straight from
        pow2_check_kernel (fsdkr_pow2_check).  a .. d: lists of ints, None for an absent
        operand (the kernel gets address 0: the value 1, exponent 0 for ea / eb).  lens:
        limbs of the a, ea, b, eb, c, d rows.  sel_i: None (d_i whenever present) or a
        bit index into sel_bits (a list of 32-bit words): d'_i = d_i if the bit is set,
        else 1.  FsdkrError(FSDKR_E_ARG) for kbits outside 1 .. 3072 or a sel past
        sel_bits; ValueError for a value wider than its row."""
        cols = [list(v) for v in (a, ea, b, eb, c, d)]
        count = len(cols[0])
        if not all(len(v) == count for v in cols) or len(kbits) != count or (sel is not None and len(sel) != count):
            raise ValueError("pow2_check: argument lists differ in length")
        out = np.zeros(count, dtype=np.uint8)
        if count == 0:
            return out
        rows = [ints_to_limbs([0 if x is None else x for x in v], l) for v, l in zip(cols, lens)]
        present = np.asarray([sum((v[i] is not None) << r for r, v in enumerate(cols)) for i in range(count)],
                             dtype=np.uint32)
        Kb = np.ascontiguousarray(np.asarray(kbits, dtype=np.uint32))
        S = W = None
        if sel is not None:
            S = np.ascontiguousarray(np.asarray([0xFFFFFFFF if v is None else v for v in sel], dtype=np.uint32))
        if sel_bits:
            W = np.ascontiguousarray(np.asarray(list(sel_bits), dtype=np.uint32))
        args = [self._h, count]
        for r, l in zip(rows, lens):
            args += [_ptr(r), l]
        self.check(self._lib.fsdkr_pow2_check(*args, _ptr(Kb), _ptr(S) if S is not None else None, _ptr(present),
                                              _ptr(W) if W is not None else None, 0 if W is None else len(W),
                                              out.ctypes.data_as(u8p)))
        return out

    def feldman_check(self, vss, commit, n, t):
        """vss: [n_msgs][t+1] points, commit: [n_msgs*n] points -> uint8 verdicts [n_msgs*n]."""
        from .batch import pack_points
        V = pack_points([p for row in vss for p in row])
        Cm = pack_points(commit)
        out = np.zeros(len(commit), dtype=np.uint8)
        self.check(self._lib.fsdkr_feldman_check(self._h, len(vss), n, t, _ptr(V), _ptr(Cm),
                                                 out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))
        return out

    def ring_pedersen_verify(self, statements, proofs, m_security, nl):
        """[(statement, proof)] -> uint8 verdicts (bit0 ok, bit1 the reference panics)."""
        from .batch import pack
        M = m_security
        zl = max(1, (max(z.bit_length() for p in proofs for z in p.Z[:M]) + 31) // 32)
        S = pack([s.S for s in statements], nl)
        T = pack([s.T for s in statements], nl)
        N = pack([s.N for s in statements], nl)
        A = pack([a for p in proofs for a in p.A[:M]], nl)
        Z = pack([z for p in proofs for z in p.Z[:M]], zl)
        out = np.zeros(len(proofs), dtype=np.uint8)
        self.check(self._lib.fsdkr_ring_pedersen_verify(self._h, nl, len(proofs), M, zl, _ptr(S), _ptr(T), _ptr(N),
                                                        _ptr(A), _ptr(Z),
                                                        out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))))
        return out

    def collect_recover(self, jobs):
        """fsdkr_collect_recover: jobs = [dict(nl, t_vss, t_key, old_index, cts, p, q, points[, flags])],
        points[i] = the first min(t_key, t_vss)+1 committed points for new party i
        (flags RECOVER_NO_DECRYPT: those pk_vec rows only, share and y zero).
        Returns per job (status, share, y, pk_vec); a ciphertext wider than N^2
        raises ValueError (ints_to_limbs)."""
        return self.collect_recover_finish(self.collect_recover_launch(jobs))

    def collect_recover_launch(self, jobs):
        """fsdkr_collect_recover_launch: the recovery's GPU work is enqueued and
        runs while the caller goes on; returns the handle collect_recover_finish takes.
        Every job's ciphertexts, keys, indices and points are packed into one array
        per field (one conversion each, however many jobs; the rows of job k at
        its offsets), and the fsdkr_recover_job rows are filled vectorised."""
        from . import _pack
        J = len(jobs)
        nls = np.array([j["nl"] for j in jobs], dtype=np.int64)
        T = np.array([len(j["cts"]) for j in jobs], dtype=np.int64)
        tp = np.array([min(j["t_key"], j["t_vss"]) + 1 for j in jobs], dtype=np.int64)
        n_new = np.array([len(j["points"]) for j in jobs], dtype=np.int64)
        for j, t in zip(jobs, T):
            assert t == j["t_vss"] + 1
        idx = np.ascontiguousarray(np.fromiter((i for j in jobs for i in j["old_index"]), dtype=np.uint32,
                                               count=int(T.sum())))
        Pt = np.zeros((max(1, int((n_new * tp).sum())), 16), dtype=np.uint32)
        pts = [pt for j in jobs for row in j["points"] for pt in row]
        if pts:
            _pack.points(pts, None, Pt)
        if J and (nls != nls[0]).any():   # rows at each job's own width
            C2, PQ2 = [], []
            for k, j in enumerate(jobs):
                C2.append(ints_to_limbs(j["cts"], 2 * j["nl"]))
                PQ2.append(ints_to_limbs([j["p"], j["q"]], j["nl"]))
            c_ptr = np.array([a.ctypes.data for a in C2], dtype=np.uint64)
            p_ptr = np.array([a.ctypes.data for a in PQ2], dtype=np.uint64)
            q_ptr = p_ptr + (nls * 4).astype(np.uint64)
            keep = (C2, PQ2)
        else:   # one width: one array per field
            W = int(nls[0]) if J else 1
            C = ints_to_limbs([c for j in jobs for c in j["cts"]], 2 * W)
            PQ = ints_to_limbs([v for j in jobs for v in (j["p"], j["q"])], W)

            def starts(c):
                return np.concatenate([[0], np.cumsum(c)[:-1]]).astype(np.uint64)
            c_ptr = np.uint64(C.ctypes.data) + starts(T) * np.uint64(2 * W * 4)
            p_ptr = np.uint64(PQ.ctypes.data) + np.arange(J, dtype=np.uint64) * np.uint64(2 * W * 4)
            q_ptr = p_ptr + np.uint64(W * 4)
            keep = (C, PQ)
        rows = np.zeros(J, dtype=_RECOVER_DT)
        rows["nl"] = nls
        rows["t_vss"] = [j["t_vss"] for j in jobs]
        rows["t_key"] = [j["t_key"] for j in jobs]
        rows["n_new"] = n_new
        off = np.concatenate([[0], np.cumsum(T)[:-1]]).astype(np.uint64)
        rows["old_index"] = np.uint64(idx.ctypes.data) + off * np.uint64(4)
        rows["cts"], rows["p"], rows["q"] = c_ptr, p_ptr, q_ptr
        poff = np.concatenate([[0], np.cumsum(n_new * tp)[:-1]]).astype(np.uint64)
        rows["points"] = np.uint64(Pt.ctypes.data) + poff * np.uint64(64)
        rows["flags"] = [j.get("flags", 0) for j in jobs]
        # the launch reads every host array before it returns (keep, idx, Pt, rows live until then)
        self.check(self._lib.fsdkr_collect_recover_launch(
            self._h, ctypes.cast(rows.ctypes.data, ctypes.POINTER(RecoverJobC)), J))
        del keep
        return [int(x) for x in n_new]

    def collect_recover_finish(self, handle):
        """Waits for the launched recovery; per job (status, share, y, pk_vec).
        Every job's pk_vec rows land in one array (job k's at its offset) and the
        results are converted in one pass each (no per-job allocations)."""
        n_new = np.asarray(handle, dtype=np.int64)
        J = len(n_new)
        outs = (RecoveredC * J)()
        PK = np.zeros((max(1, int(n_new.sum())), 16), dtype=np.uint32)
        rows = np.frombuffer(outs, dtype=_RECOVERED_DT, count=J) if J else None
        if J:
            off = np.concatenate([[0], np.cumsum(n_new)[:-1]]).astype(np.uint64)
            rows["pk_vec"] = np.uint64(PK.ctypes.data) + off * np.uint64(64)
        self.check(self._lib.fsdkr_collect_recover_finish(self._h, outs))
        if not J:
            return []

        def point(v):
            return None if v == 0 else (v & ((1 << 256) - 1), v >> 256)
        raw = np.frombuffer(outs, dtype=np.uint8).reshape(J, ctypes.sizeof(RecoveredC))
        o_sh, o_y = RecoveredC.share.offset, RecoveredC.y.offset
        shares = limbs_to_ints(raw[:, o_sh:o_sh + 32].copy().view(np.uint32))
        ys = [point(v) for v in limbs_to_ints(raw[:, o_y:o_y + 64].copy().view(np.uint32))]
        pks = [point(v) for v in limbs_to_ints(PK[:int(n_new.sum())])] if n_new.sum() else []
        res, at = [], 0
        for k in range(J):
            n = int(n_new[k])
            res.append((int(rows["status"][k]), shares[k], ys[k], pks[at:at + n]))
            at += n
        return res

    def ec_msm(self, points, scalars, secret=False):
        """points/scalars: lists (count) of equal-length lists; points are (x, y) or None.
        secret=True: the scalars are secret (fsdkr_ec_msm_ct: no scalar-dependent
        address or branch); the results are the same points."""
        from . import _pack
        count = len(points)
        if count == 0:
            return []
        terms = len(points[0])
        Pt = np.empty((count * terms, 16), dtype=np.uint32)
        _pack.points([pt for row in points for pt in row], None, Pt)
        Sc = ints_to_limbs([s for row in scalars for s in row], 8)
        O = np.zeros((count, 16), dtype=np.uint32)
        fn = self._lib.fsdkr_ec_msm_ct if secret else self._lib.fsdkr_ec_msm
        self.check(fn(self._h, count, terms, _ptr(Pt), _ptr(Sc), _ptr(O)))
        return _points_out(O)

    def ec_mul_g(self, scalars):
        """[k * G for k in scalars] for SECRET scalars (0 <= k < 2^256), always through
        the constant-time entry fsdkr_ec_mul_g_ct; points are (x, y) or None."""
        count = len(scalars)
        if count == 0:
            return []
        Sc = ints_to_limbs(list(scalars), 8)
        O = np.zeros((count, 16), dtype=np.uint32)
        self.check(self._lib.fsdkr_ec_mul_g_ct(self._h, count, _ptr(Sc), _ptr(O)))
        return _points_out(O)


def _points_out(O):
    """[count][16] affine limbs -> (x, y) tuples, None for the ABI's infinity (0, 0)."""
    out = []
    for v in limbs_to_ints(O):
        x, y = v & ((1 << 256) - 1), v >> 256
        out.append(None if (x == 0 and y == 0) else (x, y))
    return out
