"""CPU checks of the width classes of Bob's MtA range proofs: the host pre-pass
of fsdkr.mta.verify_bob picks 64 or 96 limbs from the keys alone, and the C ABI
declares fsdkr_modexp_joint3_batch_k as the ctypes binding calls it."""
import os
import re

import pytest

import mta_oracle as mo
from oracle.paillier import EncryptionKey
from oracle.zk_paillier import DLogStatement

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fsdkr", "fsdkr.h")


def _odd(bits):
    """An odd value of exactly `bits` bits (the pre-pass asks no more of a key)."""
    return (1 << (bits - 1)) | (0x5DEECE66D << 64) | 1


def _pp(n_bits, nt_bits, **fields):
    from fsdkr import mta
    ek = EncryptionKey.from_n(_odd(n_bits))
    st = DLogStatement(_odd(nt_bits), 3, 5)
    pf = mo.BobProof(**{**dict(t=7, z=11, e=13, s=17, s1=19, s2=23, t1=29, t2=31), **fields})
    return mta.prepass([pf], [37], [41], [ek], [st])


@pytest.mark.parametrize("n_bits,nt_bits,nl", [(2048, 2048, 64), (1024, 2047, 64), (3072, 2048, 96), (2048, 3072, 96),
                                               (2049, 2048, 96), (3072, 3072, 96)])
def test_prepass_width_class(n_bits, nt_bits, nl):
    from fsdkr import mta
    assert _pp(n_bits, nt_bits)["nl"] == nl
    assert mta.NL == 64


def test_prepass_key_above_3072_bits():
    from fsdkr.batch import UnsupportedInput
    with pytest.raises(UnsupportedInput):
        _pp(3073, 2048)
    with pytest.raises(UnsupportedInput):
        _pp(3072, 3073)


def test_prepass_field_wider_than_class():
    from fsdkr.batch import UnsupportedInput
    assert _pp(3072, 3072, z=(1 << 3072) - 1)["nl"] == 96
    with pytest.raises(UnsupportedInput):
        _pp(3072, 3072, z=1 << 3072)          # 3073 bits in class 96
    with pytest.raises(UnsupportedInput):
        _pp(2048, 2048, z=1 << 2048)          # the keys alone pick the class: no promotion to 96
    from fsdkr import mta
    ek, st = EncryptionKey.from_n(_odd(3072)), DLogStatement(_odd(3072), 3, 5)
    pf = mo.BobProof(t=7, z=11, e=13, s=17, s1=19, s2=23, t1=29, t2=31)
    assert mta.prepass([pf], [(1 << 6144) - 1], [41], [ek], [st])["nl"] == 96
    with pytest.raises(UnsupportedInput):
        mta.prepass([pf], [37], [1 << 6144], [ek], [st])


def test_joint3_k_declared_and_bound():
    """The header declares fsdkr_modexp_joint3_batch_k with one argument (k32) more
    than fsdkr_modexp_joint3_batch, and the ctypes binding passes as many."""
    from fsdkr import _native
    src = open(HEADER).read()

    def nargs(name):
        m = re.search(r"^int " + name + r"\(([^;]*?)\);", src, re.M | re.S)
        assert m, name
        return len(m.group(1).split(","))

    lib = _native.lib()
    assert hasattr(lib, "fsdkr_modexp_joint3_batch_k")
    assert nargs("fsdkr_modexp_joint3_batch_k") == nargs("fsdkr_modexp_joint3_batch") + 1
    assert len(lib.fsdkr_modexp_joint3_batch_k.argtypes) == nargs("fsdkr_modexp_joint3_batch_k")
    assert len(lib.fsdkr_modexp_joint3_batch.argtypes) == nargs("fsdkr_modexp_joint3_batch")
