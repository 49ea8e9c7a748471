"""CPU checks of Bob's MtA range proofs: the test oracle (tests/mta_oracle.py)
on the reference's own bob_zkp scenario (range_proofs.rs:672-745), the host
pre-pass of fsdkr.mta.verify_bob, and the layout of fsdkr_bob_batch."""
import ctypes
import os
import subprocess

import pytest

import mta_oracle as mo
from oracle import paillier
from oracle import secp256k1 as ec
from oracle.rng import Rng

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q3 = ec.Q ** 3


@pytest.fixture(scope="module")
def world():
    """generate_init (:626-648) at 2048 bits and one MtA exchange with both proofs."""
    rng = Rng("mta-cpu")
    ekt, dkt = paillier.keypair_with_modulus_size(2048, rng)
    st = mo.dlog_statement(ekt.n, dkt.p, dkt.q, rng)
    ek, dk = paillier.keypair_with_modulus_size(2048, rng)
    a_enc, mta, b, beta_prim, r = mo.mta_scenario(ek, rng)
    pf, _ = mo.generate(a_enc, mta, b, beta_prim, ek, st, r, rng, check=False)
    pfx = mo.generate_ext(a_enc, mta, b, beta_prim, ek, st, r, rng)
    return dict(ek=ek, dk=dk, st=st, a_enc=a_enc, mta=mta, X=ec.mul(ec.G, b), pf=pf, pfx=pfx)


def test_oracle_round_trip(world):
    w = world
    assert mo.verify(w["pf"], w["a_enc"], w["mta"], w["ek"], w["st"]) is True
    assert mo.verify_ext(w["pfx"], w["a_enc"], w["mta"], w["ek"], w["st"], w["X"]) is True
    # the extended proof's hash covers X and u: it is no plain proof
    assert mo.verify(w["pfx"].proof, w["a_enc"], w["mta"], w["ek"], w["st"]) is False


@pytest.mark.parametrize("kind", mo.TAMPERS)
def test_oracle_rejects_tamper(world, kind):
    w = world
    pf, a_enc, mta, X = mo.tamper(kind, w["pfx"], w["a_enc"], w["mta"], w["X"])
    assert mo.verify_ext(pf, a_enc, mta, w["ek"], w["st"], X) is False
    if kind not in ("X", "u"):
        pf, a_enc, mta, _ = mo.tamper(kind, w["pf"], w["a_enc"], w["mta"], None)
        assert mo.verify(pf, a_enc, mta, w["ek"], w["st"]) is False


def test_oracle_panics_at_infinity(world):
    w = world
    assert mo.outcome(w["pfx"], w["a_enc"], w["mta"], w["ek"], w["st"], None) == 2
    assert mo.outcome(type(w["pfx"])(w["pfx"].proof, None), w["a_enc"], w["mta"], w["ek"], w["st"], w["X"]) == 2


# ---- fsdkr.mta host pre-pass ---------------------------------------------------
def _pp(w, pf, **kw):
    from fsdkr import mta
    args = dict(a_encs=[w["a_enc"]], mta_outs=[w["mta"]], eks=[w["ek"]], statements=[w["st"]])
    args.update(kw)
    return mta.prepass([pf], **args)


def test_prepass_s1_bound(world):
    at = _pp(world, mo.with_field(world["pf"], "s1", Q3))
    over = _pp(world, mo.with_field(world["pf"], "s1", Q3 + 1))
    far = _pp(world, mo.with_field(world["pf"], "s1", 1 << 5000))
    assert at["s1_over"] == [False] and at["s1"] == [Q3]
    assert over["s1_over"] == [True] and far["s1_over"] == [True]
    assert far["s1"] == [Q3 + 1]          # packed within the field, same outcome
    wide = _pp(world, mo.with_field(world["pf"], "e", (1 << 3000) + 5))
    assert wide["e"] == [1 << 256]        # a challenge of 2^256 or more never matches


def test_prepass_t1_reduction(world):
    pf, N = world["pf"], world["ek"].n
    assert pf.t1 > N                      # the honest t1 = e beta' + gamma is wider than N
    pp = _pp(world, pf)
    assert pp["t1_red"] == [pf.t1 % N]
    assert (1 + pf.t1 * N) % (N * N) == (1 + pp["t1_red"][0] * N) % (N * N)


def test_prepass_key_dedup(world):
    from fsdkr import mta
    from oracle.paillier import EncryptionKey
    w = world
    ek2 = EncryptionKey.from_n(w["st"].N)   # another odd modulus
    eks = [w["ek"], ek2, w["ek"], type(w["ek"])(w["ek"].n, w["ek"].nn), ek2]
    pp = mta.prepass([w["pf"]] * 5, [w["a_enc"]] * 5, [w["mta"]] * 5, eks, [w["st"]] * 5)
    assert pp["key_idx"] == [0, 1, 0, 0, 1]
    assert pp["keys"] == [(w["ek"].n, w["st"].N, w["st"].g, w["st"].ni), (ek2.n, w["st"].N, w["st"].g, w["st"].ni)]


def test_prepass_unsupported(world):
    from fsdkr.batch import UnsupportedInput
    from oracle.paillier import EncryptionKey
    from oracle.zk_paillier import DLogStatement
    w = world
    with pytest.raises(UnsupportedInput):     # a negative field
        _pp(w, mo.with_field(w["pf"], "s2", -1))
    with pytest.raises(UnsupportedInput):
        _pp(w, w["pf"], a_encs=[-w["a_enc"]])
    for bad in (w["ek"].n + 1, 0):            # an even or zero N / N~
        with pytest.raises(UnsupportedInput):
            _pp(w, w["pf"], eks=[EncryptionKey.from_n(bad)])
        with pytest.raises(UnsupportedInput):
            _pp(w, w["pf"], statements=[DLogStatement(bad, w["st"].g, w["st"].ni)])
    with pytest.raises(UnsupportedInput):     # a hashed value wider than its field
        _pp(w, mo.with_field(w["pf"], "z", 1 << 2048))
    with pytest.raises(UnsupportedInput):
        _pp(w, w["pf"], mta_outs=[1 << 4096])


def test_bob_batch_layout(tmp_path):
    """sizeof / offsetof of fsdkr_bob_batch (gcc) equal the ctypes mirror."""
    from fsdkr import _native
    py = _native.BobBatchC
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "fsdkr/fsdkr.h"', "int main(void){",
             'printf("%zu\\n", sizeof(fsdkr_bob_batch));']
    for f, _ in py._fields_:
        lines.append(f'printf("%zu\\n", offsetof(fsdkr_bob_batch, {f}));')
    lines.append("return 0;}")
    c = tmp_path / "probe.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(REPO, "include"), str(c), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(py)] + [getattr(py, f).offset for f, _ in py._fields_]
    lib = _native.lib()
    for name in ("fsdkr_bob_verify", "fsdkr_bob_verify_unfused", "fsdkr_modexp_joint3_batch"):
        assert hasattr(lib, name)
