"""The provers send their secret scalars through the constant-time entry:
distribute (G*share, G*a_k, G*alpha), join.vss_share (the new polynomial's
coefficients) and mta.generate_bob(check=True) (X = G*b, u = G*alpha) issue no
public-scalar ec_msm call, and their outputs equal the oracle's provers' under
the same draws.  Inputs: the golden 1024-bit keys (t = 1), one MtA item."""
import copy
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import codec  # noqa: E402
import mta_oracle as mo  # noqa: E402
from oracle import protocol  # noqa: E402
from oracle import secp256k1 as ec  # noqa: E402
from oracle.paillier import EncryptionKey  # noqa: E402
from oracle.rng import Rng  # noqa: E402
from oracle.vss import VerifiableSS  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rec_ctx():
    """A context of its own that records the secp256k1 calls it serves."""
    from fsdkr import Context

    class Recorder(Context):
        def __init__(self):
            super().__init__()
            self.calls = []

        def ec_msm(self, points, scalars, secret=False):
            self.calls.append(("ec_msm", bool(secret), len(points)))
            return super().ec_msm(points, scalars, secret=secret)

        def ec_mul_g(self, scalars):
            self.calls.append(("ec_mul_g", True, len(scalars)))
            return super().ec_mul_g(scalars)

    ctx = Recorder()
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def golden_key():
    raw = codec.load_raw("transcript_join_t1_n4_kb1024.json.gz")
    assert raw["meta"]["t"] == 1 and raw["meta"]["key_bits"] == 1024
    return codec.dec(raw["keys"], codec.product_classes())[0]


def _secret_only(ctx, at_least):
    assert [c for c in ctx.calls if c[0] == "ec_msm" and not c[1]] == []
    assert sum(c[2] for c in ctx.calls if c[0] == "ec_mul_g") >= at_least
    ctx.calls.clear()


def test_distribute_uses_the_constant_time_entry(rec_ctx, golden_key):
    from fsdkr import distribute
    n = golden_key.n
    ko, kg = copy.deepcopy(golden_key), copy.deepcopy(golden_key)
    mo_, dko = protocol.distribute(ko.i, ko, n, Rng("ct-dist"), 1024)
    rec_ctx.calls.clear()
    mg, dkg = distribute.distribute(kg.i, kg, n, Rng("ct-dist"), ctx=rec_ctx, key_bits=1024)
    _secret_only(rec_ctx, n + 2 + n)              # shares, t + 1 coefficients, PDL blindings
    assert codec.enc(mg) == codec.enc(mo_)
    assert (dkg.p, dkg.q) == (dko.p, dko.q)
    assert codec.enc(kg.vss_scheme) == codec.enc(ko.vss_scheme)


def test_vss_share_uses_the_constant_time_entry(rec_ctx):
    from fsdkr import join
    secret = Rng("ct-vss-secret").sample_below(ec.Q)
    want, _ = VerifiableSS.share(1, 4, secret, Rng("ct-vss"))
    rec_ctx.calls.clear()
    got = join.vss_share(rec_ctx, 1, 4, secret, Rng("ct-vss").sample_below)
    _secret_only(rec_ctx, 2)
    assert (got.threshold, got.share_count) == (1, 4)
    assert list(got.commitments) == list(want.commitments)


def test_generate_bob_uses_the_constant_time_entry(rec_ctx, golden_key):
    from fsdkr import mta
    ek = EncryptionKey.from_n(golden_key.paillier_key_vec[0].n)
    st = golden_key.h1_h2_n_tilde_vec[1]
    a_enc, m, b, beta_prim, r = mo.mta_scenario(ek, Rng("ct-mta"))
    item = (a_enc, m, b, beta_prim, ek, st, r)
    pf, u = mo.generate(*item, Rng("ct-mta-draws"), check=True)
    rec_ctx.calls.clear()
    got = mta.generate_bob([item], Rng("ct-mta-draws"), ctx=rec_ctx, check=True)
    _secret_only(rec_ctx, 2)                      # X = G*b and u = G*alpha
    assert [getattr(got[0].proof, f) for f in mo.FIELDS] == [getattr(pf, f) for f in mo.FIELDS]
    assert got[0].u == u
