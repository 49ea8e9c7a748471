"""GPU checks of Alice's side of MtA at batch shapes (fsdkr.mta.initiate /
verify_alice, fsdkr_alice_verify), which tests/test_mta_alice_gpu.py (at most 18
proofs a call) does not reach: more than kInvChunk = 32 proofs of one key, so that
the verifier's simultaneous inversion forms a second group of a key, a remainder
group of one, and full groups in which a non-unit (z | p, cipher | p) sits among 31
honest proofs; the lanes forced to 4, 8 and 16 on such a batch; and the 3072-bit
class with 2048-bit rows zero-extended into it.  A non-invertible element spoils the
whole product of Montgomery's trick, so the point is that the honest neighbours of
a non-unit are still accepted: the oracle's verdict (oracle.range_proofs.verify) is
computed for every tampered row and for the nearest honest rows of each non-unit;
every other row is an honest proof, which the device must accept.

initiate's batch of 75 is checked against the oracle bit for bit on a sample of 6
exchanges under the same seeded stream."""
import copy
import dataclasses
from collections import namedtuple

import pytest

from oracle import paillier
from oracle import range_proofs as rp
from oracle import secp256k1 as ec
from oracle.rng import Rng
from test_mta_alice_gpu import _key_sets, _oracle_verdict, _t

pytestmark = pytest.mark.gpu

Q = ec.Q
Q3 = Q ** 3
# 41 exchanges under key set 0 and 34 under key set 1, neither contiguous in the call
ORDER_64 = [0 if (i % 2 == 0 or i >= 68) else 1 for i in range(75)]
SAMPLE_64 = (0, 1, 37, 38, 73, 74)
SEED_64 = ("mta-alice-shapes", 64)

Row = namedtuple("Row", "kind label idx pf c k")   # idx: position among the rows of its key set


@pytest.fixture(scope="module")
def keys(gpu_ctx):
    """Two key sets of 2048 bits and one of 3072 (a Paillier key and an N~ each,
    device-generated); pt is a prime factor of N~."""
    rng = Rng("mta-alice-shapes-keys")
    return dict(k2048=_key_sets(gpu_ctx, rng, 2048, 2), k3072=_key_sets(gpu_ctx, rng, 3072, 1))


def _initiate(ctx, ks, tag, seed):
    from fsdkr import mta
    rng = Rng(("mta-alice-shapes-a", tag))
    as_ = [0, Q - 1] + [rng.sample_below(Q) for _ in range(len(ks) - 2)]
    a_encs, rs, proofs = mta.initiate(as_, [k["ek"] for k in ks], [k["st"] for k in ks], Rng(seed), ctx=ctx)
    return dict(ks=ks, as_=as_, a_encs=a_encs, rs=rs, proofs=proofs)


@pytest.fixture(scope="module")
def made64(gpu_ctx, keys):
    """75 honest exchanges over the two 2048-bit key sets in ONE initiate call."""
    assert ORDER_64.count(0) == 41 and ORDER_64.count(1) == 34
    return _initiate(gpu_ctx, [keys["k2048"][m] for m in ORDER_64], 64, SEED_64)


@pytest.fixture(scope="module")
def made96(gpu_ctx, keys):
    """35 honest exchanges under the 3072-bit key set in ONE initiate call."""
    return _initiate(gpu_ctx, [keys["k3072"][0]] * 35, 96, ("mta-alice-shapes", 96))


def _skip_proof_draws(rng, ek, st):
    """The draws of oracle.range_proofs.generate (alpha, beta, gamma, ro) without its modexps."""
    rng.sample_below(Q3)
    rng.from_modulo(ek.n)
    rng.sample_below(Q3 * st.N)
    rng.sample_below(Q * st.N)


def test_initiate_batch_matches_the_oracle(made64):
    """The reference's alice_zkp (:650-670) over one stream in initiate's order (every
    r first, then the proofs): all 75 r, and the ciphertexts and proofs of the sample.
    The exchanges between the sampled ones only draw; that those draws are the
    oracle's is checked against its generate on the first exchange."""
    x = made64
    rng = Rng(SEED_64)
    assert [rng.from_modulo(k["ek"].n) for k in x["ks"]] == x["rs"]
    for i, (k, a, r) in enumerate(zip(x["ks"], x["as_"], x["rs"])):
        if i not in SAMPLE_64:
            _skip_proof_draws(rng, k["ek"], k["st"])
            continue
        c = paillier.encrypt_with_chosen_randomness(k["ek"], a, r)
        assert c == x["a_encs"][i]
        probe = copy.deepcopy(rng) if i == 0 else None
        want = rp.generate(a, c, k["ek"], k["st"], r, rng)
        if probe is not None:
            _skip_proof_draws(probe, k["ek"], k["st"])
            assert probe.bits(256) == copy.deepcopy(rng).bits(256)
        assert _t(x["proofs"][i]) == _t(want), i


def _tamper(kind, pf, c, k):
    N, Nt = k["ek"].n, k["st"].N
    if kind == "z|p":
        pf = dataclasses.replace(pf, z=pf.z * k["pt"] % Nt)
    elif kind == "cipher|p":
        c = c * k["dk"].p % (N * N)
    elif kind == "s":
        pf = dataclasses.replace(pf, s=pf.s + 1)
    elif kind == "e=2^256":
        pf = dataclasses.replace(pf, e=1 << 256)
    else:
        assert kind == "honest"
    return pf, c


def _place(rows, plan):
    """rows: honest (label, proof, cipher, key set) in call order; plan: the tamper of
    (label, position among the label's rows).  Returns the call's Rows."""
    seen, out, used = {}, [], set()
    for label, pf, c, k in rows:
        j = seen.get(label, 0)
        seen[label] = j + 1
        kind = plan.get((label, j), "honest")
        used.add((label, j))
        pf, c = _tamper(kind, pf, c, k)
        out.append(Row(kind, label, j, pf, c, k))
    assert set(plan) <= used
    return out, seen


def _oracle_rows(batch):
    """Indices of every tampered row and of the two nearest honest rows, in its key's
    order, of each non-unit."""
    need = set()
    for i, r in enumerate(batch):
        if r.kind == "honest":
            continue
        need.add(i)
        if r.kind in ("z|p", "cipher|p"):
            near = sorted((abs(o.idx - r.idx), o.idx, j) for j, o in enumerate(batch)
                          if o.label == r.label and o.kind == "honest")[:2]
            assert len(near) == 2
            need |= {j for _, _, j in near}
    return sorted(need)


def _check_oracle(batch):
    """The expected verdicts (1 honest, 0 tampered), confirmed by the oracle on _oracle_rows."""
    want = [1 if r.kind == "honest" else 0 for r in batch]
    for i in _oracle_rows(batch):
        r = batch[i]
        assert _oracle_verdict(r.pf, r.c, r.k["ek"], r.k["st"]) == want[i], (i, r.kind, r.label, r.idx)
    return want


def _verify(ctx, batch):
    from fsdkr import mta
    return list(mta.verify_alice([r.pf for r in batch], [r.c for r in batch], [r.k["ek"] for r in batch],
                                 [r.k["st"] for r in batch], ctx=ctx))


@pytest.fixture(scope="module")
def batch64(made64):
    """74 rows: key set 0 has 41 (inversion groups of 32 + 9), key set 1 has 33 (32 + 1:
    one of its 34 is dropped).  Non-units at both ends of key 0's full group, at the head
    of its second group and alone in key 1's remainder group; s + 1 and e = 2^256 in the
    middle of a group."""
    x = made64
    rows = [(m, pf, c, k) for m, pf, c, k in zip(ORDER_64, x["proofs"], x["a_encs"], x["ks"])]
    last1 = max(i for i, m in enumerate(ORDER_64) if m == 1)
    del rows[last1]
    plan = {(0, 0): "z|p", (0, 31): "cipher|p", (0, 32): "z|p", (1, 32): "cipher|p", (0, 15): "s", (1, 16): "e=2^256"}
    batch, per = _place(rows, plan)
    assert per == {0: 41, 1: 33} and batch[0].label == 0       # key set 0 is row 0 of the call's key table
    return batch, _check_oracle(batch)


@pytest.mark.parametrize("lanes", [0, 4, 8, 16])
def test_verify_batch_2048(gpu_ctx, batch64, lanes):
    """The automatic lane choice, then every forced one."""
    batch, want = batch64
    assert want.count(0) == 6 and len(want) == 74
    try:
        gpu_ctx.set_modexp_group(lanes)
        assert _verify(gpu_ctx, batch) == want
    finally:
        gpu_ctx.set_modexp_group(0)


@pytest.mark.parametrize("count", [9, 17])
def test_verify_batch_2048_prefix(gpu_ctx, batch64, count):
    batch, want = batch64
    assert _verify(gpu_ctx, batch[:count]) == want[:count]


@pytest.fixture(scope="module")
def batch96(made64, made96):
    """45 rows in the 3072-bit class: the 35 of the 3072-bit key set (groups of 32 + 3,
    tampered as key set 0 above) with 10 honest 2048-bit rows, five of each key set,
    between them."""
    w, n = made96, made64
    wide = [("w", pf, c, k) for pf, c, k in zip(w["proofs"], w["a_encs"], w["ks"])]
    narrow = [(m, n["proofs"][i], n["a_encs"][i], n["ks"][i]) for i, m in enumerate(ORDER_64)][2:12]
    rows = []
    for i, r in enumerate(wide):
        rows.append(r)
        if i % 3 == 1 and narrow:
            rows.append(narrow.pop(0))
    assert not narrow
    plan = {("w", 0): "z|p", ("w", 31): "cipher|p", ("w", 32): "z|p", ("w", 12): "s", ("w", 20): "e=2^256"}
    batch, per = _place(rows, plan)
    assert per == {"w": 35, 0: 5, 1: 5}
    return batch, _check_oracle(batch)


def test_verify_batch_3072(gpu_ctx, batch96):
    from fsdkr import _native
    batch, want = batch96
    assert want.count(0) == 5 and len(want) == 45
    assert _verify(gpu_ctx, batch) == want
    try:
        gpu_ctx.set_modexp_group(8)            # the class's only shape
        assert _verify(gpu_ctx, batch) == want
        gpu_ctx.set_modexp_group(16)
        with pytest.raises(_native.FsdkrError) as e:
            _verify(gpu_ctx, batch)
        assert e.value.code == _native.FSDKR_E_ARG
    finally:
        gpu_ctx.set_modexp_group(0)
