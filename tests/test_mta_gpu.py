"""GPU checks of Bob's MtA range proofs: the three-base joint tail against
Python's pow, fsdkr.mta.verify_bob against the test oracle (tests/mta_oracle.py)
on honest, tampered and edge inputs, and generate_bob bit for bit against the
oracle's prover for the same draws."""
import numpy as np
import pytest

import mta_oracle as mo
from oracle import secp256k1 as ec
from oracle.paillier import EncryptionKey
from oracle.rng import Rng

pytestmark = pytest.mark.gpu

Q3 = ec.Q ** 3


@pytest.fixture(scope="module")
def keys(gpu_ctx):
    """Two verifier key sets (Paillier ek / dk and a DLogStatement over its own N~),
    2048 bits, primes from the device's key generation."""
    from fsdkr import keygen
    rng = Rng("mta-gpu-keys")
    kps = keygen.keypairs_with_modulus_size(gpu_ctx, rng, 2048, 4)
    out = []
    for k in range(2):
        ek, dk = kps[2 * k]
        ekt, dkt = kps[2 * k + 1]
        out.append(dict(ek=EncryptionKey.from_n(ek.n), dk=dk, st=mo.dlog_statement(ekt.n, dkt.p, dkt.q, rng),
                        dkt=dkt))
    return out


@pytest.fixture(scope="module")
def honest(keys):
    """6 plain and 6 extended honest proofs under the two key sets, with the
    oracle's verdict (1) asserted once."""
    rng = Rng("mta-gpu-proofs")
    cases = []
    for k in range(12):
        key = keys[k % 2]
        a_enc, mta, b, beta_prim, r = mo.mta_scenario(key["ek"], rng)
        if k < 6:
            pf, X = mo.generate(a_enc, mta, b, beta_prim, key["ek"], key["st"], r, rng)[0], None
        else:
            pf, X = mo.generate_ext(a_enc, mta, b, beta_prim, key["ek"], key["st"], r, rng), ec.mul(ec.G, b)
        c = dict(pf=pf, a_enc=a_enc, mta=mta, X=X, key=key)
        assert _oracle(c) == 1
        cases.append(c)
    return cases


def _oracle(c):
    return mo.outcome(c["pf"], c["a_enc"], c["mta"], c["key"]["ek"], c["key"]["st"], c["X"])


def _gpu(ctx, cases, **kw):
    from fsdkr import mta
    ext = hasattr(cases[0]["pf"], "proof")
    assert all(hasattr(c["pf"], "proof") == ext for c in cases)
    return list(mta.verify_bob([c["pf"] for c in cases], [c["a_enc"] for c in cases], [c["mta"] for c in cases],
                               [c["key"]["ek"] for c in cases], [c["key"]["st"] for c in cases],
                               X=[c["X"] for c in cases] if ext else None, ctx=ctx, **kw))


def _both(ctx, cases):
    """GPU verdicts of a mixed list (plain and extended proofs go in one call each)."""
    out = [None] * len(cases)
    for ext in (False, True):
        ks = [k for k, c in enumerate(cases) if hasattr(c["pf"], "proof") == ext]
        if ks:
            for k, v in zip(ks, _gpu(ctx, [cases[k] for k in ks])):
                out[k] = int(v)
    return out


# ---- 1. fsdkr_modexp_joint3_batch ------------------------------------------------
def _joint3_cases(keys, count):
    mods = [keys[0]["ek"].nn, keys[1]["ek"].nn]
    mexp = [keys[0]["ek"].n, keys[1]["ek"].n]
    rng = Rng(("joint3", count))
    e2s = [0, 1, Q3, (1 << 768) - 1, (0xB << 764) | 0x1235, (1 << 200) + 3, rng.bits(768), rng.bits(255)]
    e3s = [0, 1, (1 << 256) - 1, rng.bits(199), rng.bits(256)]
    inst = []
    for i in range(count):
        m = (i * 7 // 3) % 2 if count > 1 else 0
        M = mods[m]
        b1 = [rng.sample_below(M), 1, M - 1][i % 3]
        b2 = [rng.sample_below(M), M - 1, 1, rng.sample_below(M)][i % 4]
        b3 = [rng.sample_below(M), rng.sample_below(M), 1, M - 1, rng.sample_below(M)][i % 5]
        inst.append((b1, b2, e2s[i % len(e2s)], b3, e3s[(i + i // 5) % len(e3s)], m))
    return mods, mexp, inst


def _check_joint3(ctx, mods, mexp, inst):
    B, B2, E2, B3, E3, I = (list(x) for x in zip(*inst))
    got = ctx.modexp_joint3_batch(B, B2, E2, B3, E3, mods, mexp, I)
    want = [pow(b, mexp[m], mods[m]) * pow(b2, e2, mods[m]) * pow(b3, e3, mods[m]) % mods[m]
            for b, b2, e2, b3, e3, m in inst]
    assert got == want
    # the third base absent: the two-base tail at the same split
    got2 = ctx.modexp_joint3_batch(B, B2, E2, None, None, mods, mexp, I)
    want2 = [pow(b, mexp[m], mods[m]) * pow(b2, e2, mods[m]) % mods[m] for b, b2, e2, _, _, m in inst]
    assert got2 == want2
    small = [k for k, e2 in enumerate(E2) if e2 < (1 << 256)]
    if small:
        ref = ctx.modexp_joint_batch([B[k] for k in small], [B2[k] for k in small], [E2[k] for k in small], mods,
                                     mexp, [I[k] for k in small])
        assert [got2[k] for k in small] == ref


@pytest.mark.parametrize("count", [1, 5, 13])
def test_joint3_matches_pow(gpu_ctx, keys, count):
    _check_joint3(gpu_ctx, *_joint3_cases(keys, count))


def test_joint3_edges(gpu_ctx, keys):
    """Every edge exponent against every edge base, and an all-ones-limb modulus."""
    ones = (1 << 4096) - 1
    mods = [keys[0]["ek"].nn, ones]
    mexp = [keys[0]["ek"].n, keys[1]["ek"].n]
    rng = Rng("joint3-edges")
    e2s = [0, 1, Q3, (1 << 768) - 1, (0xF << 764) | 1, (1 << 200) + 3]
    e3s = [0, 1, (1 << 256) - 1, rng.bits(199)]
    inst = []
    for k, e2 in enumerate(e2s):
        for j, e3 in enumerate(e3s):
            m = (k + j) % 2
            M = mods[m]
            bs = [1, M - 1, rng.sample_below(M)]
            inst.append((bs[(k + j) % 3], bs[(k + 2 * j + 1) % 3], e2, bs[(2 * k + j + 2) % 3], e3, m))
    _check_joint3(gpu_ctx, mods, mexp, inst)


@pytest.mark.parametrize("lanes", [4, 8, 32])
def test_joint3_lane_counts(gpu_ctx, keys, lanes):
    mods, mexp, inst = _joint3_cases(keys, 5)
    gpu_ctx.set_modexp_group(lanes)
    try:
        _check_joint3(gpu_ctx, mods, mexp, inst)
    finally:
        gpu_ctx.set_modexp_group(0)


# ---- 2. honest and tampered proofs ---------------------------------------------
def test_verify_bob_honest_and_tampered(gpu_ctx, honest):
    cases = list(honest)
    for k, kind in enumerate(mo.TAMPERS):
        src = honest[6 + k % 6] if (kind in ("X", "u") or k % 2) else honest[k % 6]
        pf, a_enc, mta, X = mo.tamper(kind, src["pf"], src["a_enc"], src["mta"], src["X"])
        bad = dict(pf=pf, a_enc=a_enc, mta=mta, X=X, key=src["key"])
        assert _oracle(bad) == 0, kind      # a no-op tamper would hide a miss
        cases.append(bad)
    want = [1] * 12 + [0] * 12
    assert [_oracle(c) for c in cases[12:]] == want[12:]
    assert _both(gpu_ctx, cases) == want


def test_verify_bob_unfused_agrees(gpu_ctx, honest):
    cases = honest[:3] + [dict(honest[3], a_enc=honest[3]["a_enc"] + 1)]
    assert _gpu(gpu_ctx, cases, fused=False) == [1, 1, 1, 0]
    ext = honest[6:8] + [dict(honest[8], mta=honest[8]["mta"] + 1)]
    assert _gpu(gpu_ctx, ext, fused=False) == [1, 1, 0]


# ---- 3. edge outcomes ----------------------------------------------------------
def test_verify_bob_edges(gpu_ctx, honest):
    plain, ext = honest[0], honest[6]
    key = plain["key"]
    N, NN = key["ek"].n, key["ek"].nn
    cases = []
    cases.append(dict(plain, pf=mo.with_field(plain["pf"], "s1", Q3 + 1)))
    cases.append(dict(plain, mta=key["dk"].p))                               # a non-unit modulo N^2
    cases.append(dict(plain, pf=mo.with_field(plain["pf"], "z", key["dkt"].p)))   # shares a factor with N~
    assert plain["pf"].t1 > N
    cases.append(plain)                                                      # t1 > N, honest
    small = next(c for c in honest[:6] if c["a_enc"] + c["key"]["ek"].nn < (1 << 4096))
    cases.append(dict(small, a_enc=small["a_enc"] + small["key"]["ek"].nn))  # hashed as given
    cases.append(dict(plain, pf=mo.with_field(plain["pf"], "e", plain["pf"].e + (1 << 256))))
    cases.append(dict(ext, X=None))
    cases.append(dict(ext, pf=type(ext["pf"])(ext["pf"].proof, None)))
    cases.append(dict(ext, X=ec.add(ext["X"], ec.G)))
    # the s1 bound and the inverses come before the coordinates' unwrap
    cases.append(dict(ext, X=None, pf=mo.with_field(ext["pf"], "s1", Q3 + 1)))
    cases.append(dict(ext, X=None, mta=ext["key"]["dk"].q))
    want = [_oracle(c) for c in cases]
    assert want == [0, 0, 0, 1, 0, 0, 2, 2, 0, 0, 0]
    assert _both(gpu_ctx, cases) == want


# ---- 4. the prover -------------------------------------------------------------
@pytest.mark.parametrize("check", [False, True])
def test_generate_bob_matches_oracle(gpu_ctx, keys, check):
    from fsdkr import mta
    srng = Rng(("mta-gen", check))
    items = []
    for k in range(4):
        key = keys[k % 2]
        a_enc, m, b, beta_prim, r = mo.mta_scenario(key["ek"], srng)
        items.append((a_enc, m, b, beta_prim, key["ek"], key["st"], r))
    # the oracle proves one by one, generate_bob draws proof by proof in the same order
    orng = Rng(("mta-gen-draws", check))
    want = []
    for it in items:
        pf, u = mo.generate(*it, orng, check=check)
        want.append((pf, u))
    got = mta.generate_bob(items, Rng(("mta-gen-draws", check)), ctx=gpu_ctx, check=check)
    for g, (pf, u) in zip(got, want):
        inner = g.proof if check else g
        assert [getattr(inner, f) for f in mo.FIELDS] == [getattr(pf, f) for f in mo.FIELDS]
        if check:
            assert g.u == u
    X = [ec.mul(ec.G, it[2]) for it in items] if check else None
    v = mta.verify_bob(got, [it[0] for it in items], [it[1] for it in items], [it[4] for it in items],
                       [it[5] for it in items], X=X, ctx=gpu_ctx)
    assert v.dtype == np.uint8 and list(v) == [1] * 4
