"""GPU checks of Bob's MtA range proofs for 3072-bit keys (width class nl = 96):
the 6144-bit three-base split chain against Python's pow, fsdkr.mta.verify_bob
against the test oracle (tests/mta_oracle.py) on honest, tampered, non-unit and
edge inputs, 2048- and 3072-bit keys in one call, and generate_bob bit for bit
against the oracle's prover for the same draws.  Every comparison is exact."""
import numpy as np
import pytest

import mta_oracle as mo
from oracle import secp256k1 as ec
from oracle.paillier import EncryptionKey
from oracle.rng import Rng

pytestmark = pytest.mark.gpu

Q3 = ec.Q ** 3
K = 192   # limbs of N^2 for 3072-bit keys


def _key_sets(ctx, rng, bits, sets):
    from fsdkr import keygen
    kps = keygen.keypairs_with_modulus_size(ctx, rng, bits, 2 * sets)
    out = []
    for k in range(sets):
        ek, dk = kps[2 * k]
        ekt, dkt = kps[2 * k + 1]
        out.append(dict(ek=EncryptionKey.from_n(ek.n), dk=dk, st=mo.dlog_statement(ekt.n, dkt.p, dkt.q, rng),
                        dkt=dkt))
    return out


@pytest.fixture(scope="module")
def keys(gpu_ctx):
    """Two verifier key sets (Paillier ek / dk and a DLogStatement over its own N~),
    3072 bits, and one 2048-bit set for the mixed call (keys[2]); primes from the
    device's key generation."""
    rng = Rng("mta3072-gpu-keys")
    return _key_sets(gpu_ctx, rng, 3072, 2) + _key_sets(gpu_ctx, rng, 2048, 1)


def _prove(key, rng, ext):
    a_enc, mta, b, beta_prim, r = mo.mta_scenario(key["ek"], rng)
    if not ext:
        pf, X = mo.generate(a_enc, mta, b, beta_prim, key["ek"], key["st"], r, rng)[0], None
    else:
        pf, X = mo.generate_ext(a_enc, mta, b, beta_prim, key["ek"], key["st"], r, rng), ec.mul(ec.G, b)
    return dict(pf=pf, a_enc=a_enc, mta=mta, X=X, key=key)


@pytest.fixture(scope="module")
def honest(keys):
    """3 plain and 3 extended honest proofs under the two 3072-bit key sets, with
    the oracle's verdict (1) asserted once."""
    rng = Rng("mta3072-gpu-proofs")
    cases = [_prove(keys[k % 2], rng, k >= 3) for k in range(6)]
    assert [_oracle(c) for c in cases] == [1] * 6
    return cases


def _oracle(c):
    return mo.outcome(c["pf"], c["a_enc"], c["mta"], c["key"]["ek"], c["key"]["st"], c["X"])


def _args(cases):
    ext = hasattr(cases[0]["pf"], "proof")
    assert all(hasattr(c["pf"], "proof") == ext for c in cases)
    return ([c["pf"] for c in cases], [c["a_enc"] for c in cases], [c["mta"] for c in cases],
            [c["key"]["ek"] for c in cases], [c["key"]["st"] for c in cases]), ([c["X"] for c in cases] if ext else None)


def _gpu(ctx, cases, **kw):
    from fsdkr import mta
    args, X = _args(cases)
    return [int(v) for v in mta.verify_bob(*args, X=X, ctx=ctx, **kw)]


def _both(ctx, cases, **kw):
    """GPU verdicts of a mixed list (plain and extended proofs go in one call each)."""
    out = [None] * len(cases)
    for ext in (False, True):
        ks = [k for k, c in enumerate(cases) if hasattr(c["pf"], "proof") == ext]
        if ks:
            for k, v in zip(ks, _gpu(ctx, [cases[k] for k in ks], **kw)):
                out[k] = v
    return out


# ---- 1. fsdkr_modexp_joint3_batch_k at 192 limbs -----------------------------------
def _joint3_cases(keys, count):
    mods = [keys[0]["ek"].nn, keys[1]["ek"].nn]
    mexp = [keys[0]["ek"].n, keys[1]["ek"].n]
    rng = Rng(("joint3-192", count))
    e2s = [0, 1, Q3, (1 << 768) - 1, (0xB << 764) | 0x1235, (1 << 200) + 3, rng.bits(768)]
    e3s = [0, 1, (1 << 256) - 1, rng.bits(256)]
    inst = []
    for i in range(count):
        m = (i * 7 // 3) % 2 if count > 1 else 0
        M = mods[m]
        b1 = [rng.sample_below(M), 1, M - 1][i % 3]
        b2 = [rng.sample_below(M), M - 1, 1, rng.sample_below(M)][i % 4]
        b3 = [rng.sample_below(M), rng.sample_below(M), 1, M - 1, rng.sample_below(M)][i % 5]
        inst.append((b1, b2, e2s[i % len(e2s)], b3, e3s[(i + i // 4) % len(e3s)], m))
    return mods, mexp, inst


def _want3(mods, mexp, inst):
    return [pow(b, mexp[m], mods[m]) * pow(b2, e2, mods[m]) * pow(b3, e3, mods[m]) % mods[m]
            for b, b2, e2, b3, e3, m in inst]


def _check_joint3(ctx, mods, mexp, inst, two_base=True):
    B, B2, E2, B3, E3, I = (list(x) for x in zip(*inst))
    got = ctx.modexp_joint3_batch(B, B2, E2, B3, E3, mods, mexp, I, k32=K)
    assert got == _want3(mods, mexp, inst)
    if two_base:   # base3 = None: the two-base tail at the same split
        got2 = ctx.modexp_joint3_batch(B, B2, E2, None, None, mods, mexp, I, k32=K)
        assert got2 == [pow(b, mexp[m], mods[m]) * pow(b2, e2, mods[m]) % mods[m] for b, b2, e2, _, _, m in inst]
    return got


@pytest.mark.parametrize("count", [1, 5, 9])
def test_joint3_192_matches_pow(gpu_ctx, keys, count):
    _check_joint3(gpu_ctx, *_joint3_cases(keys, count), two_base=count == 5)


def test_joint3_192_edges(gpu_ctx, keys):
    """Every edge exponent pair against the edge bases, over a 3072-bit key's N^2, the
    all-ones 6144-bit modulus and a modulus shorter than 6144 bits (N^2 of a 2048-bit N)."""
    ones = (1 << 6144) - 1
    mods = [keys[0]["ek"].nn, ones, keys[2]["ek"].nn]
    mexp = [keys[0]["ek"].n, keys[1]["ek"].n, keys[2]["ek"].n]
    rng = Rng("joint3-192-edges")
    e2s = [0, 1, Q3, (1 << 768) - 1, (0xB << 764) | 0x1235, (1 << 200) + 3, rng.bits(768)]
    e3s = [0, 1, (1 << 256) - 1, rng.bits(256)]
    inst = []
    for k, e2 in enumerate(e2s):
        for j, e3 in enumerate(e3s):
            m = (k + j) % 3
            M = mods[m]
            bs = [1, M - 1, rng.sample_below(M)]
            inst.append((bs[(k + j) % 3], bs[(k + 2 * j + 1) % 3], e2, bs[(2 * k + j + 2) % 3], e3, m))
    _check_joint3(gpu_ctx, mods, mexp, inst)


def test_joint3_192_lane_counts(gpu_ctx, keys):
    """Forced to 8 lanes the results are the automatic ones; the 6144-bit chain has no
    other shape, so 4 or 16 forced lanes are an argument error."""
    from fsdkr import _native
    mods, mexp, inst = _joint3_cases(keys, 5)
    auto = _check_joint3(gpu_ctx, mods, mexp, inst, two_base=False)
    B, B2, E2, B3, E3, I = (list(x) for x in zip(*inst))
    try:
        gpu_ctx.set_modexp_group(8)
        assert gpu_ctx.modexp_joint3_batch(B, B2, E2, B3, E3, mods, mexp, I, k32=K) == auto
        for lanes in (4, 16):
            gpu_ctx.set_modexp_group(lanes)
            with pytest.raises(_native.FsdkrError) as err:
                gpu_ctx.modexp_joint3_batch(B, B2, E2, B3, E3, mods, mexp, I, k32=K)
            assert err.value.code == _native.FSDKR_E_ARG and "8 lanes" in str(err.value)
    finally:
        gpu_ctx.set_modexp_group(0)
    with pytest.raises(_native.FsdkrError) as err:
        gpu_ctx.modexp_joint3_batch(B, B2, E2, B3, E3, mods, mexp, I, k32=256)   # no such width class
    assert err.value.code == _native.FSDKR_E_UNSUPPORTED


# ---- 2. the batched inverse at 96 and 192 limbs ------------------------------------
def test_verify_bob_3072_non_units(gpu_ctx, honest):
    """z, t (mod N~) and mta_out (mod N^2) sharing a prime factor with their modulus:
    the simultaneous inversion of their group falls back to one inverse per element."""
    plain = honest[0]
    key = plain["key"]
    cases = [plain,
             dict(plain, pf=mo.with_field(plain["pf"], "z", 3 * key["dkt"].p)),
             dict(plain, pf=mo.with_field(plain["pf"], "t", key["dkt"].q)),
             dict(plain, mta=5 * key["dk"].p),
             honest[2]]
    want = [_oracle(c) for c in cases]
    assert want == [1, 0, 0, 0, 1]
    assert _gpu(gpu_ctx, cases) == want


def test_verify_bob_3072_inverse_groups(gpu_ctx, honest):
    """40 proofs of one key: more than one 32-wide inversion group per modulus (two
    mod N^2, three mod N~ over z^e | t^e), a non-unit in the second group of each."""
    plain = honest[0]
    key = plain["key"]
    bad_m = dict(plain, mta=key["dk"].q)
    bad_z = dict(plain, pf=mo.with_field(plain["pf"], "z", key["dkt"].p))
    tam = dict(plain, a_enc=plain["a_enc"] + 1)
    verdict = {id(plain): 1, id(bad_m): _oracle(bad_m), id(bad_z): _oracle(bad_z), id(tam): _oracle(tam)}
    assert (verdict[id(bad_m)], verdict[id(bad_z)], verdict[id(tam)]) == (0, 0, 0)
    cases = [plain] * 40
    cases[35], cases[37], cases[3] = bad_m, bad_z, tam
    assert _gpu(gpu_ctx, cases) == [verdict[id(c)] for c in cases]


# ---- 3. honest and tampered proofs -------------------------------------------------
@pytest.fixture(scope="module")
def tampered(honest):
    """Every single-field tamper of the 2048-bit test, on the 3072-bit proofs, with the
    oracle's verdicts."""
    cases = []
    for k, kind in enumerate(mo.TAMPERS):
        src = honest[3 + k % 3] if (kind in ("X", "u") or k % 2) else honest[k % 3]
        pf, a_enc, mta, X = mo.tamper(kind, src["pf"], src["a_enc"], src["mta"], src["X"])
        cases.append(dict(pf=pf, a_enc=a_enc, mta=mta, X=X, key=src["key"]))
    want = [_oracle(c) for c in cases]
    assert want == [0] * len(mo.TAMPERS)      # a no-op tamper would hide a miss
    return cases, want


def test_verify_bob_3072_honest_and_tampered(gpu_ctx, honest, tampered):
    from fsdkr import mta
    cases = list(honest) + tampered[0]
    args, _ = _args(honest[:3])
    assert mta.prepass(*args)["nl"] == 96
    assert _both(gpu_ctx, cases) == [1] * 6 + tampered[1]


def test_verify_bob_3072_unfused_agrees(gpu_ctx, honest, tampered):
    cases = list(honest) + tampered[0]
    assert _both(gpu_ctx, cases, fused=False) == [1] * 6 + tampered[1]


# ---- 4. edge outcomes ---------------------------------------------------------------
def test_verify_bob_3072_edges(gpu_ctx, honest):
    plain, ext = honest[0], honest[3]
    key = plain["key"]
    N = key["ek"].n
    cases = []
    cases.append(dict(plain, pf=mo.with_field(plain["pf"], "s1", Q3)))          # accepted arithmetically
    cases.append(dict(plain, pf=mo.with_field(plain["pf"], "s1", Q3 + 1)))      # the bound (:374)
    cases.append(dict(plain, pf=mo.with_field(plain["pf"], "e", 0)))
    cases.append(dict(plain, pf=mo.with_field(plain["pf"], "e", plain["pf"].e + (1 << 256))))
    small = next(c for c in honest[:3] if c["a_enc"] + c["key"]["ek"].nn < (1 << 6144))
    cases.append(dict(small, a_enc=small["a_enc"] + small["key"]["ek"].nn))     # at or above N^2: hashed as given
    assert plain["pf"].t1 > N
    cases.append(plain)                                                         # t1 wider than N, honest
    cases.append(dict(plain, pf=mo.with_field(plain["pf"], "t1", plain["pf"].t1 + N)))   # equal mod N, hashed w differs
    cases.append(dict(ext, X=None))
    cases.append(dict(ext, pf=type(ext["pf"])(ext["pf"].proof, None)))
    # the s1 bound and the inverses come before the coordinates' unwrap
    cases.append(dict(ext, X=None, pf=mo.with_field(ext["pf"], "s1", Q3 + 1)))
    cases.append(dict(ext, X=None, mta=ext["key"]["dk"].q))
    cases.append(dict(ext, pf=type(ext["pf"])(mo.with_field(ext["pf"].proof, "z", ext["key"]["dkt"].p), None)))
    want = [_oracle(c) for c in cases]
    assert want == [0, 0, 0, 0, 0, 1, 0, 2, 2, 0, 0, 0]
    assert _both(gpu_ctx, cases) == want


# ---- 5. 2048- and 3072-bit keys in one call -----------------------------------------
def test_verify_bob_mixed_widths(gpu_ctx, keys, honest):
    from fsdkr import mta
    narrow = _prove(keys[2], Rng("mta3072-mixed"), False)
    bad = dict(narrow, mta=narrow["mta"] + 1)
    assert (_oracle(narrow), _oracle(bad)) == (1, 0)
    args, _ = _args([narrow])
    assert mta.prepass(*args)["nl"] == 64             # alone: the 2048-bit class
    assert _gpu(gpu_ctx, [narrow, bad]) == [1, 0]
    cases = [narrow, honest[0], bad, dict(honest[1], a_enc=honest[1]["a_enc"] + 1)]
    args, _ = _args(cases)
    assert mta.prepass(*args)["nl"] == 96             # with a 3072-bit key: zero-extended
    want = [_oracle(c) for c in cases]
    assert want == [1, 1, 0, 0]
    assert _gpu(gpu_ctx, cases) == want
    assert _gpu(gpu_ctx, cases, fused=False) == want


# ---- 6. the prover -------------------------------------------------------------------
@pytest.mark.parametrize("check", [False, True])
def test_generate_bob_3072_matches_oracle(gpu_ctx, keys, check):
    from fsdkr import mta
    srng = Rng(("mta3072-gen", check))
    items = []
    for k in range(2):
        key = keys[k % 2]
        a_enc, m, b, beta_prim, r = mo.mta_scenario(key["ek"], srng)
        items.append((a_enc, m, b, beta_prim, key["ek"], key["st"], r))
    # the oracle proves one by one, generate_bob draws proof by proof in the same order
    orng = Rng(("mta3072-gen-draws", check))
    want = [mo.generate(*it, orng, check=check) for it in items]
    got = mta.generate_bob(items, Rng(("mta3072-gen-draws", check)), ctx=gpu_ctx, check=check)
    for g, (pf, u) in zip(got, want):
        inner = g.proof if check else g
        assert [getattr(inner, f) for f in mo.FIELDS] == [getattr(pf, f) for f in mo.FIELDS]
        if check:
            assert g.u == u
    X = [ec.mul(ec.G, it[2]) for it in items] if check else None
    v = mta.verify_bob(got, [it[0] for it in items], [it[1] for it in items], [it[4] for it in items],
                       [it[5] for it in items], X=X, ctx=gpu_ctx)
    assert v.dtype == np.uint8 and list(v) == [1] * 2
