"""GPU checks of the one-call MtA provers (fsdkr_bob_prove, fsdkr_alice_prove;
fsdkr.mta.generate_bob / generate_alice / respond / initiate with one_call=True):
the proofs equal the oracle's provers field by field under the same seeded stream
and the default path's bit for bit, both verifiers accept them, and a recording
context shows exactly one bob_prove / alice_prove call and no other device call.
Keys: two device-generated 2048-bit sets around the golden 1024-bit key, one
3072-bit set.  The C-ABI edge rows (extreme witnesses and draws, all-ones rows, the
short transcripts of a key with h1 = 1, h2 = N~ - 1) are driven through
Context.bob_prove / alice_prove with chosen "draws" against pow, hashlib and Python
integers; counts 1, 63, 64, 65 (the 64-thread blocks of the challenge and response
launches) run under the 1024-bit key; then the error returns."""
import ctypes
import dataclasses
import hashlib
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import codec  # noqa: E402
import mta_oracle as mo  # noqa: E402
from oracle import paillier  # noqa: E402
from oracle import range_proofs as rp  # noqa: E402
from oracle import secp256k1 as ec  # noqa: E402
from oracle.paillier import EncryptionKey  # noqa: E402
from oracle.rng import Rng  # noqa: E402

pytestmark = pytest.mark.gpu

RECORDED = ("bob_prove", "alice_prove", "pedersen_commit", "bob_commit_v", "modexp_batch", "paillier_encrypt",
            "mta_respond", "ec_mul_g")
COUNTS = [1, 63, 64, 65]


@pytest.fixture(scope="module")
def rec_ctx():
    """A context of its own that records the device calls the provers issue."""
    from fsdkr import Context

    class Recorder(Context):
        def __init__(self):
            super().__init__()
            self.calls = []

    def wrap(name):
        def call(self, *a, **kw):
            self.calls.append(name)
            return getattr(Context, name)(self, *a, **kw)
        return call

    for name in RECORDED:
        setattr(Recorder, name, wrap(name))
    ctx = Recorder()
    yield ctx
    ctx.close()


def _key_sets(ctx, rng, bits, sets):
    from fsdkr import keygen
    kps = keygen.keypairs_with_modulus_size(ctx, rng, bits, 2 * sets)
    out = []
    for k in range(sets):
        ek, dk = kps[2 * k]
        ekt, dkt = kps[2 * k + 1]
        out.append(dict(ek=EncryptionKey.from_n(ek.n), st=mo.dlog_statement(ekt.n, dkt.p, dkt.q, rng)))
    return out


@pytest.fixture(scope="module")
def golden():
    """The golden 1024-bit key: its first Paillier key, its second statement."""
    raw = codec.load_raw("transcript_join_t1_n4_kb1024.json.gz")
    assert raw["meta"]["key_bits"] == 1024
    gk = codec.dec(raw["keys"], codec.product_classes())[0]
    return dict(ek=EncryptionKey.from_n(gk.paillier_key_vec[0].n), st=gk.h1_h2_n_tilde_vec[1])


@pytest.fixture(scope="module")
def sets64(rec_ctx, golden):
    a, b = _key_sets(rec_ctx, Rng("mta-prove-keys"), 2048, 2)
    return [a, golden, b]


@pytest.fixture(scope="module")
def sets96(rec_ctx):
    return _key_sets(rec_ctx, Rng("mta-prove-keys-96"), 3072, 1)


def _bob_items(sets, n, seed):
    items = []
    for k in range(n):
        key = sets[k % len(sets)]
        a_enc, m, b, beta_prim, r = mo.mta_scenario(key["ek"], Rng((seed, k)))
        items.append((a_enc, m, b, beta_prim, key["ek"], key["st"], r))
    return items


def _alice_items(sets, n, seed):
    items = []
    for k in range(n):
        key = sets[k % len(sets)]
        rng = Rng((seed, k))
        a, r = rng.sample_below(ec.Q), rng.from_modulo(key["ek"].n)
        items.append((a, paillier.encrypt_with_chosen_randomness(key["ek"], a, r), key["ek"], key["st"], r))
    return items


def _check_bob(ctx, items, seed):
    from fsdkr import mta
    n = len(items)
    ctx.calls.clear()
    got = mta.generate_bob(items, Rng(seed), ctx=ctx, one_call=True)
    assert ctx.calls == ["bob_prove"]
    orng = Rng(seed)
    for g, it in zip(got, items):
        pf, _ = mo.generate(*it, orng)
        assert [getattr(g, f) for f in mo.FIELDS] == [getattr(pf, f) for f in mo.FIELDS]
    assert mta.generate_bob(items, Rng(seed), ctx=ctx) == got
    a_encs, mtas = [it[0] for it in items], [it[1] for it in items]
    eks, sts = [it[4] for it in items], [it[5] for it in items]
    assert list(mta.verify_bob(got, a_encs, mtas, eks, sts, ctx=ctx)) == [1] * n
    assert [mo.outcome(p, a, m, ek, st) for p, a, m, ek, st in zip(got, a_encs, mtas, eks, sts)] == [1] * n


def _check_alice(ctx, items, seed):
    from fsdkr import mta
    n = len(items)
    ctx.calls.clear()
    got = mta.generate_alice(items, Rng(seed), ctx=ctx, one_call=True)
    assert ctx.calls == ["alice_prove"]
    orng = Rng(seed)
    for g, it in zip(got, items):
        assert dataclasses.astuple(g) == dataclasses.astuple(rp.generate(*it, orng))
    assert mta.generate_alice(items, Rng(seed), ctx=ctx) == got
    ciphers, eks, sts = [it[1] for it in items], [it[2] for it in items], [it[3] for it in items]
    assert list(mta.verify_alice(got, ciphers, eks, sts, ctx=ctx)) == [1] * n


def test_bob_one_call_2048(rec_ctx, sets64):
    _check_bob(rec_ctx, _bob_items(sets64, 6, "mta-prove-bob"), "mta-prove-bob-draws")


def test_bob_one_call_3072(rec_ctx, sets96):
    _check_bob(rec_ctx, _bob_items(sets96, 2, "mta-prove-bob-96"), "mta-prove-bob-draws-96")


def test_alice_one_call_2048(rec_ctx, sets64):
    _check_alice(rec_ctx, _alice_items(sets64, 6, "mta-prove-alice"), "mta-prove-alice-draws")


def test_alice_one_call_3072(rec_ctx, sets96):
    _check_alice(rec_ctx, _alice_items(sets96, 2, "mta-prove-alice-96"), "mta-prove-alice-draws-96")


def test_respond_and_initiate_one_call(rec_ctx, sets64):
    from fsdkr import mta
    rng = Rng("mta-prove-exchange")
    keys = [sets64[k % 3] for k in range(4)]
    eks, sts = [k["ek"] for k in keys], [k["st"] for k in keys]
    as_ = [rng.sample_below(ec.Q) for _ in keys]
    want = mta.initiate(as_, eks, sts, Rng("init"), ctx=rec_ctx)
    rec_ctx.calls.clear()
    assert mta.initiate(as_, eks, sts, Rng("init"), ctx=rec_ctx, one_call=True) == want
    assert rec_ctx.calls == ["paillier_encrypt", "alice_prove"]
    bs = [rng.sample_below(ec.Q) for _ in keys]
    want_r = mta.respond(want[0], bs, eks, sts, Rng("resp"), ctx=rec_ctx)
    rec_ctx.calls.clear()
    assert mta.respond(want[0], bs, eks, sts, Rng("resp"), ctx=rec_ctx, one_call=True) == want_r
    assert rec_ctx.calls == ["mta_respond", "bob_prove"]


# ---- C-ABI rows against pow / hashlib / integers -----------------------------------

def _h(*vals):
    """DigestExt::chain_bigint: SHA-256 over the minimal big-endian bytes (0 -> one 0x00)."""
    d = hashlib.sha256()
    for v in vals:
        d.update(v.to_bytes(max(1, (v.bit_length() + 7) // 8), "big"))
    return int.from_bytes(d.digest(), "big")


def _ones(limbs):
    return (1 << 32 * limbs) - 1


def _bob_expect(key, a_enc, mta, w):
    N, Nt, h1, h2 = key
    NN = N * N
    z = pow(h1, w["b"], Nt) * pow(h2, w["ro"], Nt) % Nt
    zp = pow(h1, w["alpha"], Nt) * pow(h2, w["ro_prim"], Nt) % Nt
    t = pow(h1, w["beta_prim"], Nt) * pow(h2, w["sigma"], Nt) % Nt
    ww = pow(h1, w["gamma"], Nt) * pow(h2, w["tau"], Nt) % Nt
    v = pow(a_enc, w["alpha"], NN) * (1 + w["gamma_mod_n"] * N) * pow(w["beta"], N, NN) % NN
    e = _h(N, N + 1, a_enc, mta, z, zp, t, v, ww)
    return dict(z=z, t=t, e=e, s=pow(w["r"], e, N) * w["beta"] % N, s1=e * w["b"] + w["alpha"],
                s2=e * w["ro"] + w["ro_prim"], t1=e * w["beta_prim"] + w["gamma"], t2=e * w["sigma"] + w["tau"]), (zp, v, ww)


def _alice_expect(key, cipher, w):
    N, Nt, h1, h2 = key
    NN = N * N
    z = pow(h1, w["a"], Nt) * pow(h2, w["ro"], Nt) % Nt
    ww = pow(h1, w["alpha"], Nt) * pow(h2, w["gamma"], Nt) % Nt
    u = (1 + w["alpha"] * N) * pow(w["beta"], N, NN) % NN
    e = _h(N, N + 1, cipher, z, u, ww)
    return dict(z=z, e=e, s=pow(w["r"], e, N) * w["beta"] % N, s1=e * w["a"] + w["alpha"], s2=e * w["ro"] + w["gamma"]), (u, ww)


def _edge_keys(golden):
    N, st = golden["ek"].n, golden["st"]
    return [(N, st.N, st.g % st.N, st.ni % st.N), (N, st.N, 1, st.N - 1)]   # the structured key: h1 = 1, h2 = N~ - 1


def test_bob_edge_rows(rec_ctx, golden):
    from fsdkr import _native
    nl = 64
    keys = _edge_keys(golden)
    N = keys[0][0]
    rng = Rng("mta-prove-bob-edges")
    win, _ = _native.bob_prove_widths(nl)
    rnd = {f: rng.bits(32 * l - 1) for f, l in win.items()}
    rnd.update(beta=rng.from_modulo(N), r=rng.sample_below(N), beta_prim=rng.sample_below(N))
    rows = []   # (key, a_enc, mta, witness)
    a0, m0 = rng.sample_below(N * N), rng.sample_below(N * N)
    # the ends of b, alpha, beta'; all-ones rows of ro, sigma, ro', tau, gamma
    rows.append((0, a0, m0, dict(rnd, b=0, alpha=0, beta_prim=N - 1)))
    rows.append((0, a0, m0, dict(rnd, b=(1 << 256) - 1, alpha=(1 << 768) - 1, beta_prim=0)))
    rows.append((1, a0, m0, dict(rnd, **{f: _ones(win[f]) for f in ("ro", "sigma", "ro_prim", "tau", "gamma")})))
    # every row all ones that may be: b, alpha and the five above (r, beta, beta' stay below N)
    rows.append((0, a0, m0, dict(rnd, **{f: _ones(win[f]) for f in ("b", "alpha", "ro", "sigma", "ro_prim", "tau", "gamma")})))
    # short transcripts: commitments 1 or N~ - 1, v = 1, mta = 0 (one 0x00 byte)
    rows.append((1, 1, 0, dict(rnd, beta=1, gamma=0)))
    rows.append((1, 1, 0, dict(rnd, beta=1, gamma=3 * N, ro=rnd["ro"] | 1, ro_prim=rnd["ro_prim"] & ~1)))
    for _, _, _, w in rows:
        w["gamma_mod_n"] = w["gamma"] % N
    got = rec_ctx.bob_prove(keys, [r[0] for r in rows], nl, [r[1] for r in rows], [r[2] for r in rows],
                            **{f: [r[3][f] for r in rows] for f in _native.BobProveC.SECRET})
    for i, (k, a_enc, mta, w) in enumerate(rows):
        want, (zp, v, ww) = _bob_expect(keys[k], a_enc, mta, w)
        assert {f: got[f][i] for f in want} == want, i
        if k == 1:
            assert {want["z"], zp, want["t"], ww} <= {1, keys[1][1] - 1}
        if a_enc == 1:
            assert v == 1
    # the carry case of every response: e x + y reaches its top limb's neighbourhood
    assert got["s2"][3].bit_length() > 32 * (nl + 23)


def test_alice_edge_rows(rec_ctx, golden):
    from fsdkr import _native
    nl = 64
    keys = _edge_keys(golden)
    N = keys[0][0]
    rng = Rng("mta-prove-alice-edges")
    win, _ = _native.alice_prove_widths(nl)
    rnd = {f: rng.bits(32 * l - 1) for f, l in win.items()}
    rnd.update(beta=rng.from_modulo(N), r=rng.sample_below(N))
    c0 = rng.sample_below(N * N)
    rows = [(0, c0, dict(rnd, a=0, alpha=0)),
            (0, c0, dict(rnd, a=(1 << 768) - 1, alpha=(1 << 768) - 1)),
            (1, c0, dict(rnd, ro=_ones(win["ro"]), gamma=_ones(win["gamma"]))),
            (1, 0, dict(rnd, alpha=0, beta=1)),          # u = 1, cipher = 0: the short transcript
            (1, 1, dict(rnd, alpha=0, beta=1, a=1, ro=rnd["ro"] | 1))]
    got = rec_ctx.alice_prove(keys, [r[0] for r in rows], nl, [r[1] for r in rows],
                              **{f: [r[2][f] for r in rows] for f in _native.AliceProveC.SECRET})
    for i, (k, cipher, w) in enumerate(rows):
        want, (u, ww) = _alice_expect(keys[k], cipher, w)
        assert {f: got[f][i] for f in want} == want, i
        if k == 1:
            assert {want["z"], ww} <= {1, keys[1][1] - 1}
        if w["alpha"] == 0 and w["beta"] == 1:
            assert u == 1


# ---- counts on both sides of the 64-thread blocks -----------------------------------

@pytest.fixture(scope="module")
def bob_ref(golden):
    """65 proofs of the oracle under the 1024-bit key; the draws run proof by proof, so
    every count is a prefix."""
    items = _bob_items([golden], max(COUNTS), "mta-prove-counts")
    rng = Rng("mta-prove-count-draws")
    return items, [mo.generate(*it, rng)[0] for it in items]


@pytest.fixture(scope="module")
def alice_ref(golden):
    items = _alice_items([golden], max(COUNTS), "mta-prove-counts-alice")
    rng = Rng("mta-prove-count-draws-alice")
    return items, [rp.generate(*it, rng) for it in items]


@pytest.mark.parametrize("count", COUNTS)
def test_bob_counts(rec_ctx, bob_ref, count):
    from fsdkr import mta
    items, want = bob_ref
    got = mta.generate_bob(items[:count], Rng("mta-prove-count-draws"), ctx=rec_ctx, one_call=True)
    assert [[getattr(g, f) for f in mo.FIELDS] for g in got] == [[getattr(p, f) for f in mo.FIELDS] for p in want[:count]]


@pytest.mark.parametrize("count", COUNTS)
def test_alice_counts(rec_ctx, alice_ref, count):
    from fsdkr import mta
    items, want = alice_ref
    got = mta.generate_alice(items[:count], Rng("mta-prove-count-draws-alice"), ctx=rec_ctx, one_call=True)
    assert [dataclasses.astuple(g) for g in got] == [dataclasses.astuple(p) for p in want[:count]]


# ---- error returns -------------------------------------------------------------------

def _bob_call(ctx, keys, nl=64, key_idx=(0,), a_enc=None):
    from fsdkr import _native
    win, _ = _native.bob_prove_widths(nl)
    return ctx.bob_prove(keys, list(key_idx), nl, [7 if a_enc is None else a_enc], [9], **{f: [5] for f in win})


def _alice_call(ctx, keys, nl=64, key_idx=(0,)):
    from fsdkr import _native
    win, _ = _native.alice_prove_widths(nl)
    return ctx.alice_prove(keys, list(key_idx), nl, [7], **{f: [5] for f in win})


def test_error_returns(rec_ctx, golden):
    from fsdkr import _native
    N, Nt, h1, h2 = _edge_keys(golden)[0]
    bad_keys = {"even N": (N + 1, Nt, h1, h2), "N = 1": (1, Nt, h1, h2), "even N~": (N, Nt + 1, h1, h2),
                "N~ = 1": (N, 1, 0, 0), "h1 = N~": (N, Nt, Nt, h2), "h2 > N~": (N, Nt, h1, Nt + 2)}
    for what, key in bad_keys.items():
        for call in (lambda: _bob_call(rec_ctx, [key]), lambda: _alice_call(rec_ctx, [key])):
            with pytest.raises(_native.FsdkrError) as ei:
                call()
            assert ei.value.code == _native.FSDKR_E_ARG, what
    good = [(N, Nt, h1, h2)]
    for call in (lambda: _bob_call(rec_ctx, good, key_idx=(1,)), lambda: _alice_call(rec_ctx, good, key_idx=(1,)),
                 lambda: _bob_call(rec_ctx, good, a_enc=N * N)):
        with pytest.raises(_native.FsdkrError) as ei:
            call()
        assert ei.value.code == _native.FSDKR_E_ARG
    # a width class that is none
    L, h = rec_ctx._lib, rec_ctx.handle
    for fn, bcls, ocls in ((L.fsdkr_bob_prove, _native.BobProveC, _native.BobProofsC),
                           (L.fsdkr_alice_prove, _native.AliceProveC, _native.AliceProofsC)):
        b, o = bcls(), ocls()
        b.count, b.n_keys, b.nl = 1, 1, 32
        assert fn(h, ctypes.byref(b), ctypes.byref(o)) == _native.FSDKR_E_UNSUPPORTED
        b.nl = 64   # every pointer NULL
        assert fn(h, ctypes.byref(b), ctypes.byref(o)) == _native.FSDKR_E_ARG
        assert fn(h, None, ctypes.byref(o)) == _native.FSDKR_E_ARG
        assert fn(h, ctypes.byref(b), None) == _native.FSDKR_E_ARG
        b.count = 0
        assert fn(h, ctypes.byref(b), None) == _native.FSDKR_OK
    # a forced lane count that the comb refuses: the comb's error
    rec_ctx.set_modexp_group(16)
    try:
        with pytest.raises(_native.FsdkrError) as ei:
            _bob_call(rec_ctx, good)
        assert ei.value.code == _native.FSDKR_E_ARG
    finally:
        rec_ctx.set_modexp_group(0)
    # the context still proves after the refusals
    assert _bob_call(rec_ctx, good)["e"][0] > 0


def test_one_call_value_errors_record_no_call(rec_ctx, golden):
    from fsdkr import mta
    it = _bob_items([golden], 1, "mta-prove-valueerrors")[0]
    ek = it[4]
    rec_ctx.calls.clear()
    for bad, kw in ((it, dict(check=True)), (it[:2] + (1 << 256,) + it[3:], {}), (it[:2] + (-1,) + it[3:], {}),
                    (it[:3] + (ek.n,) + it[4:], {}), (it[:3] + (-1,) + it[4:], {}), ((ek.nn,) + it[1:], {})):
        with pytest.raises(ValueError):
            mta.generate_bob([bad], Rng("x"), ctx=rec_ctx, one_call=True, **kw)
    assert rec_ctx.calls == []
