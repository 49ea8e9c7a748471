"""Restatement of BobProof / BobProofExt (the respondent's MtA range proofs) from
the reference crate's src/range_proofs.rs:205-590 -- TEST INFRASTRUCTURE ONLY.

oracle/ holds the initiator's half (oracle/range_proofs.py: AliceProof); this
file adds the respondent's half over the same primitives.  A condition on which
the reference panics raises bigint.PanicError."""
from dataclasses import dataclass
from typing import Optional, Tuple

from oracle import bigint
from oracle import secp256k1 as ec
from oracle.hashing import chain_bigint
from oracle.paillier import EncryptionKey
from oracle.zk_paillier import DLogStatement


@dataclass(frozen=True)
class BobProof:                    # :346-356
    t: int
    z: int
    e: int
    s: int
    s1: int
    s2: int
    t1: int
    t2: int


@dataclass(frozen=True)
class BobProofExt:                 # :520-523
    proof: BobProof
    u: Optional[Tuple[int, int]]


def _coords(pt):
    """Point::x_coord().unwrap(), y_coord().unwrap() (:428-431, :486-489)."""
    if pt is None:
        raise bigint.PanicError("x_coord().unwrap() on the point at infinity")
    return pt


def _challenge(ek, a_enc, mta, z, z_prim, t, v, w, check):
    """:413-439 / :467-497; check = (X, u) or None."""
    vals = [ek.n, ek.n + 1, a_enc, mta, z, z_prim, t, v, w]
    if check is not None:
        X, u = check
        Xx, Xy = _coords(X)
        ux, uy = _coords(u)
        vals += [Xx, Xy, ux, uy]
    return chain_bigint(*vals)


def generate(a_enc: int, mta: int, b: int, beta_prim: int, ek: EncryptionKey, st: DLogStatement, r: int, rng,
             check: bool = False):
    """BobProof::generate (:448-515) with BobZkpRound1::from (:245-300) and
    BobZkpRound2::from (:313-335); b is the scalar's value in [0, q).  Returns
    (BobProof, u or None)."""
    q = ec.Q
    h1, h2, Nt = st.g, st.ni, st.N
    alpha = rng.sample_below(q ** 3)
    beta = rng.from_modulo(ek.n)
    gamma = rng.sample_below(q ** 2 * ek.n)
    ro = rng.sample_below(q * Nt)
    ro_prim = rng.sample_below(q ** 3 * Nt)
    sigma = rng.sample_below(q * Nt)
    tau = rng.sample_below(q ** 3 * Nt)
    z = bigint.mod_pow(h1, b, Nt) * bigint.mod_pow(h2, ro, Nt) % Nt
    z_prim = bigint.mod_pow(h1, alpha, Nt) * bigint.mod_pow(h2, ro_prim, Nt) % Nt
    t = bigint.mod_pow(h1, beta_prim, Nt) * bigint.mod_pow(h2, sigma, Nt) % Nt
    w = bigint.mod_pow(h1, gamma, Nt) * bigint.mod_pow(h2, tau, Nt) % Nt
    v = bigint.mod_pow(a_enc, alpha, ek.nn) * (gamma * ek.n + 1) * bigint.mod_pow(beta, ek.n, ek.nn) % ek.nn
    u = None
    chk = None
    if check:
        X = ec.mul(ec.G, b)
        u = ec.mul(ec.G, alpha)
        chk = (X, u)
    e = _challenge(ek, a_enc, mta, z, z_prim, t, v, w, chk)
    s = bigint.mod_pow(r, e, ek.n) * beta % ek.n
    return BobProof(t, z, e, s, e * b + alpha, e * ro + ro_prim, e * beta_prim + gamma, e * sigma + tau), u


def generate_ext(a_enc, mta, b, beta_prim, ek, st, r, rng) -> BobProofExt:
    """BobProofExt::generate (:564-589)."""
    pf, u = generate(a_enc, mta, b, beta_prim, ek, st, r, rng, check=True)
    return BobProofExt(pf, u)


def verify(pf: BobProof, a_enc: int, mta: int, ek: EncryptionKey, st: DLogStatement, check=None) -> bool:
    """BobProof::verify (:360-446); check = (X, u) or None."""
    N, NN = ek.n, ek.nn
    Nt, h1, h2 = st.N, st.g, st.ni
    if pf.s1 > ec.Q ** 3:
        return False
    z_e_inv = bigint.mod_inv(bigint.mod_pow(pf.z, pf.e, Nt), Nt)
    if z_e_inv is None:
        return False
    z_prim = bigint.mod_pow(h1, pf.s1, Nt) * bigint.mod_pow(h2, pf.s2, Nt) * z_e_inv % Nt
    mta_e_inv = bigint.mod_inv(bigint.mod_pow(mta, pf.e, NN), NN)
    if mta_e_inv is None:
        return False
    v = bigint.mod_pow(a_enc, pf.s1, NN) * bigint.mod_pow(pf.s, N, NN) * (pf.t1 * N + 1) * mta_e_inv % NN
    t_e_inv = bigint.mod_inv(bigint.mod_pow(pf.t, pf.e, Nt), Nt)
    if t_e_inv is None:
        return False
    w = bigint.mod_pow(h1, pf.t1, Nt) * bigint.mod_pow(h2, pf.t2, Nt) * t_e_inv % Nt
    return _challenge(ek, a_enc, mta, pf.z, z_prim, pf.t, v, w, check) == pf.e


def verify_ext(pfx: BobProofExt, a_enc: int, mta: int, ek: EncryptionKey, st: DLogStatement, X) -> bool:
    """BobProofExt::verify (:527-562)."""
    if not verify(pfx.proof, a_enc, mta, ek, st, (X, pfx.u)):
        return False
    x1 = ec.mul(ec.G, pfx.proof.s1)
    x2 = ec.add(ec.mul(X, pfx.proof.e), pfx.u)
    return x1 == x2


def outcome(pf, a_enc, mta, ek, st, X=None) -> int:
    """1 accepted, 0 rejected, 2 the reference panics: fsdkr.mta.verify_bob's verdict."""
    try:
        if not hasattr(pf, "proof"):
            return int(verify(pf, a_enc, mta, ek, st))
        return int(verify_ext(pf, a_enc, mta, ek, st, X))
    except bigint.PanicError:
        return 2


def mta_scenario(ek, rng):
    """One MtA exchange of the reference's bob_zkp test (:682-704): Alice's a and
    Enc(a); Bob's b, beta', r and mta = Enc(a)^b * Enc(beta'; r).  Returns
    (a_enc, mta, b, beta_prim, r)."""
    from oracle import paillier
    a = rng.sample_below(ec.Q)
    a_enc = paillier.encrypt(ek, a, rng)
    b = rng.sample_below(ec.Q)
    beta_prim = rng.sample_below(ek.n)
    r = rng.sample_below(ek.n)
    mta = paillier.add(ek, paillier.mul(ek, a_enc, b), paillier.encrypt_with_chosen_randomness(ek, beta_prim, r))
    return a_enc, mta, b, beta_prim, r


def dlog_statement(nt: int, p: int, q: int, rng) -> DLogStatement:
    """The reference tests' generate_init (:626-648) for a given N~ = p q: h1 random,
    h2 = h1^xhi with xhi invertible modulo phi."""
    phi = (p - 1) * (q - 1)
    h1 = rng.sample_below(nt)
    while True:
        xhi = rng.sample_below(phi)
        if bigint.mod_inv(xhi, phi) is not None:
            break
    return DLogStatement(nt, h1, bigint.mod_pow(h1, xhi, nt))


FIELDS = ("t", "z", "e", "s", "s1", "s2", "t1", "t2")
TAMPERS = FIELDS + ("a_enc", "mta", "X", "u")   # X / u: extended proofs only


def with_field(pf, name, value):
    """pf (BobProof or BobProofExt, any structurally equal type) with one inner field replaced."""
    if hasattr(pf, "proof"):
        return type(pf)(with_field(pf.proof, name, value), pf.u)
    return type(pf)(**{**{f: getattr(pf, f) for f in FIELDS}, name: value})


def tamper(kind, pf, a_enc, mta, X):
    """One changed input: a proof field, a_enc or mta off by one; X or u off by G.
    Returns (pf, a_enc, mta, X)."""
    if kind in FIELDS:
        inner = pf.proof if hasattr(pf, "proof") else pf
        return with_field(pf, kind, getattr(inner, kind) + 1), a_enc, mta, X
    if kind == "a_enc":
        return pf, a_enc + 1, mta, X
    if kind == "mta":
        return pf, a_enc, mta + 1, X
    if kind == "X":
        return pf, a_enc, mta, ec.add(X, ec.G)
    if kind == "u":
        return type(pf)(pf.proof, ec.add(pf.u, ec.G)), a_enc, mta, X
    raise ValueError(kind)
