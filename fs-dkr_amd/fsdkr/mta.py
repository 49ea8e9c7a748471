"""GG20's MtA exchange (range_proofs.rs) on the MI355X engine: Alice's first
message with its range proof (AliceProof, :26-203), the respondent's proofs
(BobProof, BobProofExt, :205-590), Bob's response and Alice's decryption.

initiate     Alice's first message for every exchange: c_A = Enc(a; r) in one
             device call, then its proofs (generate_alice).
generate_alice  the prover of AliceProof (AliceZkpRound1 / Round2, :40-96,
             :168-202): the commitments z = h1^a h2^ro and w = h1^alpha h2^gamma of
             ALL proofs in one call of the constant-time two-base comb
             (Context.pedersen_commit, fsdkr_pedersen_commit_ct), u = Enc(alpha;
             beta), s = r^e beta.
verify_alice Bob's check of that message: AliceProof::verify (:112-164) of
             `count` proofs in one device pass (fsdkr_alice_verify).

verify_bob   `count` independent proofs in one device pass (fsdkr_bob_verify):
             the four h1 / h2 powers as fixed-base combs, z^e and t^e with one
             simultaneous inversion, a_enc^s1 * s^N * mta^-e mod N^2 as ONE split
             chain of bits(N) squarings, the transcript hash and, for the extended
             proof, G*s1 == X*e + u.  Keys of up to 2048 bits run in the 64-limb
             class, keys of up to 3072 bits in the 96-limb class (one per call).
generate_bob the prover (BobZkpRound1 / Round2, BobProof::generate), batched
             per round over the existing entry points; secret exponents run
             through the regular-access kernel, or with fused=True through the
             constant-time comb (z, z', t, w: one Context.pedersen_commit call)
             and one constant-time chain per v (Context.bob_commit_v).
respond      Bob's side of one exchange ("Bob follows MtA", :688-704): the
             response mta_out = a_enc^b * Enc(beta'; r) on the device
             (fsdkr_mta_respond: one constant-time chain per response in both
             width classes), then its proofs (generate_bob).
finish       Alice's last step: alpha = Dec(mta_out) mod q.

one_call=True (generate_bob, generate_alice, and through them respond, initiate)
             the whole prover as ONE device call (Context.bob_prove / alice_prove,
             fsdkr_bob_prove / fsdkr_alice_prove): the same draws, then the
             commitments, the challenge hash, r^e beta mod N and the integer
             responses all on the device; bit for bit the default path's proofs."""
import math

import numpy as np

from . import _native
from .batch import UnsupportedInput, _limbs_for, pack, pack_points
from .refresh import Q, FsDkrPanic, _ctx
from .types import AliceProof, BobProof, BobProofExt

PANIC = 2          # verdict: the reference panics (X or u at infinity, range_proofs.rs:428-431)
Q3 = Q ** 3
NL = 64            # limbs of N, N~ in the class of 2048-bit keys
NL_CLASSES = (64, 96)   # width classes of a call: keys of up to 2048 / 3072 bits
_u32p = _native.u32p


def _fits(name, values, limbs):
    for v in values:
        if v < 0:
            raise UnsupportedInput(f"{name}: negative value")
        if v.bit_length() > 32 * limbs:
            raise UnsupportedInput(f"{name}: wider than {32 * limbs} bits")


def width_class(eks, statements):
    """Limbs of N, N~ for a call: the smallest class that fits every N and N~ (the
    keys alone decide; a proof field wider than its place in that class is not
    representable, see verify_bob)."""
    bits = max([1] + [v.bit_length() for ek, st in zip(eks, statements) for v in (ek.n, st.N)])
    for nl in NL_CLASSES:
        if bits <= 32 * nl:
            return nl
    raise UnsupportedInput(f"N / Ntilde: wider than {32 * NL_CLASSES[-1]} bits")


def key_table(eks, statements):
    """Dedup the (ek, statement) pairs: (keys, key_idx) with keys a list of
    (N, N~, h1, h2) and key_idx[p] the row of proof p."""
    rows, keys, idx = {}, [], []
    for ek, st in zip(eks, statements):
        k = (ek.n, st.N, st.g, st.ni)
        if k not in rows:
            rows[k] = len(keys)
            keys.append(k)
        idx.append(rows[k])
    return keys, idx


def prepass(proofs, a_encs, mta_outs, eks, statements, X=None):
    """The host pre-pass of verify_bob: validation, key dedup and the values the
    device reads.  Returns a dict of ints / lists (packed by verify_bob):
    keys, key_idx, nl (the call's width class, width_class), the proof fields with
    s1 and e clamped to their packed widths, and t1_red = t1 mod N (what the device
    multiplies into 1 + t1*N mod N^2)."""
    count = len(proofs)
    if not (len(a_encs) == len(mta_outs) == len(eks) == len(statements) == count):
        raise ValueError("verify_bob: argument lists differ in length")
    ext = X is not None
    if ext and len(X) != count:
        raise ValueError("verify_bob: X differs in length")
    inner = [p.proof for p in proofs] if ext else list(proofs)
    for ek, st in zip(eks, statements):
        for name, v in (("N", ek.n), ("Ntilde", st.N)):
            if v <= 0 or v % 2 == 0:
                raise UnsupportedInput(f"{name}: even, zero or negative modulus (the verifier's own key)")
    keys, key_idx = key_table(eks, statements)
    nl = width_class(eks, statements)
    for name, col, limbs in (("N", 0, nl), ("Ntilde", 1, nl), ("h1", 2, nl), ("h2", 3, nl)):
        _fits(name, [k[col] for k in keys], limbs)
    _fits("a_enc", a_encs, 2 * nl)
    _fits("mta_out", mta_outs, 2 * nl)
    for f in ("z", "t", "s"):
        _fits(f, [getattr(p, f) for p in inner], nl)
    for f in ("e", "s1", "s2", "t1", "t2"):
        if any(getattr(p, f) < 0 for p in inner):
            raise UnsupportedInput(f"{f}: negative value")
    # s1 > q^3 is rejected whatever its size, a challenge of 2^256 or more never
    # equals the hash: both are packed as the smallest value with that outcome
    s1 = [min(p.s1, Q3 + 1) for p in inner]
    e = [min(p.e, 1 << 256) for p in inner]
    t1_red = [p.t1 % ek.n for p, ek in zip(inner, eks)]
    return {"count": count, "ext": ext, "keys": keys, "key_idx": key_idx, "nl": nl, "inner": inner, "s1": s1, "e": e,
            "t1_red": t1_red, "s1_over": [p.s1 > Q3 for p in inner]}


def _batch(pp, a_encs, mta_outs, proofs, X):
    inner, count, nl = pp["inner"], pp["count"], pp["nl"]
    keep = []

    def arr(values, limbs):
        a = pack(list(values), limbs)
        keep.append(a)
        return a.ctypes.data_as(_u32p)

    def width(values):
        return _limbs_for(max(1, max(v.bit_length() for v in values)))

    b = _native.BobBatchC()
    b.count, b.n_keys, b.nl = count, len(pp["keys"]), nl
    s2, t1, t2 = [p.s2 for p in inner], [p.t1 for p in inner], [p.t2 for p in inner]
    b.el, b.s1l, b.s2l, b.t1l, b.t2l = width(pp["e"]), width(pp["s1"]), width(s2), width(t1), width(t2)
    for col, name in enumerate(("N", "Ntilde", "h1", "h2")):
        setattr(b, name, arr([k[col] for k in pp["keys"]], nl))
    ki = np.ascontiguousarray(np.asarray(pp["key_idx"], dtype=np.uint32))
    keep.append(ki)
    b.key_idx = ki.ctypes.data_as(_u32p)
    b.a_enc, b.mta = arr(a_encs, 2 * nl), arr(mta_outs, 2 * nl)
    b.z, b.t, b.s = (arr([getattr(p, f) for p in inner], nl) for f in ("z", "t", "s"))
    b.e, b.s1 = arr(pp["e"], b.el), arr(pp["s1"], b.s1l)
    b.s2, b.t1, b.t2 = arr(s2, b.s2l), arr(t1, b.t1l), arr(t2, b.t2l)
    if pp["ext"]:
        px, pu = pack_points(list(X)), pack_points([p.u for p in proofs])
        keep += [px, pu]
        b.X, b.u = px.ctypes.data_as(_u32p), pu.ctypes.data_as(_u32p)
    return b, keep


def verify_bob(proofs, a_encs, mta_outs, eks, statements, X=None, ctx=None, fused=True):
    """BobProof::verify (range_proofs.rs:360-446) of every proof, or with X (one
    point per proof, None = infinity) BobProofExt::verify (:527-562) of
    BobProofExt objects.  eks / statements: the verifier's Paillier key and
    (N~, h1, h2) per proof; equal pairs share one row of the device's key table.

    Returns np.uint8[count]: 1 accepted, 0 rejected, PANIC (2) where the
    reference panics (X or u at infinity, after the checks before the hash pass).

    Raises batch.UnsupportedInput for what the C ABI does not represent: a
    negative field; an even, zero or negative N or N~ (the verifier's own keys);
    a key above 3072 bits; a hashed value wider than its field in the call's width
    class (the smallest of 2048 and 3072 bits that fits every N and N~: h1, h2, z,
    t, s above that width, a_enc, mta_out above twice it).  The reference's own
    outcome for these (a panic in mod_pow for a negative exponent, a plain
    rejection otherwise) is not reproduced per instance.  Narrower keys in a call
    of the 3072-bit class are zero-extended; the hash covers the values as given.

    fused=False runs the mod-N^2 part as three separate chains (A/B timing)."""
    pp = prepass(proofs, a_encs, mta_outs, eks, statements, X)
    if pp["count"] == 0:
        return np.zeros(0, dtype=np.uint8)
    b, keep = _batch(pp, a_encs, mta_outs, proofs, X)
    out = _ctx(ctx).bob_verify(b, pp["count"], fused=fused)
    del keep
    return out


def prepass_alice(proofs, ciphers, eks, statements):
    """The host pre-pass of verify_alice: prepass without Bob's fields.  Returns
    keys, key_idx, nl (the call's width class) and the proof fields with s1 clamped
    to q^3 + 1 and e to 2^256 (the smallest values with their outcome)."""
    count = len(proofs)
    if not (len(ciphers) == len(eks) == len(statements) == count):
        raise ValueError("verify_alice: argument lists differ in length")
    for ek, st in zip(eks, statements):
        for name, v in (("N", ek.n), ("Ntilde", st.N)):
            if v <= 0 or v % 2 == 0:
                raise UnsupportedInput(f"{name}: even, zero or negative modulus (the verifier's own key)")
    keys, key_idx = key_table(eks, statements)
    nl = width_class(eks, statements)
    for name, col, limbs in (("N", 0, nl), ("Ntilde", 1, nl), ("h1", 2, nl), ("h2", 3, nl)):
        _fits(name, [k[col] for k in keys], limbs)
    _fits("cipher", ciphers, 2 * nl)
    for f in ("z", "s"):
        _fits(f, [getattr(p, f) for p in proofs], nl)
    for f in ("e", "s1", "s2"):
        if any(getattr(p, f) < 0 for p in proofs):
            raise UnsupportedInput(f"{f}: negative value")
    return {"count": count, "keys": keys, "key_idx": key_idx, "nl": nl, "s1": [min(p.s1, Q3 + 1) for p in proofs],
            "e": [min(p.e, 1 << 256) for p in proofs], "s2": [p.s2 for p in proofs]}


def _alice_batch(pp, ciphers, proofs):
    count, nl = pp["count"], pp["nl"]
    keep = []

    def arr(values, limbs):
        a = pack(list(values), limbs)
        keep.append(a)
        return a.ctypes.data_as(_u32p)

    def width(values):
        return _limbs_for(max(1, max(v.bit_length() for v in values)))

    b = _native.AliceBatchC()
    b.count, b.n_keys, b.nl = count, len(pp["keys"]), nl
    b.el, b.s1l, b.s2l = width(pp["e"]), width(pp["s1"]), width(pp["s2"])
    for col, name in enumerate(("N", "Ntilde", "h1", "h2")):
        setattr(b, name, arr([k[col] for k in pp["keys"]], nl))
    ki = np.ascontiguousarray(np.asarray(pp["key_idx"], dtype=np.uint32))
    keep.append(ki)
    b.key_idx = ki.ctypes.data_as(_u32p)
    b.cipher = arr(ciphers, 2 * nl)
    b.z, b.s = (arr([getattr(p, f) for p in proofs], nl) for f in ("z", "s"))
    b.e, b.s1, b.s2 = arr(pp["e"], b.el), arr(pp["s1"], b.s1l), arr(pp["s2"], b.s2l)
    return b, keep


def verify_alice(proofs, ciphers, eks, statements, ctx=None):
    """AliceProof::verify (range_proofs.rs:112-164) of every proof: Bob's check of
    Alice's first MtA message ciphers[k] under her key eks[k], against his own
    (N~, h1, h2) statements[k]; equal pairs share one row of the device's key table.

    Returns np.uint8[count]: 1 accepted, 0 rejected (this path never panics).

    Raises batch.UnsupportedInput as verify_bob does: a negative field; an even,
    zero or negative N or N~; a key above 3072 bits; a hashed value wider than its
    field in the call's width class (h1, h2, z, s above that width, cipher above
    twice it)."""
    proofs, ciphers, eks, statements = list(proofs), list(ciphers), list(eks), list(statements)
    pp = prepass_alice(proofs, ciphers, eks, statements)
    if pp["count"] == 0:
        return np.zeros(0, dtype=np.uint8)
    b, keep = _alice_batch(pp, ciphers, proofs)
    out = _ctx(ctx).alice_verify(b, pp["count"])
    del keep
    return out


def _from_modulo(rng, n):
    """SampleFromMultiplicativeGroup::from_modulo (range_proofs.rs:599-607)."""
    while True:
        r = rng.sample_below(n)
        if math.gcd(r, n) == 1:
            return r


ALICE_XL = 24   # limbs of the comb's x rows: a < q and alpha < q^3 both run as 768-bit values


def commit_yl(nl):
    """Limbs of the comb's y rows in the width class nl: the public bound q^3 N~ of
    gamma (ro < q N~ runs at the same width)."""
    return ALICE_XL + nl


def _prove_keys(eks, sts):
    """The key table of a whole-prover call: ([(N, N~, h1 mod N~, h2 mod N~)], key_idx)."""
    keys, row, idx = [], {}, []
    for ek, st in zip(eks, sts):
        k = (ek.n, st.N, st.g % st.N, st.ni % st.N)
        if k not in row:
            row[k] = len(keys)
            keys.append(k)
        idx.append(row[k])
    return keys, idx


def generate_alice(items, rng, ctx=None, one_call=False):
    """AliceProof::generate (range_proofs.rs:168-202) for every item (a, cipher, ek,
    statement, r): Alice's secret a in [0, 2^768), her ciphertext cipher = Enc(a; r)
    under her key ek, the verifier's (N~, h1, h2) and the randomness r.

    Per proof the draws go through `rng` (sample_below) in the reference's order
    (:54-57): alpha, beta (from_modulo), gamma, ro.  The commitments z = h1^a h2^ro and
    w = h1^alpha h2^gamma mod N~ of all proofs are ONE Context.pedersen_commit call (two
    instances per proof, x rows of 24 limbs, y rows of commit_yl limbs: public bounds,
    so the kernel's geometry tells nothing about the values); u = Enc(alpha; beta) runs
    through Context.paillier_encrypt and s = r^e beta mod N through modexp_batch (e is
    public).  Returns types.AliceProofs.

    one_call=True: the same draws in the same order and bit for bit the same proofs
    from exactly ONE Context.alice_prove call (fsdkr_alice_prove: the comb, u, the
    challenge hash, r^e beta and the responses e a + alpha, e ro + gamma on the device;
    nothing secret is combined in host integers)."""
    ctx = _ctx(ctx)
    items = list(items)
    n = len(items)
    if n == 0:
        return []
    for a, _, _, _, _ in items:
        if a < 0 or a >> (32 * ALICE_XL):
            raise ValueError("generate_alice: a must satisfy 0 <= a < 2^768")
    eks, sts = [it[2] for it in items], [it[3] for it in items]
    nl = width_class(eks, sts)
    rnd = []
    for a, cipher, ek, st, r in items:
        alpha = rng.sample_below(Q3)
        beta = _from_modulo(rng, ek.n)
        gamma = rng.sample_below(Q3 * st.N)
        ro = rng.sample_below(Q * st.N)
        rnd.append((alpha, beta, gamma, ro))
    if one_call:
        keys, idx = _prove_keys(eks, sts)
        o = ctx.alice_prove(keys, idx, nl, [it[1] for it in items], a=[it[0] for it in items],
                            r=[it[4] % ek.n for it, ek in zip(items, eks)], alpha=[x[0] for x in rnd],
                            beta=[x[1] for x in rnd], gamma=[x[2] for x in rnd], ro=[x[3] for x in rnd])
        return [AliceProof(o["z"][k], o["e"][k], o["s"][k], o["s1"][k], o["s2"][k]) for k in range(n)]
    keys, row = [], {}
    for st in sts:
        k = (st.N, st.g % st.N, st.ni % st.N)
        if k not in row:
            row[k] = len(keys)
            keys.append(k)
    xs, ys, idx = [], [], []
    for (a, cipher, ek, st, r), (alpha, beta, gamma, ro) in zip(items, rnd):
        k = row[(st.N, st.g % st.N, st.ni % st.N)]
        xs += [a, alpha]
        ys += [ro, gamma]
        idx += [k, k]
    zw = ctx.pedersen_commit(xs, ys, keys, idx, nl, xl=ALICE_XL, yl=commit_yl(nl))
    ns, n_row = [], {}
    for ek in eks:
        if ek.n not in n_row:
            n_row[ek.n] = len(ns)
            ns.append(ek.n)
    n_idx = [n_row[ek.n] for ek in eks]
    us = ctx.paillier_encrypt([x[0] for x in rnd], [x[1] for x in rnd], ns, n_idx, nl)
    from .distribute import chain_bigint
    es = [chain_bigint(ek.n, ek.n + 1, it[1], zw[2 * k], us[k], zw[2 * k + 1]) for k, (it, ek) in enumerate(zip(items, eks))]
    re = ctx.modexp_batch([it[4] % ek.n for it, ek in zip(items, eks)], es, ns, n_idx, nl)   # public e
    out = []
    for k, ((a, cipher, ek, st, r), (alpha, beta, gamma, ro)) in enumerate(zip(items, rnd)):
        e = es[k]
        out.append(AliceProof(zw[2 * k], e, re[k] * beta % ek.n, e * a + alpha, e * ro + gamma))
    return out


def initiate(as_, eks, statements, rng, ctx=None, one_call=False):
    """Alice starts MtA (range_proofs.rs:650-670) for every exchange k: her secret
    as_[k] (0 <= a < q), her own Paillier key eks[k] and Bob's (N~, h1, h2)
    statements[k].

    First, for every exchange in order, r_k = from_modulo(N_k) through `rng` (:656);
    then ONE Context.paillier_encrypt call makes every c_A = Enc(a; r), at the width
    class of the call's keys (width_class); then ONE generate_alice call over the same
    rng proves them.  Returns (a_encs, rs, proofs).  one_call is generate_alice's."""
    ctx = _ctx(ctx)
    as_, eks, statements = list(as_), list(eks), list(statements)
    n = len(as_)
    if not (len(eks) == len(statements) == n):
        raise ValueError("initiate: argument lists differ in length")
    for a in as_:
        if a < 0 or a >= Q:
            raise ValueError("initiate: a must satisfy 0 <= a < q")
    if n == 0:
        return [], [], []
    nl = width_class(eks, statements)
    rs = [_from_modulo(rng, ek.n) for ek in eks]
    ns, n_row = [], {}
    for ek in eks:
        if ek.n not in n_row:
            n_row[ek.n] = len(ns)
            ns.append(ek.n)
    a_encs = ctx.paillier_encrypt(as_, rs, ns, [n_row[ek.n] for ek in eks], nl)
    proofs = generate_alice(list(zip(as_, a_encs, eks, statements, rs)), rng, ctx=ctx, one_call=one_call)
    return a_encs, rs, proofs


def _challenge(ek, a_enc, mta, z, z_prim, t, v, w, check):
    from .distribute import chain_bigint
    vals = [ek.n, ek.n + 1, a_enc, mta, z, z_prim, t, v, w]
    if check is not None:
        for pt in check:
            if pt is None:
                raise FsDkrPanic("x_coord().unwrap() on the point at infinity (range_proofs.rs:486-489)")
            vals += [pt[0], pt[1]]
    return chain_bigint(*vals)


BOB_XL_OVER = 16   # limbs of the comb's x rows above nl: gamma < q^2 N (b, alpha, beta' are narrower)


def _bob_round1_fused(ctx, items, rnd, nl):
    """z, z', t, w of every proof from ONE pedersen_commit call of four instances per
    proof (xs = b, alpha, beta', gamma; ys = ro, ro', sigma, tau) at the public widths
    xl = 16 + nl (gamma < q^2 N) and yl = commit_yl(nl) (tau, ro' < q^3 N~), and every
    v from ONE bob_commit_v call over a_enc mod N^2, alpha, gamma mod N and beta.
    Returns ([(z, z', t, w)], [v])."""
    keys, row = [], {}
    xs, ys, idx = [], [], []
    for (a_enc, mta, b, beta_prim, ek, st, r), (alpha, beta, gamma, ro, ro_prim, sigma, tau) in zip(items, rnd):
        k = (st.N, st.g % st.N, st.ni % st.N)
        if k not in row:
            row[k] = len(keys)
            keys.append(k)
        xs += [b, alpha, beta_prim, gamma]
        ys += [ro, ro_prim, sigma, tau]
        idx += [row[k]] * 4
    cm = ctx.pedersen_commit(xs, ys, keys, idx, nl, xl=BOB_XL_OVER + nl, yl=commit_yl(nl))
    ns, n_row = [], {}
    for it in items:
        if it[4].n not in n_row:
            n_row[it[4].n] = len(ns)
            ns.append(it[4].n)
    vs = ctx.bob_commit_v([it[0] % it[4].nn for it in items], [x[0] for x in rnd],
                          [x[2] % it[4].n for it, x in zip(items, rnd)], [x[1] for x in rnd], ns,
                          [n_row[it[4].n] for it in items], nl)
    return [tuple(cm[4 * k:4 * k + 4]) for k in range(len(items))], vs


def generate_bob(items, rng, ctx=None, check=False, fused=False, one_call=False):
    """BobProof::generate (range_proofs.rs:448-515) / BobProofExt::generate
    (:564-589) for every item (a_enc, mta_out, b, beta_prim, ek, statement, r):
    Alice's ciphertext, the MtA output, Bob's secret scalar b in [0, q), the
    beta' and randomness r of Enc(beta'; r), and the verifier's keys.

    Per proof the draws go through `rng` (sample_below) in the reference's order:
    alpha, beta (from_modulo), gamma, ro, ro_prim, sigma, tau (:266-272).  The
    exponentiations of all proofs are batched per round; every one with a secret
    exponent runs through the regular-access kernel, at the width class of the
    call's keys (width_class).  Returns BobProofs, or BobProofExts with check=True.

    fused=True: the same draws and bit for bit the same proofs, with the four
    commitments z, z', t, w of all proofs from ONE Context.pedersen_commit call (the
    constant-time two-base comb, 4 n instances at public widths) and every v from ONE
    Context.bob_commit_v call (fsdkr_bob_commit_v: one constant-time chain per v in
    both width classes); no regular-access modexp is issued.  It needs 0 <= b <
    2^256 and 0 <= beta' < N (ValueError before any device call otherwise).

    one_call=True: the same draws in the same order and bit for bit the same proofs
    from exactly ONE Context.bob_prove call (fsdkr_bob_prove: the comb and the v chain
    of fused=True, then the challenge hash, r^e beta mod N and the four responses
    e x + y on the device; nothing secret is combined in host integers).  It needs what
    fused=True needs and 0 <= a_enc < N^2, and has no BobProofExt yet: check=True is a
    ValueError, as the others before any device call."""
    ctx = _ctx(ctx)
    items = list(items)
    n = len(items)
    if n == 0:
        return []
    if one_call:
        if check:
            raise ValueError("generate_bob: one_call has no BobProofExt (check=True)")
        for a_enc, mta, b, beta_prim, ek, st, r in items:
            if a_enc < 0 or a_enc >= ek.nn:
                raise ValueError("generate_bob: one_call needs 0 <= a_enc < N^2")
    if fused or one_call:
        for a_enc, mta, b, beta_prim, ek, st, r in items:
            if b < 0 or b >> 256:
                raise ValueError("generate_bob: b must satisfy 0 <= b < 2^256")
            if beta_prim < 0 or beta_prim >= ek.n:
                raise ValueError("generate_bob: beta' must satisfy 0 <= beta' < N")
    nl = width_class([it[4] for it in items], [it[5] for it in items])
    rnd = []
    for a_enc, mta, b, beta_prim, ek, st, r in items:
        alpha = rng.sample_below(Q3)
        beta = _from_modulo(rng, ek.n)
        gamma = rng.sample_below(Q * Q * ek.n)
        ro = rng.sample_below(Q * st.N)
        ro_prim = rng.sample_below(Q3 * st.N)
        sigma = rng.sample_below(Q * st.N)
        tau = rng.sample_below(Q3 * st.N)
        rnd.append((alpha, beta, gamma, ro, ro_prim, sigma, tau))
    if one_call:
        eks = [it[4] for it in items]
        keys, idx = _prove_keys(eks, [it[5] for it in items])
        o = ctx.bob_prove(keys, idx, nl, [it[0] for it in items], [it[1] for it in items], b=[it[2] for it in items],
                          beta_prim=[it[3] for it in items], r=[it[6] % it[4].n for it in items],
                          alpha=[x[0] for x in rnd], beta=[x[1] for x in rnd], gamma=[x[2] for x in rnd],
                          gamma_mod_n=[x[2] % ek.n for x, ek in zip(rnd, eks)], ro=[x[3] for x in rnd],
                          ro_prim=[x[4] for x in rnd], sigma=[x[5] for x in rnd], tau=[x[6] for x in rnd])
        return [BobProof(o["t"][k], o["z"][k], o["e"][k], o["s"][k], o["s1"][k], o["s2"][k], o["t1"][k], o["t2"][k])
                for k in range(n)]
    # round 1: h1^(b, alpha, beta', gamma), h2^(ro, ro', sigma, tau) mod N~; a_enc^alpha, beta^N mod N^2
    if fused:
        commits, vs = _bob_round1_fused(ctx, items, rnd, nl)
    else:
        commits, vs = _bob_round1_composed(ctx, items, rnd, nl)
    pts = None
    if check:   # X = G*b, u = G*alpha (:480-484): secret scalars, the constant-time comb
        pts = ctx.ec_mul_g([it[2] % Q for it in items] + [x[0] % Q for x in rnd])
    es, firsts = [], []
    for k, ((a_enc, mta, b, beta_prim, ek, st, r), x) in enumerate(zip(items, rnd)):
        z, z_prim, t, w = commits[k]
        chk = (pts[k], pts[n + k]) if check else None
        es.append(_challenge(ek, a_enc, mta, z, z_prim, t, vs[k], w, chk))
        firsts.append((t, z))
    # round 2: r^e mod N (:328)
    ns, n_row = [], {}
    for it in items:
        if it[4].n not in n_row:
            n_row[it[4].n] = len(ns)
            ns.append(it[4].n)
    re = ctx.modexp_batch([it[6] % it[4].n for it in items], es, ns, [n_row[it[4].n] for it in items], nl)   # public e
    out = []
    for k, ((a_enc, mta, b, beta_prim, ek, st, r), x) in enumerate(zip(items, rnd)):
        alpha, beta, gamma, ro, ro_prim, sigma, tau = x
        e = es[k]
        t, z = firsts[k]
        pf = BobProof(t, z, e, re[k] * beta % ek.n, e * b + alpha, e * ro + ro_prim, e * beta_prim + gamma,
                      e * sigma + tau)
        out.append(BobProofExt(pf, pts[n + k]) if check else pf)
    return out


def _bob_round1_composed(ctx, items, rnd, nl):
    """z, z', t, w and v of every proof through the regular-access modexp: eight
    powers mod N~ and a_enc^alpha mod N^2 per proof, beta^N with its public exponent,
    the products on the host.  Returns ([(z, z', t, w)], [v])."""
    nts, nt_row = [], {}
    nns, nn_row = [], {}
    for _, _, _, _, ek, st, _ in items:
        if st.N not in nt_row:
            nt_row[st.N] = len(nts)
            nts.append(st.N)
        if ek.nn not in nn_row:
            nn_row[ek.nn] = len(nns)
            nns.append(ek.nn)
    bases, exps, idx = [], [], []
    for (a_enc, mta, b, beta_prim, ek, st, r), (alpha, beta, gamma, ro, ro_prim, sigma, tau) in zip(items, rnd):
        for base, ex in ((st.g, b), (st.ni, ro), (st.g, alpha), (st.ni, ro_prim), (st.g, beta_prim), (st.ni, sigma),
                         (st.g, gamma), (st.ni, tau)):
            bases.append(base % st.N)
            exps.append(ex)
            idx.append(nt_row[st.N])
    pw = ctx.modexp_batch(bases, exps, nts, idx, nl, secret=True)
    va = ctx.modexp_batch([it[0] % it[4].nn for it in items], [x[0] for x in rnd], nns,
                          [nn_row[it[4].nn] for it in items], 2 * nl, secret=True)
    bn = ctx.modexp_batch([x[1] for x in rnd], [it[4].n for it in items], nns, [nn_row[it[4].nn] for it in items],
                          2 * nl)   # beta^N: public exponent
    commits, vs = [], []
    for k, ((a_enc, mta, b, beta_prim, ek, st, r), x) in enumerate(zip(items, rnd)):
        p = pw[8 * k:8 * k + 8]
        commits.append((p[0] * p[1] % st.N, p[2] * p[3] % st.N, p[4] * p[5] % st.N, p[6] * p[7] % st.N))
        vs.append(va[k] * (x[2] * ek.n + 1) * bn[k] % ek.nn)
    return commits, vs


def respond(a_encs, bs, eks, statements, rng, ctx=None, check=False, fused_proofs=False, one_call=False):
    """Bob follows MtA (range_proofs.rs:688-715) for every exchange k: Alice's
    ciphertext a_encs[k] under her key eks[k], Bob's secret scalar bs[k] (0 <= b <
    2^256) and Alice's (N~, h1, h2) statements[k].

    Per exchange the draws go through `rng` in the reference test's order (:696-697):
    beta' = sample_below(N), then r = sample_below(N); then ONE device call computes
    every mta_out = a_enc^b (1 + beta' N) r^N mod N^2 (Context.mta_respond, at the
    width class of the call's keys, width_class; a_enc is reduced mod N^2), and
    ONE generate_bob call over the same rng proves them.

    Returns (mta_outs, betas, proofs): the responses, Bob's additive shares
    beta = -beta' mod q, and BobProofs (check=True: BobProofExts, whose verifier
    takes X = G*b).  fused_proofs is generate_bob's `fused`, one_call its `one_call`
    (the response itself stays its own Context.mta_respond call)."""
    ctx = _ctx(ctx)
    a_encs, bs, eks, statements = list(a_encs), list(bs), list(eks), list(statements)
    n = len(a_encs)
    if not (len(bs) == len(eks) == len(statements) == n):
        raise ValueError("respond: argument lists differ in length")
    for b in bs:
        if b < 0 or b >> 256:
            raise ValueError("respond: b must satisfy 0 <= b < 2^256")
    if n == 0:
        return [], [], []
    nl = width_class(eks, statements)
    draws = []
    for ek in eks:
        beta_prim = rng.sample_below(ek.n)
        draws.append((beta_prim, rng.sample_below(ek.n)))
    ns, n_row = [], {}
    for ek in eks:
        if ek.n not in n_row:
            n_row[ek.n] = len(ns)
            ns.append(ek.n)
    a_red = [a % ek.nn for a, ek in zip(a_encs, eks)]
    mta_outs = ctx.mta_respond(a_red, bs, [d[0] for d in draws], [d[1] for d in draws], ns,
                               [n_row[ek.n] for ek in eks], nl)
    items = [(a, m, b, d[0], ek, st, d[1]) for a, m, b, d, ek, st in zip(a_encs, mta_outs, bs, draws, eks, statements)]
    proofs = generate_bob(items, rng, ctx=ctx, check=check, fused=fused_proofs, one_call=one_call)
    return mta_outs, [(-d[0]) % Q for d in draws], proofs


def finish(mta_outs, dks, ctx=None):
    """Alice's last step of MtA: alpha_k = Dec(mta_outs[k]) mod q under her
    DecryptionKey dks[k] (Context.paillier_decrypt for one key, paillier_decrypt_many
    otherwise), so that alpha + beta = a b mod q with respond's beta."""
    ctx = _ctx(ctx)
    mta_outs, dks = list(mta_outs), list(dks)
    if len(mta_outs) != len(dks):
        raise ValueError("finish: argument lists differ in length")
    if not mta_outs:
        return []
    keys, row = [], {}
    for dk in dks:
        if (dk.p, dk.q) not in row:
            row[(dk.p, dk.q)] = len(keys)
            keys.append((dk.p, dk.q))
    bits = max(max(p.bit_length(), q.bit_length()) for p, q in keys) * 2
    nl = next((c for c in NL_CLASSES if bits <= 32 * c), None)
    if nl is None:
        raise UnsupportedInput(f"finish: key wider than {32 * NL_CLASSES[-1]} bits")
    if len(keys) == 1:
        ms = ctx.paillier_decrypt(mta_outs, keys[0][0], keys[0][1], nl)
    else:
        ms = ctx.paillier_decrypt_many(mta_outs, [row[(dk.p, dk.q)] for dk in dks], [k[0] for k in keys],
                                       [k[1] for k in keys], nl)
    return [m % Q for m in ms]
