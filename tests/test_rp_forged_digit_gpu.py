"""Ring-Pedersen proofs that are wrong in chosen digits only, through the public entry
Context.ring_pedersen_verify (fsdkr_ring_pedersen_verify): the proof-level face of
tests/test_eq_check_gpu.py.

The final check of index k compares the Montgomery residues x = T^Z_k R^-1 and
y = A_k S^e_k R^-1 (mod N, R = 2^(29 KD)) digit by digit over the lanes of
eq_check_kernel.  A prover who guesses the challenge bit e_k = beta can pick A_k so
that y equals x in the low digits and differs above a chosen bit: Z_k = a_k + beta
lambda, A_k = y R S^-beta.  The guess is right every other try (a_k is redrawn until
the challenge agrees).  oracle.ring_pedersen.verify rejects such a proof, and a
kernel that leaves the lanes above the cut out of its comparison accepts it.  No
primes are needed: the verifier never uses phi(N).

The same entry is also run at the edge of the kernel's precondition (each product
below R N): a small odd N in the wide slot with S, T and A near the end of the slot."""
import pytest

from oracle import bigint, ring_pedersen
from oracle.paillier import EncryptionKey
from oracle.ring_pedersen import RingPedersenProof, RingPedersenStatement
from oracle.rng import Rng
from test_eq_check_gpu import coprime, digits, geom

pytestmark = pytest.mark.gpu

M = 16   # the smallest M of tests/test_hash_lengths.py's ring-Pedersen sets


def cuts(nl):
    """Bit above which the forged side differs: past lanes 0-1, and the top lane alone."""
    KD, G, L, _ = geom(nl)
    return {"above-lanes01": 29 * 2 * L, "top-lane": 29 * (G - 1) * L}


def statement(nl):
    rng = Rng(("rp-forged", nl))
    N = rng.bits(32 * nl) | (1 << (32 * nl - 1)) | 1
    T = rng.sample_below(N)
    while not coprime(T, N):
        T = rng.sample_below(N)
    lam = rng.sample_below(N)
    return RingPedersenStatement(bigint.mod_pow(T, lam, N), T, N, 0, EncryptionKey.from_n(N)), lam


def honest(st, lam, rng):
    a = [rng.sample_below(st.N) for _ in range(M)]
    A = [bigint.mod_pow(st.T, ai, st.N) for ai in a]
    bits = ring_pedersen.challenge_bits(A, M)
    return RingPedersenProof(tuple(A), tuple(ai + e * lam for ai, e in zip(a, bits)))


def forged(st, lam, rng, nl, cut, k, beta):
    """A proof whose check k compares residues equal below bit `cut` and different above."""
    KD, G, L, R = geom(nl)
    N = st.N
    a = [rng.sample_below(N) for _ in range(M)]
    A = [bigint.mod_pow(st.T, ai, N) for ai in a]
    s_inv = pow(st.S, -1, N)
    for tries in range(1, 65):
        a[k] = rng.sample_below(N)
        zk = a[k] + beta * lam
        x = bigint.mod_pow(st.T, zk, N) * pow(R, -1, N) % N
        y = x % (1 << cut)
        if y == x:
            continue
        A[k] = y * R * (s_inv if beta else 1) % N
        bits = ring_pedersen.challenge_bits(A, M)
        if bits[k] == beta:
            break
    else:
        raise AssertionError("no challenge agreed with the guess in 64 tries")
    # what the device compares at index k: equal digits below the cut, different ones above
    lhs = bigint.mod_pow(st.T, zk, N) * pow(R, -1, N) % N
    rhs = A[k] * (st.S if beta else 1) * pow(R, -1, N) % N
    dl, dr = digits(lhs, KD), digits(rhs, KD)
    assert (lhs, rhs) == (x, y) and dl[:cut // 29] == dr[:cut // 29] and dl[cut // 29:] != dr[cut // 29:]
    Z = [ai + e * lam for ai, e in zip(a, bits)]
    return RingPedersenProof(tuple(A), tuple(Z)), tries


@pytest.mark.parametrize("nl", [64, 96])
def test_wide_values_over_a_small_modulus(gpu_ctx, nl):
    """A small odd N in the wide slot with S, T and every A_i near the end of the slot
    (valid residues plus a multiple of N): the kernel reduces each side by one
    conditional subtraction, so the entry has to hand it S reduced; A stays as sent.
    N = 3 and a half-width N; the honest proof and its A_0 + 1 tamper for each."""
    rng = Rng(("rp-wide-small", nl))
    top = (1 << (32 * nl)) - 1
    sts, pfs = [], []
    for N in (3, rng.bits(16 * nl) | (1 << (16 * nl - 1)) | 1):
        def lift(v):
            return v + (top - v) // N * N
        t = 2 if N == 3 else rng.sample_below(N)
        while not coprime(t, N):
            t = rng.sample_below(N)
        lam = rng.bits(200)
        st = RingPedersenStatement(lift(pow(t, lam, N)), lift(t), N, 0, EncryptionKey.from_n(N))
        assert st.S > top - N and st.T > top - N
        a = [rng.bits(200) for _ in range(M)]
        A = [lift(pow(t, ai, N)) for ai in a]
        bits = ring_pedersen.challenge_bits(A, M)
        good = RingPedersenProof(tuple(A), tuple(ai + e * lam for ai, e in zip(a, bits)))
        A2 = [A[0] - N + 1] + A[1:]
        bits2 = ring_pedersen.challenge_bits(A2, M)
        bad = RingPedersenProof(tuple(A2), tuple(ai + e * lam for ai, e in zip(a, bits2)))
        sts += [st, st]
        pfs += [good, bad]
    want = [int(ring_pedersen.verify(p, s, M)) for p, s in zip(pfs, sts)]
    assert want == [1, 0, 1, 0]
    got = gpu_ctx.ring_pedersen_verify(sts, pfs, M, nl).tolist()
    print(f"nl={nl}: device {got}, oracle {want}")
    assert got == want


@pytest.mark.parametrize("where", ["above-lanes01", "top-lane"])
@pytest.mark.parametrize("nl", [64, 96])
def test_forged_digits_rejected(gpu_ctx, nl, where):
    """One forged proof per guessed bit and the honest proof beside them in one call.
    nl = 64 is the 8-lane shape of the kernel, nl = 96 the 4-lane one."""
    st, lam = statement(nl)
    rng = Rng(("rp-forged-proofs", nl, where))
    cut = cuts(nl)[where]
    f0, t0 = forged(st, lam, rng, nl, cut, 5, 0)
    f1, t1 = forged(st, lam, rng, nl, cut, 11, 1)
    good = honest(st, lam, rng)
    want = [int(ring_pedersen.verify(p, st, M)) for p in (f0, good, f1)]
    assert want == [0, 1, 0]
    got = gpu_ctx.ring_pedersen_verify([st] * 3, [f0, good, f1], M, nl).tolist()
    print(f"nl={nl} {where}: cut at bit {cut}, tries {t0} and {t1}, device {got}, oracle {want}")
    assert got == want
