"""GPU checks of the commitment v of Bob's range proof (fsdkr_bob_commit_v,
Context.bob_commit_v): the fused chain (the head over N's bits >= 768, then
bob_v_tail_ct_kernel) and the composed path against Python's pow bit for bit.
The moduli need not be products of two primes for that, so they are built to
meet the tail's edges: a head of 1280 bits, of 256 bits, of one bit and of none, and
low 768 bits that are all ones or all zero but bit 0 (the window look-ahead across
every limb of the shift register).  alpha cycles through values that a tail of 8
limbs, or one that dropped a limb, would get wrong."""
import pytest

from oracle import secp256k1 as ec
from oracle.rng import Rng

pytestmark = pytest.mark.gpu

Q3 = ec.Q ** 3
LO = 768
COUNTS_64 = (1, 7, 8, 9, 33)
COUNTS_96 = (1, 5)
N_ALPHA, N_A, N_BETA, N_GAMMA = 13, 5, 3, 4


def _moduli_64():
    rng = Rng("bob-v-moduli")
    full = [rng.bits(2048) | (1 << 2047) | 1 for _ in range(2)]
    ones = (rng.bits(2048) | (1 << 2047)) | ((1 << LO) - 1)
    sparse = ((rng.bits(2048) | (1 << 2047)) >> LO << LO) | 1
    ns = [full[0], rng.bits(1024) | (1 << 1023) | 1, rng.bits(768) | (1 << 767) | 1, full[1],
          rng.bits(767) | (1 << 766) | 1, ones, sparse, 3]
    assert [n.bit_length() for n in ns] == [2048, 1024, 768, 2048, 767, 2048, 2048, 2]
    assert all(n & 1 for n in ns)
    return ns


def _instances(ns, count, tag):
    """`count` instances with the keys interleaved instance by instance and every
    operand cycling through its edge values: alpha's 13 against the 8 keys (coprime:
    104 instances hold every alpha once per key), the shorter cycles offset against
    each other and against the keys.  Returns (a_enc, alpha, gamma, beta, key) rows."""
    rng = Rng(("bob-v", tag))
    alt = int("0f" * 96, 16)                     # every second nibble zero
    out = []
    for i in range(count):
        m = i % len(ns)
        N = ns[m]
        NN = N * N
        al = [0, 1, 15, 16, 1 << 256, 1 << 767, 0xF << 764, (1 << 768) - 1, Q3 - 1, alt, 0x9E3779B9 << (32 * 8),
              0x80000001 << (32 * 23), rng.bits(768)][i % N_ALPHA]
        a = [0, 1, NN - 1, N, rng.sample_below(NN)][(i + i // N_A) % N_A]
        be = [1, N - 1, rng.sample_below(N)][(i + i // N_BETA) % N_BETA]
        ga = [0, 1, N - 1, rng.sample_below(N)][(i + i // N_GAMMA) % N_GAMMA]
        out.append((a, al, ga, be, m))
    return out


def _want(ns, inst):
    return [pow(a, al, ns[m] ** 2) * (1 + ga * ns[m]) * pow(be, ns[m], ns[m] ** 2) % ns[m] ** 2
            for a, al, ga, be, m in inst]


FULL = 104   # 8 keys x 13 alphas: every alpha once per key (the other cycles are shorter)


@pytest.fixture(scope="module")
def ref64():
    ns = _moduli_64()
    inst = _instances(ns, FULL, "nl64")
    seen = {(m, i % N_ALPHA) for i, (_, _, _, _, m) in enumerate(inst)}
    assert len(seen) == len(ns) * N_ALPHA
    return ns, inst, _want(ns, inst)


@pytest.fixture(scope="module")
def ref96():
    rng = Rng("bob-v-moduli-96")
    ns = [rng.bits(3072) | (1 << 3071) | 1, rng.bits(2048) | (1 << 2047) | 1, rng.bits(3072) | (1 << 3071) | 1]
    inst = _instances(ns, max(COUNTS_96), "nl96")
    return ns, inst, _want(ns, inst)


def _run(ctx, ns, inst, nl, fused):
    A, AL, GA, BE, I = (list(x) for x in zip(*inst))
    return ctx.bob_commit_v(A, AL, GA, BE, ns, I, nl, fused=fused)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("count", COUNTS_64 + (FULL,))
def test_commit_v_2048_matches_pow(gpu_ctx, ref64, count, fused):
    ns, inst, want = ref64
    assert _run(gpu_ctx, ns, inst[:count], 64, fused) == want[:count]


@pytest.mark.parametrize("fused", [True, False])
def test_commit_v_short_keys_alone(gpu_ctx, ref64, fused):
    """Only keys of at most 768 bits in the call: the launch's window is chosen for them
    and no head has more than one bit."""
    ns, inst, want = ref64
    pick = [i for i, row in enumerate(inst) if row[4] in (2, 4, 7)][:20]
    sub = [ns[2], ns[4], ns[7]]
    rows = [inst[i][:4] + ({2: 0, 4: 1, 7: 2}[inst[i][4]],) for i in pick]
    assert _run(gpu_ctx, sub, rows, 64, fused) == [want[i] for i in pick]


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("count", COUNTS_96)
def test_commit_v_3072_matches_pow(gpu_ctx, ref96, count, fused):
    ns, inst, want = ref96
    assert _run(gpu_ctx, ns, inst[:count], 96, fused) == want[:count]


def test_error_returns(gpu_ctx, ref64):
    from fsdkr import _native
    ns, inst, want = ref64
    with pytest.raises(_native.FsdkrError) as e:
        _run(gpu_ctx, ns, inst[:3], 80, True)
    assert e.value.code == _native.FSDKR_E_UNSUPPORTED
    for fused in (True, False):
        for bad in (ns[0] + 1, 1):                       # even N, N <= 1
            with pytest.raises(_native.FsdkrError) as e:
                _run(gpu_ctx, [ns[0], bad], [(1, 1, 0, 1, m) for m in range(2)], 64, fused)
            assert e.value.code == _native.FSDKR_E_ARG
        with pytest.raises(_native.FsdkrError) as e:     # n_idx out of range
            _run(gpu_ctx, ns[:2], [(1, 1, 0, 1, 2)], 64, fused)
        assert e.value.code == _native.FSDKR_E_ARG
        with pytest.raises(_native.FsdkrError) as e:     # a_enc is public: an unreduced one is refused
            _run(gpu_ctx, ns, [(ns[0] * ns[0], 1, 1, 1, 0)], 64, fused)
        assert e.value.code == _native.FSDKR_E_ARG
        assert gpu_ctx.bob_commit_v([], [], [], [], ns, [], 64, fused=fused) == []
    for al, ga in ((1 << 768, 0), (-1, 0), (0, -1), (0, 1 << 2048)):   # refused on the host, before the device
        with pytest.raises(ValueError):
            gpu_ctx.bob_commit_v([1], [al], [ga], [1], ns[:1], [0], 64)
    # the fused chain has the 8-lane shape only; the composed path takes any setting
    try:
        for lanes in (4, 16):
            gpu_ctx.set_modexp_group(lanes)
            with pytest.raises(_native.FsdkrError) as e:
                _run(gpu_ctx, ns, inst[:3], 64, True)
            assert e.value.code == _native.FSDKR_E_ARG
            assert _run(gpu_ctx, ns, inst[:3], 64, False) == want[:3]
        gpu_ctx.set_modexp_group(8)
        assert _run(gpu_ctx, ns, inst[:9], 64, True) == want[:9]
    finally:
        gpu_ctx.set_modexp_group(0)
