"""GPU checks of the constant-time two-base comb (fsdkr_pedersen_commit_ct) at the
width pairs Bob's prover is the first to use: x rows of 16 + nl limbs (gamma < q^2 N)
and y rows of 24 + nl (tau < q^3 N~), that is (80, 88) at nl = 64 and (112, 120) at
nl = 96, against Python's pow bit for bit.  pow parity needs no prime factors, so
the moduli are random odd values of full width."""
import pytest

from oracle.rng import Rng

pytestmark = pytest.mark.gpu

COUNTS = (1, 3, 17)
SHAPES = ((64, 80, 88), (96, 112, 120))


def _edge(rng, limbs):
    bits = 32 * limbs
    return [0, 1, 1 << (bits - 1), (1 << bits) - 1, rng.bits(bits)]


def _instances(nl, xl, yl):
    """17 commitments over two interleaved keys: x and y cycle through 0, 1, the top
    limb's top bit alone, all ones and random values, offset against each other and
    against the keys; x also takes a value with only its top 16 limbs set (the part
    of the row above a 2048- or 3072-bit N)."""
    rng = Rng(("commit-ct-bob-widths", nl))
    keys = []
    for _ in range(2):
        nt = rng.bits(32 * nl) | (1 << (32 * nl - 1)) | 1
        keys.append((nt, rng.sample_below(nt), rng.sample_below(nt)))
    inst = []
    for i in range(max(COUNTS)):
        ex = _edge(rng, xl) + [rng.bits(512) << (32 * (xl - 16))]
        ey = _edge(rng, yl)
        inst.append((ex[(i + i // 6) % 6], ey[(i + i // 5 + 2) % 5], i % 2))
    assert inst[2][0] >> (32 * (xl - 1) + 31) and not inst[5][0] & ((1 << (32 * (xl - 16))) - 1)
    want = [pow(keys[k][1], x, keys[k][0]) * pow(keys[k][2], y, keys[k][0]) % keys[k][0] for x, y, k in inst]
    return keys, inst, want


@pytest.fixture(scope="module")
def refs():
    return {shape: _instances(*shape) for shape in SHAPES}


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("shape", SHAPES)
def test_commit_at_bobs_widths_matches_pow(gpu_ctx, refs, shape, count):
    nl, xl, yl = shape
    keys, inst, want = refs[shape]
    X, Y, I = (list(v) for v in zip(*inst[:count]))
    assert gpu_ctx.pedersen_commit(X, Y, keys, I, nl, xl=xl, yl=yl) == want[:count]
