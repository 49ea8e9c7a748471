"""prod3_kernel (csrc/vmont.hip) through its parity entry Context.prod3 (fsdkr_prod3):
out = a*b*c mod N, every limb against Python integers, at the four launch shapes of
the kernel (tests/test_eq_check_gpu.py SHAPES: the two kernels share the table).

The kernel takes its operands as given: nothing has to be reduced, the two closing
products by R^2 mod N bring any slot-wide value under 2N before the one conditional
subtraction.  So the edges are operands at the end of the slot over a full-width, a
half-width and a three-valued modulus; the output side is covered by results whose
only nonzero limbs lie in one lane's digits."""
import functools

import pytest

from oracle.rng import Rng
from test_eq_check_gpu import COUNTS, SHAPES, WIDTHS, geom

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def moduli(K):
    """Full-width, 2^bits - 1, half-width, 3, and one 61 bits short."""
    rng = Rng(("prod3-mod", K))
    return [rng.bits(32 * K) | (1 << (32 * K - 1)) | 1, (1 << (32 * K)) - 1,
            rng.bits(16 * K) | (1 << (16 * K - 1)) | 1, 3, rng.bits(32 * K - 61) | (1 << (32 * K - 62)) | 1]


def run(ctx, K, rows, mods, lens=None):
    """rows: (a, b, c, modulus index); every output limb against a*b*c % N."""
    want = [a * b * c % mods[mi] for a, b, c, mi in rows]
    got = ctx.prod3([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], mods, [r[3] for r in rows], K,
                    lens=lens)
    wrong = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    print(f"K32={K}: {len(rows)} rows, rows that differ: {wrong[:16]}")
    assert not wrong, f"{len(wrong)} of {len(rows)} products differ; first rows: {wrong[:16]}"
    return want


@functools.lru_cache(maxsize=None)
def mixed_rows(K):
    """257 rows over the five moduli: random operands (anywhere in the slot), the end of
    the slot in one, two and all three operands, zero and one in every position."""
    mods = moduli(K)
    rng = Rng(("prod3-rows", K))
    top = (1 << (32 * K)) - 1
    rows = []
    for i in range(max(COUNTS)):
        mi = i % 5
        a, b, c = rng.bits(32 * K), rng.bits(32 * K), rng.bits(32 * K)
        kind = (i // 5) % 10
        if kind == 1:
            a = b = c = top
        elif kind == 2:
            a, c = top, mods[mi] - 1
        elif kind == 3:
            b = top
        elif kind == 4:
            a, b, c = [(0, b, c), (a, 0, c), (a, b, 0)][(i // 50) % 3]
        elif kind == 5:
            a, b, c = [(1, 1, c), (a, 1, 1), (1, b, 1)][(i // 50) % 3]
        elif kind == 6:
            a, b, c = 1, 1, 1
        elif kind == 7:
            a, b, c = mods[mi] - 1, mods[mi] - 1, mods[mi] - 1
        rows.append((a, b, c, mi))
    return rows


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("K", WIDTHS)
def test_prod3_matches_integers(gpu_ctx, K, count):
    """Prefixes of one row set at counts around the 32 (8 lanes) and 64 (4 lanes)
    instances of a block; the last instance is all three operands at the end of the
    slot over the full-width modulus."""
    top = (1 << (32 * K)) - 1
    rows = list(mixed_rows(K)[:count - 1]) + [(top, top, top, 0)]
    want = run(gpu_ctx, K, rows, moduli(K))
    if count == max(COUNTS):
        assert {0, 1} <= set(want) and sum(1 for r in rows if r[:3] == (top, top, top)) >= 5
        assert {r[3] for r in rows if r[:3] == (top, top, top)} == set(range(5))


@pytest.mark.parametrize("K", WIDTHS)
def test_prod3_result_in_one_lane(gpu_ctx, K):
    """a = 2^p, b = c = 1 with p at the first and last bit of every lane's digits (those
    below N), and the same value as a product 2^s * 2^t * 2^(p - s - t): the result's
    only nonzero limb moves through every lane and every output limb is compared."""
    KD, G, L, R = geom(K)
    N = moduli(K)[0]
    rows, ps = [], []
    for j in range(G):
        for p in (29 * j * L, min(29 * (j + 1) * L - 1, 32 * K - 2)):
            ps.append(p)
            rows += [(1 << p, 1, 1, 0), (1, 1 << p, 1, 0), (1, 1, 1 << p, 0), (1 << (p // 3), 1 << (p // 3), 1 << (p - 2 * (p // 3)), 0)]
    assert len(set(p // 29 // L for p in ps)) == G and max(ps) == 32 * K - 2
    want = run(gpu_ctx, K, rows, [N])
    assert want == [1 << p for p in ps for _ in range(4)]


@pytest.mark.parametrize("K", WIDTHS)
def test_prod3_short_rows(gpu_ctx, K):
    """Operand rows of 1 limb, of K32 limbs, and mixed (1, K32, 8)."""
    mods = moduli(K)
    for lens in [(1, 1, 1), (K, K, K), (1, K, 8), (K - 1, 1, K)]:
        rng = Rng(("prod3-short", K, lens))
        rows = [tuple(rng.bits(32 * n) for n in lens) + (i % 5,) for i in range(33)]
        rows += [tuple((1 << (32 * n)) - 1 for n in lens) + (mi,) for mi in range(5)]
        run(gpu_ctx, K, rows, mods, lens=lens)


def test_prod3_refusals(gpu_ctx):
    from fsdkr import _native
    from fsdkr._native import FsdkrError
    N = moduli(64)[0]
    for mods, idx, K in (([N + 1], [0], 64), ([1], [0], 64), ([N], [1], 64)):
        with pytest.raises(FsdkrError) as e:
            gpu_ctx.prod3([2], [3], [5], mods, idx, K)
        assert e.value.code == _native.FSDKR_E_ARG
    with pytest.raises(FsdkrError) as e:
        gpu_ctx.prod3([2], [3], [5], [N], [0], 80)
    assert e.value.code == _native.FSDKR_E_UNSUPPORTED
    assert gpu_ctx.prod3([], [], [], [N], [], 64) == []
    assert gpu_ctx.prod3([2], [3], [5], [N], [0], 64) == [30]
    assert set(SHAPES) == {64, 96, 128, 192}
