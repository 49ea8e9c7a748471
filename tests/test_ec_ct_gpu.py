"""The secret-scalar secp256k1 entry points on the GPU (csrc/ec_ct.hip:
fsdkr_ec_mul_g_ct, the four-lane nibble comb; fsdkr_ec_msm_ct, masked windows
over a per-term table) against the oracle's curve arithmetic and against the
public-scalar fsdkr_ec_msm on the same inputs: edge scalars (the model test's
list: 0, q, q +- 1, 2^256 - 1, +-C, values >= q), counts at the quad, wave and
block boundaries, a partial last quad, points at infinity and identity outputs."""
import random

import pytest

from oracle import secp256k1 as ec

from test_ec_ct_model import EDGE_CT

pytestmark = pytest.mark.gpu
N = ec.Q
_WANT = {}


def _g(k):
    """k G by the oracle, computed once per scalar for the whole module."""
    if k not in _WANT:
        _WANT[k] = ec.mul(ec.G, k % N)
    return _WANT[k]


def _via_msm(ctx, ks):
    return ctx.ec_msm([[ec.G]] * len(ks), [[k] for k in ks])


def test_mul_g_edge_and_random_scalars(gpu_ctx):
    rnd = random.Random(31)
    ks = EDGE_CT + [N + rnd.randrange(2 ** 256 - N) for _ in range(4)] + [rnd.randrange(2 ** 256) for _ in range(12)]
    got = gpu_ctx.ec_mul_g(ks)
    assert got == [_g(k) for k in ks]
    assert got == _via_msm(gpu_ctx, ks)


@pytest.mark.parametrize("count", [1, 3, 4, 5, 63, 64, 65, 257])
def test_mul_g_counts(gpu_ctx, count):
    rnd = random.Random(32)                       # one stream: every count shares its leading scalars
    ks = [rnd.randrange(2 ** 256) for _ in range(257)][:count]
    got = gpu_ctx.ec_mul_g(ks)
    assert len(got) == count
    assert got == _via_msm(gpu_ctx, ks)
    assert got[:8] == [_g(k) for k in ks[:8]] and got[-1] == _g(ks[-1])


def test_mul_g_edges_in_the_partial_last_quad(gpu_ctx):
    rnd = random.Random(33)
    for tail in ([0, N, 2 ** 256 - 1], [N - 1], [EDGE_CT[-3], EDGE_CT[-4]]):
        ks = [rnd.randrange(2 ** 256) for _ in range(64)] + tail
        assert gpu_ctx.ec_mul_g(ks) == [_g(k) for k in ks]


def _msm_case(rnd, outputs, terms):
    pts = [ec.G, ec.neg(ec.G), None] + [ec.mul(ec.G, rnd.randrange(1, N)) for _ in range(5)]
    rows, scs = [], []
    for o in range(outputs):
        rows.append([pts[(o + j) % len(pts)] for j in range(terms)])
        scs.append([EDGE_CT[(o * terms + j) % len(EDGE_CT)] if o < 2 * len(EDGE_CT) else rnd.randrange(2 ** 256)
                    for j in range(terms)])
    return rows, scs


def _msm_want(rows, scs):
    want = []
    for row, ks in zip(rows, scs):
        acc = None
        for pt, k in zip(row, ks):
            acc = ec.add(acc, ec.mul(pt, k % N))
        want.append(acc)
    return want


@pytest.mark.parametrize("terms", [1, 3])
def test_msm_secret_edges_vs_oracle(gpu_ctx, terms):
    rows, scs = _msm_case(random.Random(34 + terms), 2 * len(EDGE_CT) + 8, terms)
    # k = 0 on a finite point and any k on the point at infinity are both in the walk
    assert any(k == 0 and pt is not None for r, s in zip(rows, scs) for pt, k in zip(r, s))
    assert any(k != 0 and pt is None for r, s in zip(rows, scs) for pt, k in zip(r, s))
    got = gpu_ctx.ec_msm(rows, scs, secret=True)
    assert got == _msm_want(rows, scs)
    assert got == gpu_ctx.ec_msm(rows, scs)


def test_msm_secret_identity_outputs(gpu_ctx):
    rnd = random.Random(36)
    pts = [ec.G, ec.neg(ec.G), ec.mul(ec.G, rnd.randrange(1, N))]
    ks = [1, N - 1, rnd.randrange(1, N), (N + 1) // 2]
    rows = [[pt, pt] for pt in pts for _ in ks]
    scs = [[k, N - k] for _ in pts for k in ks]
    assert gpu_ctx.ec_msm(rows, scs, secret=True) == [None] * len(rows)
    assert gpu_ctx.ec_msm([[None]], [[5]], secret=True) == [None]
    assert gpu_ctx.ec_msm([[ec.G]], [[0]], secret=True) == [None]


@pytest.mark.parametrize("count", [1, 65, 257])
def test_msm_secret_counts(gpu_ctx, count):
    rnd = random.Random(37)
    pt = ec.mul(ec.G, 0xC0FFEE)
    ks = [rnd.randrange(2 ** 256) for _ in range(257)][:count]
    got = gpu_ctx.ec_msm([[pt]] * count, [[k] for k in ks], secret=True)
    assert len(got) == count
    assert got == gpu_ctx.ec_msm([[pt]] * count, [[k] for k in ks])
    assert got[0] == ec.mul(pt, ks[0] % N) and got[-1] == ec.mul(pt, ks[-1] % N)


def test_empty_calls(gpu_ctx):
    assert gpu_ctx.ec_mul_g([]) == []
    assert gpu_ctx.ec_msm([], [], secret=True) == []


def test_cached_table_gives_the_same_answers(gpu_ctx):
    ks = EDGE_CT[:12]
    first = gpu_ctx.ec_mul_g(ks)
    assert gpu_ctx.ec_mul_g(ks) == first == [_g(k) for k in ks]
