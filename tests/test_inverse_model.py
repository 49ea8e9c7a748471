"""The lane-level model of coop_inverse (inverse_model.py) on the shared edge inputs,
at the six shapes csrc/inverse.hip instantiates.  Pure Python, no GPU.

The model checks itself as it runs (every norm against big integers, no carry
pending when norm's round loop ends, u, v in [0, m) after every mdiv); this test
adds that its result equals pow(y, -1, m) and that the edge inputs reach the paths
random inputs do not: the sign fix (T < 0) on both sides, mdiv's three outcomes,
a norm of G - 1 rounds (the longest a carry can travel), norm's slow path with
either carry sign and on the top lane, and the nbits = 62 clamp.

Which inputs reach what (the same at all four widths): y = m - 2^k for k = 30, 31,
59, 60, 61 and bits(m)/2 takes T < 0 on the a side; y = m - 2 under
m = (2^(bits/2) - 1)^2 and y = m - 2^29 under the random or the square modulus take
it on the b side.  mdiv's subtraction (a step ending at or above m) mostly happens
on the step where a reaches 0 and then for about one plain y in three; the
structured y above do not reach it, the non-units and the plain values under the
61-bit modulus do."""
import random

import pytest

import inverse_model as im


@pytest.fixture(scope="module")
def cases():
    return {K32: im.edge_cases(K32) for K32 in (64, 96, 128, 192)}


def test_edge_cases_shape(cases):
    for K32, cs in cases.items():
        names = [c[0] for c in cs]
        assert len(set(names)) == len(names)
        assert 55 <= len(cs) <= 90
        assert {n.split(":")[0] for n in names} == {n for n, _ in im.edge_moduli(K32)}
        assert sum(im.python_inverse(y, m) is None for _, y, m in cs) >= 5


@pytest.mark.parametrize("K32,G", im.SHAPES)
def test_model_matches_pow_and_covers(cases, K32, G):
    total = im.Coverage(G)
    neg_cases = []
    for name, y, m in cases[K32]:
        got, cov = im.inverse(y, m, K32, G)
        assert got == im.python_inverse(y, m), name
        total.add(cov)
        if cov.neg_a or cov.neg_b:
            neg_cases.append(name)
    print(total)
    print("sign fix taken by:", neg_cases)
    assert total.neg_a >= 1, total
    assert total.neg_b >= 1, total
    assert total.mdiv_add >= 1 and total.mdiv_sub >= 1 and total.mdiv_keep >= 1, total
    assert total.max_rounds <= G - 1, total
    assert total.rounds_max >= 1, total
    assert total.slow_plus >= 1 and total.slow_minus >= 1 and total.slow_top >= 1, total
    assert total.clamp62 >= 1, total
    # y = m - 2^k, 30 <= k <= bits(m)/2, answers with the sign fix on every full-size modulus
    for mname in ("odd", "nsq", "short137", "ones", "halfones_sq"):
        assert any(n.startswith(mname + ":m-2^30") for n in neg_cases), (mname, neg_cases)


@pytest.mark.parametrize("K32,G", [(64, 8), (96, 4)])
def test_random_inputs_do_not_reach_the_sign_fix(K32, G):
    """Why the edge inputs exist: random units below a random modulus never take T < 0."""
    rnd = random.Random(K32)
    total = im.Coverage(G)
    for _ in range(6):
        m = rnd.getrandbits(32 * K32) | 1 | (1 << (32 * K32 - 1))
        y = rnd.randrange(m)
        got, cov = im.inverse(y, m, K32, G)
        assert got == im.python_inverse(y, m)
        total.add(cov)
    assert total.neg_a == 0 and total.neg_b == 0, total
