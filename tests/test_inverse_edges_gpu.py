"""csrc/inverse.hip on the inputs that reach the binary GCD's sign fix (y = m - 2^k,
inverse_model.edge_cases: negate, its top-lane case, the flipped cofactors) and on
the batch kernel's own launch shapes and group layouts, all six instantiations of
coop_inverse: inverse_coop_kernel <64, 8>, <96, 8>, <128, 8>, <192, 16> through
mod_inverse under FSDKR_CFG_INV_EACH, inverse_batch_kernel <64, 8>, <96, 4>,
<128, 8>, <192, 8> through mod_inverse(grouped=True).  Every value and unit flag is
compared with pow(y, -1, m) exactly."""
import math
import random

import pytest

import inverse_model as im

pytestmark = pytest.mark.gpu

LIMBS = [64, 96, 128, 192]


def _check(got, ys, ms, names=None):
    assert len(got) == len(ys)
    for k, (y, m, g) in enumerate(zip(ys, ms, got)):
        assert g == im.python_inverse(y, m), (names[k] if names else k, hex(y)[:40], hex(m)[:40])


def _odd(rnd, bits):
    return rnd.getrandbits(bits) | 1 | (1 << (bits - 1))


def _square(rnd, bits):
    return _odd(rnd, bits // 2) ** 2


def _unit(rnd, m):
    while True:
        y = rnd.randrange(2, m)
        if math.gcd(y, m) == 1:
            return y


@pytest.mark.parametrize("limbs", LIMBS)
def test_edge_inputs_one_inverse_each(gpu_ctx, limbs):
    """inverse_coop_kernel's four shapes"""
    from fsdkr._native import FSDKR_CFG_INV_EACH
    names, ys, ms = zip(*im.edge_cases(limbs))
    old = gpu_ctx.set_flags(gpu_ctx.flags | FSDKR_CFG_INV_EACH)
    try:
        got = gpu_ctx.mod_inverse(list(ys), list(ms), limbs)
    finally:
        gpu_ctx.set_flags(old)
    _check(got, ys, ms, names)


@pytest.mark.parametrize("limbs", LIMBS)
def test_edge_inputs_groups_of_one(gpu_ctx, limbs):
    """inverse_batch_kernel's one-element path: coop_inverse<limbs, G_batch> on the raw y.
    Cases that share a modulus go into different calls, so every group has one element."""
    calls = []
    for case in im.edge_cases(limbs):
        for call in calls:
            if all(case[2] != c[2] for c in call):
                call.append(case)
                break
        else:
            calls.append([case])
    assert sum(len(c) for c in calls) == len(im.edge_cases(limbs))
    for call in calls:
        names, ys, ms = zip(*call)
        assert len(set(ms)) == len(ms)
        _check(gpu_ctx.mod_inverse(list(ys), list(ms), limbs, grouped=True), ys, ms, names)


@pytest.mark.parametrize("limbs", LIMBS)
def test_edge_inputs_beside_a_non_unit(gpu_ctx, limbs):
    """Every modulus's group ends with a non-unit (3 where 3 divides m, else 0), so the
    group's product is not a unit and inverse_batch_kernel inverts each raw y on its own,
    after the prefix products and one inverse of the product."""
    names, ys, ms = (list(t) for t in zip(*im.edge_cases(limbs)))
    for m in sorted(set(ms)):
        names.append("non-unit")
        ys.append(3 if m % 3 == 0 and m > 3 else 0)
        ms.append(m)
        assert im.python_inverse(ys[-1], m) is None
    _check(gpu_ctx.mod_inverse(ys, ms, limbs, grouped=True), ys, ms, names)


@pytest.mark.parametrize("limbs", LIMBS)
def test_sign_fix_on_the_group_product(gpu_ctx, limbs):
    """In a unit group the binary GCD sees the prefix product y_1 .. y_n R^-(n-1) mod m
    (R = 2^(29 KD)), not any y: the last element is chosen so that this product is
    exactly m - 2^k, which takes the sign fix."""
    rnd = random.Random(31000 + limbs)
    bits = 32 * limbs
    R = 1 << (29 * im.BATCH_KD[limbs])
    names, ys, ms = [], [], []
    for make in (_odd, _square):
        for n in (2, 5):
            for kk in (30, 61, None):
                m = make(rnd, bits)
                assert m not in ms
                k = m.bit_length() // 2 if kk is None else kk
                head = [_unit(rnd, m) for _ in range(n - 1)]
                last = (m - (1 << k)) * pow(R, n - 1, m) * pow(math.prod(head), -1, m) % m
                group = head + [last]
                assert math.prod(group) * pow(R, -(n - 1), m) % m == m - (1 << k)
                P = group[0]                       # the kernel's chain, product by product
                for y in group[1:]:
                    P = P * y * pow(R, -1, m) % m
                assert P == m - (1 << k)
                for y in group:
                    names.append("%s n=%d k=%d" % (make.__name__, n, k))
                    ys.append(y)
                    ms.append(m)
    # the model takes T < 0 on such a product at the batch kernel's shape
    _, cov = im.inverse(ms[0] - (1 << 30), ms[0], limbs, im.BATCH_G[limbs])
    assert cov.neg_a + cov.neg_b >= 1
    _check(gpu_ctx.mod_inverse(ys, ms, limbs, grouped=True), ys, ms, names)


def _layout(limbs):
    """19 moduli, groups of 1, 2, 3, 8, 9 and 17 interleaved: (names, ys, ms)"""
    rnd = random.Random(47000 + limbs)
    bits = 32 * limbs
    sizes = [1, 2, 3, 8, 9, 17, 1, 2, 3, 8, 1, 2, 3, 1, 2, 3, 2, 1, 2]
    assert len(sizes) == 19 and set(sizes) == {1, 2, 3, 8, 9, 17}
    groups = []
    for gi, n in enumerate(sizes):
        if gi in (3, 4, 6):                        # the groups that get a non-unit: 3 | m
            m = 3 * (rnd.getrandbits(bits - 2) | 1 | (1 << (bits - 3)))
        elif gi == 5:                              # shorter than its slot
            m = _odd(rnd, bits - 137)
        elif gi % 3 == 0:
            m = _square(rnd, bits)
        else:
            m = _odd(rnd, bits)
        assert m < 1 << bits and m & 1 and all(m != g[0] for g in groups)
        ys = [_unit(rnd, m) for _ in range(n)]
        tag = ["g%d[%d/%d]" % (gi, i, n) for i in range(n)]
        if gi == 3:                                # n = 8: a non-unit first
            ys[0] = 3 * rnd.randrange(1, m // 3)
        if gi == 4:                                # n = 9: a non-unit last
            ys[-1] = 3 * rnd.randrange(1, m // 3)
        if gi == 6:                                # n = 1: a non-unit alone
            ys[0] = 3 * rnd.randrange(1, m // 3)
        if gi == 2:                                # n = 3: y = 0 first
            ys[0] = 0
        if gi == 5:                                # n = 17: 1 and m - 1 inside
            ys[5], ys[11] = 1, m - 1
        if gi == 9:                                # n = 8: m - 1 last, 1 first
            ys[0], ys[-1] = 1, m - 1
        groups.append((m, list(zip(tag, ys))))
    assert sizes[3] == 8 and sizes[4] == 9 and sizes[6] == 1 and sizes[2] == 3 and sizes[5] == 17 and sizes[9] == 8
    names, ys, ms = [], [], []
    heads = [0] * len(groups)
    while True:                                    # a random merge: the order inside a group is kept
        live = [i for i, (m, g) in enumerate(groups) if heads[i] < len(g)]
        if not live:
            break
        i = rnd.choice(live)
        m, g = groups[i]
        names.append(g[heads[i]][0])
        ys.append(g[heads[i]][1])
        ms.append(m)
        heads[i] += 1
    return names, ys, ms


@pytest.mark.parametrize("limbs", LIMBS)
def test_group_layout(gpu_ctx, limbs):
    """More groups than one block holds (8 at 8 lanes, 16 at 4), every group size class,
    instances interleaved so that `order` is a real permutation, non-units first, last
    and alone, y = 0 first, 1 and m - 1 inside, one short modulus."""
    names, ys, ms = _layout(limbs)
    assert len(set(ms)) == 19 and 60 <= len(ys) <= 80
    order = sorted(range(len(ms)), key=lambda i: ms[i])
    assert order != list(range(len(ms)))
    none = [n for n, y, m in zip(names, ys, ms) if im.python_inverse(y, m) is None]
    assert sorted(none) == sorted(["g2[0/3]", "g3[0/8]", "g4[8/9]", "g6[0/1]"])
    got = gpu_ctx.mod_inverse(ys, ms, limbs, grouped=True)
    _check(got, ys, ms, names)
    if limbs in (64, 128):
        assert got == gpu_ctx.mod_inverse(ys, ms, limbs)
