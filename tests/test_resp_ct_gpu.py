"""GPU checks of the provers' response kernel (csrc/resp_ct.hip) through its parity
entry Context.resp_ct (fsdkr_resp_ct): out = e x + y against Python integers, at the
width pairs of both provers in both width classes ((8, 24) s1 of Bob, (24, 24) s1 of
Alice, (64, 80) / (96, 112) t1, (72, 88) / (104, 120) s2 and t2) and at the ends of
the accepted range, for counts on both sides of the 4-instance block and of 64.  The
operands cycle through 0, 1, all ones, 0x0f.., 0xf0.., the top bit alone and random
values, offset against each other as tests/test_commit_ct_gpu.py offsets its edge
values; e cycles through 0, 1, 2^256 - 1 and random.  all ones x all ones + all ones
drives a carry through every limb into the top one, and is placed at every pair."""
import ctypes

import numpy as np
import pytest

from oracle.rng import Rng

pytestmark = pytest.mark.gpu

PAIRS = [(8, 24), (24, 24), (64, 80), (72, 88), (96, 112), (104, 120), (1, 1), (128, 128)]
COUNTS = [1, 63, 64, 65, 130]
E_ONES = (1 << 256) - 1


@pytest.fixture(scope="module")
def ctx():
    from fsdkr import Context
    c = Context()
    yield c
    c.close()


def _edge(rng, limbs):
    bits = 32 * limbs
    return [0, 1, (1 << bits) - 1, int("0f" * (4 * limbs), 16), int("f0" * (4 * limbs), 16), 1 << (bits - 1),
            rng.bits(bits)]


def _rows(xl, yl, count):
    """(e, x, y) per row; row 0 is all ones x all ones + all ones."""
    rng = Rng(("resp-ct", xl, yl))
    out = [(E_ONES, (1 << 32 * xl) - 1, (1 << 32 * yl) - 1)]
    for i in range(1, count):
        ex, ey = _edge(rng, xl), _edge(rng, yl)
        es = [0, 1, E_ONES, rng.bits(256)]
        out.append((es[(i + i // 7) % 4], ex[(i + i // 7) % 7], ey[(i + i // 7 + i // 3) % 7]))
    return out


@pytest.fixture(scope="module")
def refs():
    """Per width pair: the 130 rows and their values; every count uses a prefix."""
    made = {}

    def get(pair):
        if pair not in made:
            rows = _rows(pair[0], pair[1], max(COUNTS))
            made[pair] = (rows, [e * x + y for e, x, y in rows])
        return made[pair]
    return get


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}x{p[1]}")
def test_resp_ct_matches_integers(ctx, refs, pair, count):
    xl, yl = pair
    rows, want = refs(pair)
    rows, want = rows[:count], want[:count]
    got = ctx.resp_ct([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], xl, yl)
    assert got == want
    # the carry case fills the top limb's first bit and nothing above it
    assert want[0].bit_length() <= 32 * (max(xl + 8, yl) + 1)
    # what the device was just compared on: the carry case at every count, and in the
    # full batch every edge value of e, x and y
    assert rows[0] == (E_ONES, (1 << 32 * xl) - 1, (1 << 32 * yl) - 1)
    if count == max(COUNTS):
        assert {0, 1, E_ONES} <= {r[0] for r in rows}
        for col, limbs in ((1, xl), (2, yl)):
            assert set(_edge(Rng("unused"), limbs)[:6]) <= {r[col] for r in rows}


def test_error_returns(ctx):
    from fsdkr import _native
    L, h = ctx._lib, ctx.handle
    buf = np.ones((4, 140), dtype=np.uint32)
    p = buf.ctypes.data_as(_native.u32p)
    null = ctypes.cast(None, _native.u32p)
    for xl, yl in ((0, 8), (129, 8), (8, 0), (8, 129)):
        assert L.fsdkr_resp_ct(h, 2, p, p, xl, p, yl, p) == _native.FSDKR_E_ARG
    for args in ((null, p, p, p), (p, null, p, p), (p, p, null, p), (p, p, p, null)):
        e, x, y, o = args
        assert L.fsdkr_resp_ct(h, 2, e, x, 8, y, 24, o) == _native.FSDKR_E_ARG
    assert L.fsdkr_resp_ct(h, 0, null, null, 8, null, 24, null) == _native.FSDKR_OK
    assert ctx.resp_ct([], [], [], 8, 24) == []
    # the context still works after the refusals
    assert ctx.resp_ct([3], [5], [7], 8, 24) == [22]
