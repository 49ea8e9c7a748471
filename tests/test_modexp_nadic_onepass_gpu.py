"""The one-pass table product of GA's N-adic head (csrc/mont29.hpp product_pair2)
through fsdkr_modexp_nadic_batch: exponents that drive the head's windows into
every corner (all-ones: the top table row in every window; one set bit per window:
the bottom row; set bits on either side of the hand-over at bit 256), bit-exact
against Python's pow and the full-width split chains at 16 lanes."""
import random

import pytest

pytestmark = pytest.mark.gpu

TOP = (1 << 2048) - 1
LOW = (1 << 256) - 1


def _odd(rnd, bits):
    return rnd.getrandbits(bits) | (1 << (bits - 1)) | 1


def test_modexp_nadic_onepass(gpu_ctx):
    rnd = random.Random(8008)
    N0, N1 = _odd(rnd, 2048), _odd(rnd, 1500)
    hi = rnd.getrandbits(1792) << 256
    pairs = [                                   # (N, E): E is shared by the chains of its entry
        (N0, TOP),                              # every window 127
        (N0, sum(1 << k for k in range(256, 2048, 7))),   # every window 1, six squarings between
        (N0, 0xFF << 255),                      # bits 255-262: the head's last window is clamped at 256
        (N0, 1 << 256),
        (N0, 1 << 255),                         # nothing for the head
        (N0, hi | LOW),
        (N0, hi | 1),
        (TOP, TOP),
        (TOP, (0xFF << 255) | 1),
        (N1, hi | LOW),
        (N1, TOP),
        (3, TOP),
        (3, 1 << 256),
        (N0, 0),
    ]
    Ns = [p[0] for p in pairs]
    exps = [p[1] for p in pairs]
    idx, bases, bases2, e2 = [], [], [], []
    for k, N in enumerate(Ns):
        NN = N * N
        half = rnd.getrandbits(2048)
        b2s = [(0, 0), (0, rnd.getrandbits(256) | 1), (half % NN, rnd.getrandbits(256)),
               ((half << 2048) % NN if NN >> 2048 else half % NN, rnd.getrandbits(256)), (NN - 1, LOW), (1, 0)]
        row = [0, 1, N - 1, TOP] + [rnd.getrandbits(2048) for _ in range(9 + k % 3)]
        for j, b in enumerate(row):
            y, f = b2s[j] if j < len(b2s) else (rnd.randrange(NN), rnd.getrandbits(256))
            idx.append(k)
            bases.append(b)
            bases2.append(y)
            e2.append(f)
    order = list(range(len(idx)))
    rnd.shuffle(order)
    idx, bases, bases2, e2 = ([v[o] for o in order] for v in (idx, bases, bases2, e2))
    assert 180 <= len(idx) <= 210
    mods = [n * n for n in Ns]
    got = gpu_ctx.modexp_nadic_batch(bases, bases2, e2, Ns, exps, idx)
    want = [pow(b, exps[i], mods[i]) * pow(y, f, mods[i]) % mods[i] for b, y, f, i in zip(bases, bases2, e2, idx)]
    bad = [k for k in range(len(idx)) if got[k] != want[k]]
    assert not bad, f"{len(bad)} mismatches against pow, first at {bad[0]} (modulus entry {idx[bad[0]]})"
    gpu_ctx.set_modexp_group(16)
    try:
        full = gpu_ctx.modexp_joint_batch(bases, bases2, e2, mods, exps, idx)
    finally:
        gpu_ctx.set_modexp_group(0)
    assert got == full
