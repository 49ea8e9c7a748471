"""GA's half-width N-adic head (csrc/modexp.hip modexp_nadic_head_kernel) and the
tail that takes over from it, through fsdkr_modexp_nadic_batch: bit-exact against
Python's pow for base^E * base2^e2 mod N^2, and equal to the full-width split
chains (fsdkr_modexp_joint_batch at 16 lanes) on the zero-extended inputs."""
import random

import pytest

pytestmark = pytest.mark.gpu

TOP = (1 << 2048) - 1


def _odd(rnd, bits):
    return rnd.getrandbits(bits) | (1 << (bits - 1)) | 1


def test_modexp_nadic_head(gpu_ctx):
    """Moduli: three random 2048-bit N, N = 2^2048 - 1, a 2047-bit N, a 1500-bit N and
    N = 3.  Exponents: E = N shared per modulus (ragged runs, so the waves are padded),
    one E < 2^256 (no bits for the head) and E = 0.  Bases 0, 1, N - 1, N, 2^2048 - 1
    and random ones below 2^2048.  Second exponents 0, 1, 15, 16, 2^255, 2^256 - 1 and
    random, second base 1 and random."""
    rnd = random.Random(7077)
    Ns = [_odd(rnd, 2048) for _ in range(3)] + [TOP, _odd(rnd, 2047), _odd(rnd, 1500), 3]
    exps = list(Ns)
    Ns += [Ns[0], Ns[1]]                       # the same moduli under short exponents
    exps += [rnd.getrandbits(200) | 1, 0]
    e2_special = [0, 1, 15, 16, 1 << 255, (1 << 256) - 1]
    idx, bases, bases2, e2 = [], [], [], []
    for k, N in enumerate(Ns):
        row = [0, 1, N - 1, N, TOP] + [rnd.getrandbits(2048) for _ in range(11 + k % 3)]
        for j, b in enumerate(row):
            idx.append(k)
            bases.append(b)
            bases2.append(1 if j % 5 == 4 else rnd.randrange(N * N))
            e2.append(e2_special[j % 8] if j % 8 < 6 and k in (0, 3, 6, 7) else rnd.getrandbits(256))
    e2[:6] = e2_special                        # with base2 = 1 as well
    bases2[:6] = [1] * 6
    order = list(range(len(idx)))
    rnd.shuffle(order)
    idx, bases, bases2, e2 = ([v[o] for o in order] for v in (idx, bases, bases2, e2))
    assert 140 <= len(idx) <= 170
    mods = [n * n for n in Ns]
    got = gpu_ctx.modexp_nadic_batch(bases, bases2, e2, Ns, exps, idx)
    want = [pow(b, exps[i], mods[i]) * pow(y, f, mods[i]) % mods[i] for b, y, f, i in zip(bases, bases2, e2, idx)]
    bad = [k for k in range(len(idx)) if got[k] != want[k]]
    assert not bad, f"{len(bad)} mismatches against pow, first at {bad[0]} (modulus {idx[bad[0]]})"
    gpu_ctx.set_modexp_group(16)
    try:
        full = gpu_ctx.modexp_joint_batch(bases, bases2, e2, mods, exps, idx)
    finally:
        gpu_ctx.set_modexp_group(0)
    assert got == full
