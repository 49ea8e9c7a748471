"""GA's N-adic joint tail (csrc/modexp.hip modexp_nadic_tail_kernel) through
fsdkr_modexp_nadic_batch and collect(): the low 256 exponent bits in pair form over
the head's own odd-power table, base2 entered in one pass from its two 2048-bit
halves.  Bit-exact against Python's pow, against the same call with the full-width
tail (FSDKR_CFG_GA_TAIL_FULLWIDTH) and against the full-width split chains at 16
lanes; one collect() at n = 4, t = 1 with a tampered PDL s2 and a tampered Alice s
gives the same verdicts and LocalKey under both tails, equal to the oracle's."""
import copy
import os
import random
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import tamper  # noqa: E402

pytestmark = pytest.mark.gpu

TOP = (1 << 2048) - 1
LOW = (1 << 256) - 1
KB = 2048
FIELDS = ("feldman", "pdl", "range", "ped", "ck")


def _odd(rnd, bits):
    return rnd.getrandbits(bits) | (1 << (bits - 1)) | 1


def _with_tail(ctx, fullwidth):
    from fsdkr._native import FSDKR_CFG_GA_TAIL_FULLWIDTH
    return ctx.set_flags((ctx.flags | FSDKR_CFG_GA_TAIL_FULLWIDTH) if fullwidth
                         else (ctx.flags & ~FSDKR_CFG_GA_TAIL_FULLWIDTH))


def test_modexp_nadic_tail(gpu_ctx):
    rnd = random.Random(9009)
    N0, N1, N2 = _odd(rnd, 2048), _odd(rnd, 2048), _odd(rnd, 1500)
    hi = (rnd.getrandbits(1791) | (1 << 1791)) << 256
    pairs = [                                   # (N, E): E is shared by the chains of its entry
        (N0, N0),
        (N0, hi | (0x5B << 252) | rnd.getrandbits(250)),   # a window straddles bit 256
        (N0, hi | LOW),                         # the low 256 bits all ones
        (N0, hi),                               # all zero
        (N1, hi | 1),                           # a single bit 0
        (N1, rnd.getrandbits(255) | (1 << 255)),   # E < 2^256: a head without bits
        (N1, rnd.getrandbits(200) | 1),
        (N1, 0),
        (TOP, TOP),
        (TOP, (0x7F << 250) | 1),
        (N2, N2),
        (N2, hi | LOW),
        (3, 3),
        (3, hi | rnd.getrandbits(256)),
        (3, 5),
    ]
    Ns = [p[0] for p in pairs]
    exps = [p[1] for p in pairs]
    e2_edge = [0, 1, 15, 16, 1 << 255, LOW]
    idx, bases, bases2, e2 = [], [], [], []
    for k, N in enumerate(Ns):
        NN = N * N
        b2_edge = [1, NN - 1, TOP, 1 << 2048, rnd.randrange(NN)]   # any base2 below 2^4096 (not reduced at N = 3)
        row = [0, 1, N - 1, TOP] + [rnd.getrandbits(2048) for _ in range(8 + k % 4)]   # ragged: the waves are padded
        for j, b in enumerate(row):
            idx.append(k)
            bases.append(b)
            bases2.append(b2_edge[j % 5] if j < 10 else rnd.randrange(NN))
            e2.append(e2_edge[(j + k) % 6] if j < 9 else rnd.getrandbits(256))
    order = list(range(len(idx)))
    rnd.shuffle(order)
    idx, bases, bases2, e2 = ([v[o] for o in order] for v in (idx, bases, bases2, e2))
    assert 190 <= len(idx) <= 215
    mods = [n * n for n in Ns]
    got = gpu_ctx.modexp_nadic_batch(bases, bases2, e2, Ns, exps, idx)
    want = [pow(b, exps[i], mods[i]) * pow(y, f, mods[i]) % mods[i] for b, y, f, i in zip(bases, bases2, e2, idx)]
    bad = [k for k in range(len(idx)) if got[k] != want[k]]
    assert not bad, f"{len(bad)} mismatches against pow, first at {bad[0]} (modulus entry {idx[bad[0]]})"
    old = _with_tail(gpu_ctx, True)
    try:
        wide = gpu_ctx.modexp_nadic_batch(bases, bases2, e2, Ns, exps, idx)
    finally:
        gpu_ctx.set_flags(old)
    assert got == wide
    # the full-width split chains take a reduced base2
    gpu_ctx.set_modexp_group(16)
    try:
        full = gpu_ctx.modexp_joint_batch(bases, [y % mods[i] for y, i in zip(bases2, idx)], e2, mods, exps, idx)
    finally:
        gpu_ctx.set_modexp_group(0)
    assert got == full


def _run(ctx, msgs, lk, dk, fullwidth):
    from fsdkr import refresh
    from fsdkr.batch import CollectBatch
    old = _with_tail(ctx, fullwidth)
    try:
        b = CollectBatch(msgs, lk, [], 256, KB)
        v = ctx.verify_collect(b)
        e = refresh._error_of(b.first_error(v))
        first = None if e is None else (e.variant, e.fields)
        vec = {f: np.array(getattr(v, f)).copy() for f in FIELDS}
        k = copy.deepcopy(lk)
        try:
            refresh.collect(copy.deepcopy(msgs), k, dk, [], ctx=ctx, key_bits=KB)
            out = None
        except refresh.FsDkrError as err:
            out = (err.variant, err.fields)
    finally:
        ctx.set_flags(old)
    return vec, first, out, k


def _key(k):
    return (k.x_i, k.y, list(k.pk_vec), [x.n for x in k.paillier_key_vec])


def test_collect_n4_t1_tail_vs_fullwidth(gpu_ctx):
    from fsdkr import synth
    from oracle import protocol
    from oracle.rng import Rng
    msgs, joins, lk, dk = synth.synth_sessions(gpu_ctx, 1, n=4, t=1, seed=909, key_bits=KB)[0]
    assert not joins
    ko = copy.deepcopy(lk)
    protocol.collect(tamper.to_oracle(msgs), ko, dk, [], Rng("a9"), KB)
    R = n = len(msgs)
    for spec in ([], [("pdl_s2", 2, 1), ("range_s", 1, 3)]):
        m2, _ = tamper.inject(msgs, [], spec)
        pairs, mres, jres, first = tamper.expected(m2, [], lk, spec, KB)
        nad = _run(gpu_ctx, m2, lk, dk, False)
        wide = _run(gpu_ctx, m2, lk, dk, True)
        for f in FIELDS:
            assert np.array_equal(nad[0][f], wide[0][f]), f
        assert nad[1] == wide[1] == first
        assert nad[2] == wide[2] == first
        assert _key(nad[3]) == _key(wide[3])
        for v in (nad, wide):
            tamper.check_verdicts(type("V", (), {**v[0], "dlog": np.zeros(0, np.uint8)}), R, 0, n, pairs, mres, jres)
        if spec:
            assert first is not None and first[0] in ("PDLwSlackProof", "RangeProof")
        else:
            assert first is None and _key(nad[3]) == _key(ko)
