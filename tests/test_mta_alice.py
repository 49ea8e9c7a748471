"""CPU checks of Alice's side of MtA: fsdkr.mta.initiate / generate_alice over a
stand-in context that serves the device calls with pow (draw order, the single
commitment call and its public widths, bit equality with oracle.range_proofs, the
ValueErrors), verify_alice's host pre-pass, the AliceBatchC layout against the
header, and a Python model of the two-base comb's schedule (csrc/comb_ct.hip)
against pow."""
import ctypes
import dataclasses
import os
import subprocess

import pytest

import mta_oracle as mo
from oracle import paillier
from oracle import range_proofs as rp
from oracle import secp256k1 as ec
from oracle.rng import Rng

Q = ec.Q
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class PowContext:
    """The device calls of initiate / generate_alice by pow, recorded."""

    def __init__(self):
        self.calls = []

    def pedersen_commit(self, xs, ys, keys, key_idx, nl, xl=None, yl=None):
        self.calls.append(("pedersen_commit", dict(xs=list(xs), ys=list(ys), keys=list(keys), key_idx=list(key_idx),
                                                    nl=nl, xl=xl, yl=yl)))
        assert all(x >> (32 * xl) == 0 for x in xs) and all(y >> (32 * yl) == 0 for y in ys)
        assert all(h1 < nt and h2 < nt for nt, h1, h2 in keys)
        return [pow(keys[k][1], x, keys[k][0]) * pow(keys[k][2], y, keys[k][0]) % keys[k][0]
                for x, y, k in zip(xs, ys, key_idx)]

    def paillier_encrypt(self, ms, rs, ns, n_idx, nl):
        self.calls.append(("paillier_encrypt", dict(count=len(ms), ns=list(ns), n_idx=list(n_idx), nl=nl)))
        return [(1 + m * ns[i]) * pow(r, ns[i], ns[i] ** 2) % ns[i] ** 2 for m, r, i in zip(ms, rs, n_idx)]

    def modexp_batch(self, bases, exps, mods, mod_idx, mod_limbs, secret=False):
        self.calls.append(("modexp_batch", dict(count=len(bases), nl=mod_limbs, secret=secret)))
        return [pow(b, e, mods[i]) for b, e, i in zip(bases, exps, mod_idx)]


class LoggedRng:
    def __init__(self, seed):
        self.rng, self.bounds = Rng(seed), []

    def sample_below(self, upper):
        self.bounds.append(upper)
        return self.rng.sample_below(upper)


@pytest.fixture(scope="module")
def small_keys():
    """Two 768-bit Paillier keys with a statement each (the 2048-bit class)."""
    rng = Rng("mta-alice-cpu-keys")
    out = []
    for _ in range(2):
        ek, dk = paillier.keypair_with_modulus_size(768, rng)
        ekt, dkt = paillier.keypair_with_modulus_size(768, rng)
        out.append(dict(ek=ek, dk=dk, st=mo.dlog_statement(ekt.n, dkt.p, dkt.q, rng)))
    return out


def _oracle_run(keys, as_, seed):
    """The reference's alice_zkp (:650-670) per exchange over one stream, in initiate's
    order: every r first, then the proofs."""
    rng = Rng(seed)
    rs = [rng.from_modulo(k["ek"].n) for k in keys]
    cs = [paillier.encrypt_with_chosen_randomness(k["ek"], a, r) for k, a, r in zip(keys, as_, rs)]
    pfs = [rp.generate(a, c, k["ek"], k["st"], r, rng) for k, a, c, r in zip(keys, as_, cs, rs)]
    return cs, rs, pfs


def _t(pf):
    return dataclasses.astuple(pf)


def test_initiate_over_pow_matches_the_oracle(small_keys):
    from fsdkr import mta
    keys = [small_keys[k % 2] for k in range(5)]
    rng0 = Rng("mta-alice-cpu-a")
    as_ = [0, Q - 1] + [rng0.sample_below(Q) for _ in range(3)]
    eks, sts = [k["ek"] for k in keys], [k["st"] for k in keys]
    ctx, rng = PowContext(), LoggedRng("mta-alice-cpu")
    a_encs, rs, proofs = mta.initiate(as_, eks, sts, rng, ctx=ctx)
    want_c, want_r, want_p = _oracle_run(keys, as_, "mta-alice-cpu")
    assert a_encs == want_c and rs == want_r
    assert [_t(p) for p in proofs] == [_t(p) for p in want_p]
    assert all(rp.verify(rp.AliceProof(*_t(p)), c, ek, st) for p, c, ek, st in zip(proofs, a_encs, eks, sts))
    # draw order: every r (below N, repeated until a unit) first, then per proof alpha,
    # beta, gamma, ro
    b = rng.bounds
    assert b[:5] == [ek.n for ek in eks]                  # no rejection at these sizes
    assert len(b) == 5 + 4 * 5
    for k, (ek, st) in enumerate(zip(eks, sts)):
        assert b[5 + 4 * k:9 + 4 * k] == [Q ** 3, ek.n, Q ** 3 * st.N, Q * st.N]
    # calls: Enc(a; r), ONE commitment call of two instances per proof at the public
    # widths, Enc(alpha; beta), r^e with a public exponent
    names = [c[0] for c in ctx.calls]
    assert names == ["paillier_encrypt", "pedersen_commit", "paillier_encrypt", "modexp_batch"]
    pc = ctx.calls[1][1]
    assert pc["nl"] == 64 and pc["xl"] == 24 and pc["yl"] == 88
    assert len(pc["xs"]) == 10 and pc["xs"][0::2] == as_
    assert pc["keys"] == [(k["st"].N, k["st"].g, k["st"].ni) for k in small_keys]
    assert pc["key_idx"] == [0, 0, 1, 1, 0, 0, 1, 1, 0, 0]
    assert ctx.calls[0][1]["ns"] == [small_keys[0]["ek"].n, small_keys[1]["ek"].n]
    assert ctx.calls[3][1]["secret"] is False
    # generate_alice alone over the same stream position
    replay = Rng("mta-alice-cpu")
    for ek in eks:
        replay.from_modulo(ek.n)
    again = mta.generate_alice(list(zip(as_, a_encs, eks, sts, rs)), replay, ctx=PowContext())
    assert again == proofs


def test_width_class_and_errors(small_keys):
    from fsdkr import mta
    from fsdkr.types import DLogStatement
    keys = small_keys
    eks, sts = [k["ek"] for k in keys], [k["st"] for k in keys]
    wide = DLogStatement((1 << 2100) + 1, 3, 5)            # an N~ above 2048 bits: the 3072-bit class
    ctx = PowContext()
    mta.initiate([1, 2], eks, [sts[0], wide], Rng("w"), ctx=ctx)
    pc = [c[1] for c in ctx.calls if c[0] == "pedersen_commit"][0]
    assert pc["nl"] == 96 and pc["xl"] == 24 and pc["yl"] == 120
    assert all(c[1]["nl"] == 96 for c in ctx.calls)
    for bad in (-1, Q):
        ctx = PowContext()
        with pytest.raises(ValueError):
            mta.initiate([1, bad], eks, sts, Rng("w"), ctx=ctx)
        assert ctx.calls == []
    with pytest.raises(ValueError):
        mta.initiate([1], eks, sts, Rng("w"), ctx=PowContext())
    with pytest.raises(ValueError):
        mta.generate_alice([(1 << 768, 1, eks[0], sts[0], 1)], Rng("w"), ctx=PowContext())
    assert mta.initiate([], [], [], Rng("w"), ctx=PowContext()) == ([], [], [])
    assert mta.generate_alice([], Rng("w"), ctx=PowContext()) == []
    assert list(mta.verify_alice([], [], [], [], ctx=PowContext())) == []


def test_verify_prepass(small_keys):
    from fsdkr import mta
    from fsdkr.batch import UnsupportedInput
    from fsdkr.types import AliceProof
    keys = [small_keys[k % 2] for k in range(4)]
    eks, sts = [k["ek"] for k in keys], [k["st"] for k in keys]
    cs, rs, pfs = _oracle_run(keys, [1, 2, 3, 4], "mta-alice-prepass")
    pfs = [AliceProof(*_t(p)) for p in pfs]
    pfs[1] = dataclasses.replace(pfs[1], s1=Q ** 3 + 12345, e=(1 << 300) + 7)
    pfs[2] = dataclasses.replace(pfs[2], s1=Q ** 3, e=0)
    pp = mta.prepass_alice(pfs, cs, eks, sts)
    assert pp["count"] == 4 and pp["nl"] == 64 and pp["key_idx"] == [0, 1, 0, 1]
    assert pp["keys"] == [(k["ek"].n, k["st"].N, k["st"].g, k["st"].ni) for k in small_keys]
    assert pp["s1"] == [pfs[0].s1, Q ** 3 + 1, Q ** 3, pfs[3].s1]
    assert pp["e"] == [pfs[0].e, 1 << 256, 0, pfs[3].e]
    b, keep = mta._alice_batch(pp, cs, pfs)
    assert (b.count, b.n_keys, b.nl, b.el, b.s1l) == (4, 2, 64, 9, 24)
    # not representable: negative fields, values wider than their field, even moduli
    for f, v in (("s", 1 << 2048), ("z", 1 << 2048), ("s1", -1), ("e", -1), ("s2", -1), ("z", -1)):
        with pytest.raises(UnsupportedInput):
            mta.prepass_alice([dataclasses.replace(pfs[0], **{f: v})], cs[:1], eks[:1], sts[:1])
    with pytest.raises(UnsupportedInput):
        mta.prepass_alice(pfs[:1], [1 << 4096], eks[:1], sts[:1])
    with pytest.raises(UnsupportedInput):
        mta.prepass_alice(pfs[:1], cs[:1], [paillier.EncryptionKey.from_n(eks[0].n + 1)], sts[:1])
    with pytest.raises(ValueError):
        mta.prepass_alice(pfs[:2], cs[:1], eks[:2], sts[:2])


def test_alice_batch_layout(tmp_path):
    """sizeof / offsetof of fsdkr_alice_batch (gcc) equal the ctypes mirror."""
    from fsdkr import _native
    py = _native.AliceBatchC
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "fsdkr/fsdkr.h"', "int main(void){",
             'printf("%zu\\n", sizeof(fsdkr_alice_batch));']
    lines += [f'printf("%zu\\n", offsetof(fsdkr_alice_batch, {f}));' for f, _ in py._fields_]
    lines.append("return 0;}")
    c = tmp_path / "probe.c"
    c.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(REPO, "include"), str(c), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(py)] + [getattr(py, f).offset for f, _ in py._fields_]
    assert [f for f, _ in py._fields_] == ["count", "n_keys", "nl", "el", "s1l", "s2l", "N", "Ntilde", "h1", "h2",
                                           "key_idx", "cipher", "z", "s", "e", "s1", "s2"]


# ---- the two-base comb's schedule (csrc/comb_ct.hip, comb.hip comb_sched_kernel) -----
H = 4


def blocks(limbs, b):
    """v = ceil(32 limbs / (4 b)): the geometry comes from the limb count alone."""
    return (32 * limbs + H * b - 1) // (H * b)


def sched(e, limbs, v, b):
    """comb_sched_kernel: step s = (b - 1 - k) v + j holds the 4 bits t = (r v + j) b + k,
    r < 4, of the exponent zero-padded from `limbs` limbs."""
    assert e >> (32 * limbs) == 0
    out = []
    for s in range(v * b):
        k, j = b - 1 - s // v, s % v
        out.append(sum(((e >> ((r * v + j) * b + k)) & 1) << r for r in range(H)))
    return out


def tables(base, v, b, N):
    """G[j][u] = prod over the bits r of u of base^(2^((r v + j) b))."""
    G = []
    for j in range(v):
        P = [pow(base, 1 << ((r * v + j) * b), N) for r in range(H)]
        row = []
        for u in range(1 << H):
            g = 1
            for r in range(H):
                if (u >> r) & 1:
                    g = g * P[r] % N
            row.append(g)
        G.append(row)
    return G


def commit_model(h1, h2, x, y, xl, yl, b, N):
    """commit_ct_kernel's loop: per column the x blocks then the y blocks, a squaring
    before every column but the first; every digit is multiplied in, zeros as G[j][0]
    = 1.  Returns (value, squarings, products)."""
    vx, vy = blocks(xl, b), blocks(yl, b)
    Gx, Gy = tables(h1, vx, b, N), tables(h2, vy, b, N)
    sx, sy = sched(x, xl, vx, b), sched(y, yl, vy, b)
    acc = Gx[0][sx[0]]
    j, ix, iy, sq, mul = 0, 1, 0, 0, 0
    for _ in range(1, (vx + vy) * b):
        j += 1
        if j == vx + vy:
            j = 0
            acc = acc * acc % N
            sq += 1
        if j < vx:
            acc = acc * Gx[j][sx[ix]] % N
            ix += 1
        else:
            acc = acc * Gy[j - vx][sy[iy]] % N
            iy += 1
        mul += 1
    assert ix == vx * b and iy == vy * b
    return acc, sq, mul


@pytest.mark.parametrize("widths", [(8, 72), (24, 88), (64, 88), (1, 1), (24, 120)])
@pytest.mark.parametrize("b", [1, 3, 8, 13, 64])
def test_comb_schedule_model(widths, b):
    xl, yl = widths
    rng = Rng(("comb-ct-model", xl, yl, b))
    N = rng.bits(190) | (1 << 189) | 1
    h1, h2 = rng.sample_below(N), rng.sample_below(N)
    vx, vy = blocks(xl, b), blocks(yl, b)
    assert H * vx * b >= 32 * xl and H * vy * b >= 32 * yl
    assert (widths == (1, 1) or b == 1 or vx != vy) and (b == 1) == (vx == 8 * xl)

    def edge(limbs):
        bits = 32 * limbs
        return [0, 1, (1 << bits) - 1, int("0f" * (4 * limbs), 16), int("f0" * (4 * limbs), 16), 1 << (bits - 1),
                rng.bits(bits)]

    ex, ey = edge(xl), edge(yl)
    for i in range(7):
        x, y = ex[i], ey[(i + 3) % 7 if i else 0]
        got, sq, mul = commit_model(h1, h2, x, y, xl, yl, b, N)
        assert got == pow(h1, x, N) * pow(h2, y, N) % N
        assert (sq, mul) == (b - 1, b * (vx + vy) - 1)     # the same count for every exponent
    assert commit_model(1, N - 1, ex[2], ey[2], xl, yl, b, N)[0] == pow(N - 1, ey[2], N)
