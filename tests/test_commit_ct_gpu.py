"""GPU checks of the constant-time two-base comb (fsdkr_pedersen_commit_ct,
csrc/comb_ct.hip): h1^x h2^y mod N~ against Python's pow bit for bit, on edge
values of both exponents offset against each other and against three interleaved
keys, at every width pair of the range proofs and at counts around one and four of
the small launch's blocks (16 instances at 4 lanes: 15 / 16 / 17 and 63 / 64 / 65),
with the key padding; and the error returns.  Every count here runs the small
launch; the full block of 64 instances and the column counts of large batches are
in tests/test_commit_ct_shapes_gpu.py."""
import numpy as np
import pytest

from oracle.rng import Rng

pytestmark = pytest.mark.gpu

COUNTS_64 = (1, 15, 16, 17, 63, 64, 65, 130)
COUNTS_96 = (1, 5, 17)
WIDTHS_64 = ((8, 72), (24, 88), (64, 88), (1, 1))
WIDTHS_96 = ((24, 120),)


@pytest.fixture(scope="module")
def moduli(gpu_ctx):
    """Device-generated N~: two of 2048 bits, one of 1024 (zero-extended), two of 3072."""
    from fsdkr import keygen
    rng = Rng("commit-ct-keys")
    n2048 = [ek.n for ek, _ in keygen.keypairs_with_modulus_size(gpu_ctx, rng, 2048, 2)]
    short = keygen.keypairs_with_modulus_size(gpu_ctx, rng, 1024, 1)[0][0].n
    wide = [ek.n for ek, _ in keygen.keypairs_with_modulus_size(gpu_ctx, rng, 3072, 2)]
    assert short.bit_length() <= 1024 and all(n.bit_length() > 2048 for n in wide)
    return dict(n2048=n2048, short=short, wide=wide)


def _keys(nts, tag):
    """(N~, h1, h2) per modulus: random bases below N~; the middle key has h1 = 1, h2 = N~ - 1."""
    rng = Rng(("commit-ct-bases", tag))
    keys = [(nt, rng.sample_below(nt), rng.sample_below(nt)) for nt in nts]
    keys[1] = (nts[1], 1, nts[1] - 1)
    return keys


def _edge(rng, limbs):
    bits = 32 * limbs
    ones = (1 << bits) - 1
    return [0, 1, ones, int("0f" * (4 * limbs), 16), int("f0" * (4 * limbs), 16), 1 << (bits - 1), 1, rng.bits(bits)]


def _instances(n_keys, count, xl, yl, tag):
    """`count` commitments with the keys interleaved instance by instance and both
    exponents cycling through their edge values: 0, 1, all ones (every digit 15),
    0x0f..0f, 0xf0..f0, the top bit alone, bit 0 alone, random; the cycles are offset
    against each other and against the keys, and x = y = 0 occurs (i = 0)."""
    rng = Rng(("commit-ct", tag, xl, yl))
    out = []
    for i in range(count):
        ex, ey = _edge(rng, xl), _edge(rng, yl)
        x = ex[(i + i // 8) % 8]
        y = ey[(i + i // 8 + i // 3) % 8]
        out.append((x, y, i % n_keys))
    assert out[0][:2] == (0, 0)
    return out


def _want(keys, inst):
    return [pow(keys[k][1], x, keys[k][0]) * pow(keys[k][2], y, keys[k][0]) % keys[k][0] for x, y, k in inst]


class _Refs:
    """(instances, values by pow) per width pair, computed once on first use."""

    def __init__(self, keys, count, tag):
        self.keys, self.count, self.tag, self.made = keys, count, tag, {}

    def __getitem__(self, widths):
        if widths not in self.made:
            inst = _instances(len(self.keys), self.count, widths[0], widths[1], self.tag)
            self.made[widths] = (inst, _want(self.keys, inst))
        return self.made[widths]


@pytest.fixture(scope="module")
def ref64(moduli):
    """Per width pair: the 130 instances over three interleaved keys (one of 1024
    bits, one with h1 = 1, h2 = N~ - 1) and their values by pow; every count uses a prefix."""
    keys = _keys([moduli["n2048"][0], moduli["short"], moduli["n2048"][1]], "nl64")
    return keys, _Refs(keys, max(COUNTS_64), "nl64")


@pytest.fixture(scope="module")
def ref96(moduli):
    keys = _keys([moduli["wide"][0], moduli["n2048"][0], moduli["wide"][1]], "nl96")
    return keys, _Refs(keys, max(COUNTS_96), "nl96")


def _run(ctx, keys, inst, nl, xl, yl):
    X, Y, I = (list(v) for v in zip(*inst))
    return ctx.pedersen_commit(X, Y, keys, I, nl, xl=xl, yl=yl)


@pytest.mark.parametrize("count", COUNTS_64)
@pytest.mark.parametrize("widths", WIDTHS_64)
def test_commit_2048_matches_pow(gpu_ctx, ref64, widths, count):
    keys, refs = ref64
    inst, want = refs[widths]
    assert want[0] == 1                                   # x = y = 0
    assert _run(gpu_ctx, keys, inst[:count], 64, *widths) == want[:count]


@pytest.mark.parametrize("count", COUNTS_96)
@pytest.mark.parametrize("widths", WIDTHS_96)
def test_commit_3072_matches_pow(gpu_ctx, ref96, widths, count):
    keys, refs = ref96
    inst, want = refs[widths]
    assert _run(gpu_ctx, keys, inst[:count], 96, *widths) == want[:count]


def test_one_key_many_instances(gpu_ctx, ref64):
    """All instances under one key (a run of several blocks of that key), and a key
    of the table that no instance uses."""
    keys, refs = ref64
    inst, _ = refs[(24, 88)]
    one = [(x, y, 2) for x, y, _ in inst[:70]]
    assert _run(gpu_ctx, keys, one, 64, 24, 88) == _want(keys, one)


def test_error_returns(gpu_ctx, ref64):
    from fsdkr import _native
    keys, refs = ref64
    inst, want = refs[(8, 72)]
    L, h = gpu_ctx._lib, gpu_ctx.handle

    def call(nl, count, xl, yl, idx, ks):
        X = _native.ints_to_limbs([1] * max(1, count), max(1, min(xl, 128)))
        Y = _native.ints_to_limbs([1] * max(1, count), max(1, min(yl, 128)))
        Nt, H1, H2 = (_native.ints_to_limbs([k[c] for k in ks], nl) for c in range(3))
        I = np.ascontiguousarray(np.asarray(idx, dtype=np.uint32))
        O = np.zeros((max(1, count), nl), dtype=np.uint32)
        p = lambda a: a.ctypes.data_as(_native.u32p)
        return L.fsdkr_pedersen_commit_ct(h, nl, count, p(X), xl, p(Y), yl, p(I), p(Nt), p(H1), p(H2), len(ks), p(O))

    k0 = keys[0]
    assert call(80, 2, 8, 72, [0, 0], keys) == _native.FSDKR_E_UNSUPPORTED
    assert call(64, 0, 8, 72, [0], keys) == _native.FSDKR_OK               # count == 0
    assert call(64, 2, 8, 72, [0, 1], keys) == _native.FSDKR_OK
    for xl, yl in ((0, 72), (129, 72), (8, 0), (8, 129)):
        assert call(64, 2, xl, yl, [0, 0], keys) == _native.FSDKR_E_ARG
    assert call(64, 2, 8, 72, [0, 3], keys) == _native.FSDKR_E_ARG          # key_idx out of range
    for bad in ((k0[0] + 1, k0[1], k0[2]),                                  # even N~
                (1, 0, 0),                                                  # N~ = 1
                (k0[0], k0[0], k0[2]),                                      # h1 = N~: refused, not reduced
                (k0[0], k0[1], k0[0] + 5)):                                 # h2 > N~
        assert call(64, 2, 8, 72, [0, 0], [bad, keys[1]]) == _native.FSDKR_E_ARG
    with pytest.raises(_native.FsdkrError) as e:
        _run(gpu_ctx, keys, inst[:3], 80, 8, 72)
    assert e.value.code == _native.FSDKR_E_UNSUPPORTED
    assert gpu_ctx.pedersen_commit([], [], keys, [], 64) == []
    # the comb has the 4-lane shape only
    try:
        for lanes in (8, 16):
            gpu_ctx.set_modexp_group(lanes)
            with pytest.raises(_native.FsdkrError) as e:
                _run(gpu_ctx, keys, inst[:3], 64, 8, 72)
            assert e.value.code == _native.FSDKR_E_ARG
        gpu_ctx.set_modexp_group(4)
        assert _run(gpu_ctx, keys, inst[:17], 64, 8, 72) == want[:17]
    finally:
        gpu_ctx.set_modexp_group(0)
