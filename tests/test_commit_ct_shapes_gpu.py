"""GPU checks of the constant-time two-base comb (fsdkr_pedersen_commit_ct,
csrc/comb_ct.hip) at the launch shapes of production-size batches, which
tests/test_commit_ct_gpu.py does not reach: the small column counts b <= 8, b = 1
and (3072 bits) b = 16 with their many table blocks, column counts that do not
divide the exponents' lengths (the comb's top block is partly padding past the top
limb), and the 64-instance block with its padding of every key's run.  The rows are
those of tests/commit_ct_shapes.py; tests/test_commit_geom.py shows on the CPU that
the compiled geometry puts each in its class.  Every output is compared with
Python's pow bit for bit.

The geometry depends on counts and widths alone, so a row's count is reached by
repeating a few distinct instances (the edge values of test_commit_ct_gpu.py), each
computed by pow once.  The moduli are seeded random odd numbers of full width (the
comb needs no more of N~ than that it is odd); one key has h1 = 0, h2 = 1."""
import ctypes

import pytest

import commit_ct_shapes as shapes
from oracle.rng import Rng
from test_commit_ct_gpu import _instances

pytestmark = pytest.mark.gpu


def _odd(rng, bits):
    return rng.bits(bits) | (1 << (bits - 1)) | 1


@pytest.fixture(scope="module")
def keysets():
    """Per width class, four keys (N~, h1, h2): random bases; h1 = 1, h2 = N~ - 1;
    h1 = 0, h2 = 1 (the value is 1 where x = 0, else 0); random bases."""
    rng = Rng("commit-ct-shapes-keys")
    out = {}
    for nl in (64, 96):
        nts = [_odd(rng, 32 * nl) for _ in range(4)]
        out[nl] = [(nts[0], rng.sample_below(nts[0]), rng.sample_below(nts[0])), (nts[1], 1, nts[1] - 1),
                   (nts[2], 0, 1), (nts[3], rng.sample_below(nts[3]), rng.sample_below(nts[3]))]
    return out


def _free_device_memory():
    """hipMemGetInfo's free bytes, from the HIP runtime the library has loaded into this process."""
    with open("/proc/self/maps") as f:
        paths = {ln.split()[-1] for ln in f if "libamdhip64" in ln}
    assert paths, "the HIP runtime is not loaded"
    hip = ctypes.CDLL(sorted(paths)[0])
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def _row_keys(keysets, row):
    ks = keysets[row.nl]
    if len(row.per) == 1:
        return [ks[0]]
    if len(row.per) == 2:
        return [ks[0], ks[2]]
    return ks[:len(row.per)]


def _key_order(per):
    """The keys of the call's instances, interleaved instance by instance while a key has any left."""
    left, seq = list(per), []
    while any(left):
        for k in range(len(left)):
            if left[k]:
                seq.append(k)
                left[k] -= 1
    return seq


def _distinct(row):
    """The row's distinct (x, y): test_commit_ct_gpu's edge cycles; a single instance has every bit of both set."""
    if row.distinct == 1:
        return [((1 << (32 * row.xl)) - 1, (1 << (32 * row.yl)) - 1)]
    return [(x, y) for x, y, _ in _instances(1, row.distinct, row.xl, row.yl, ("shapes", row.name))]


@pytest.mark.parametrize("row", shapes.ROWS, ids=[r.name for r in shapes.ROWS])
def test_commit_shape_matches_pow(gpu_ctx, keysets, row):
    keys = _row_keys(keysets, row)
    # the device's table cap (a quarter of the free memory, at most 24 GiB) cannot bind:
    # every key's tables are within the budget, so b is the one the CPU test saw
    assert len(keys) * shapes.KEY_BUDGET <= min(_free_device_memory() // 4, 24 << 30)
    pairs = _distinct(row)
    if row.want == "padded":
        # the top real bit sits right under the padding: all ones, and the top bit alone
        for col, limbs in ((0, row.xl), (1, row.yl)):
            vals = {p[col] for p in pairs}
            assert (1 << (32 * limbs)) - 1 in vals and (row.distinct == 1 or 1 << (32 * limbs - 1) in vals)
    order = _key_order(row.per)
    assert [order.count(k) for k in range(len(row.per))] == list(row.per)
    inst = [pairs[j % len(pairs)] + (k,) for j, k in enumerate(order)]
    ref = {}
    for x, y, k in set(inst):
        nt, h1, h2 = keys[k]
        ref[(x, y, k)] = pow(h1, x, nt) * pow(h2, y, nt) % nt
    assert len(ref) <= row.distinct * len(row.per)
    X, Y, I = (list(v) for v in zip(*inst))
    got = gpu_ctx.pedersen_commit(X, Y, keys, I, row.nl, xl=row.xl, yl=row.yl)
    want = [ref[i] for i in inst]
    bad = [j for j, (g, w) in enumerate(zip(got, want)) if g != w]
    assert len(got) == len(want) and not bad, (row.name, len(bad), bad[:8])


def test_zero_base_key(gpu_ctx, keysets):
    """h1 = 0, h2 = 1 on its own and beside a random key: 1 where x = 0, 0 otherwise."""
    ks = keysets[64]
    inst = _instances(2, 40, 8, 72, "shapes-zero-base")
    keys = [ks[2], ks[0]]
    X, Y, I = (list(v) for v in zip(*inst))
    got = gpu_ctx.pedersen_commit(X, Y, keys, I, 64, xl=8, yl=72)
    for (x, y, k), g in zip(inst, got):
        nt, h1, h2 = keys[k]
        assert g == pow(h1, x, nt) * pow(h2, y, nt) % nt
        if k == 0:
            assert g == (1 if x == 0 else 0)
    assert {g for (x, y, k), g in zip(inst, got) if k == 0} == {0, 1}
