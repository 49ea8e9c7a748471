"""GPU checks of the constant-time chains on structured moduli: Bob's response
(fsdkr_mta_respond: mta_tail_ct_kernel and the composed path, modulo N^2) and the
two-base comb (fsdkr_pedersen_commit_ct: commit_ct_kernel, modulo N~) against
Python's pow bit for bit.  tests/test_mta_respond_gpu.py and
tests/test_commit_ct_gpu.py run device-generated random keys only; these moduli are
the carry and final-subtraction cases of the 29-bit Montgomery rows (carry_exact,
sub_if_ge, the quotient-scaled chain modulo N' = N (-N^-1 mod 2^29)):

  2^2048 - 1            every limb all ones
  2^2047 + 1            the top bit and bit 0 alone
  2^2048 - 2^29 + 1     lowest digit 1: the quotient digit -N^-1 is 2^29 - 1
  2^2047 + 2^29 - 1     lowest digit all ones: the quotient digit is 1
  2^2047 + 2^1024 + 1   long runs of zero digits
  2^2030 - 1            70 digits of 2^29 - 1: the largest value below 2^2048 whose
                        29-bit digits are all 2^29 - 1 (a 71st would pass 2^2048)
  2^1024 + 1, 2^2017 - 1, 3     short moduli (the fused chain's head has no bit of
                        N = 3 or of its low 256 bits to run)

and, in the 3072-bit class, 2^3072 - 1 and 2^3071 + 1 in one call.  The operands
are the edge cycles of the two neighbouring files, so that every modulus meets
every edge of b (and every edge exponent of the comb)."""
import pytest

from oracle.rng import Rng
from test_commit_ct_gpu import _instances as commit_instances
from test_mta_respond_gpu import _instances as respond_instances

gpu = pytest.mark.gpu

MODULI_64 = [
    (1 << 2048) - 1,
    (1 << 2047) + 1,
    (1 << 2048) - (1 << 29) + 1,
    (1 << 2047) + (1 << 29) - 1,
    (1 << 2047) + (1 << 1024) + 1,
    (1 << 2030) - 1,
    (1 << 1024) + 1,
    (1 << 2017) - 1,
    3,
]
MODULI_96 = [(1 << 3072) - 1, (1 << 3071) + 1]
ROWS_96 = MODULI_96 + MODULI_96[:1]      # the key rows of the 3072-bit response call
M29 = (1 << 29) - 1


def test_the_moduli_are_what_they_are_named():
    assert all(n & 1 for n in MODULI_64 + MODULI_96)
    assert all(n.bit_length() <= 2048 for n in MODULI_64) and all(3071 < n.bit_length() <= 3072 for n in MODULI_96)
    q = [(-pow(n, -1, 1 << 29)) % (1 << 29) for n in MODULI_64]   # the Montgomery quotient digit
    assert q[2] == M29 and MODULI_64[2] & M29 == 1 and q[3] == 1 and MODULI_64[3] & M29 == M29
    n = MODULI_64[5]
    assert all((n >> (29 * j)) & M29 == M29 for j in range(70)) and n >> (29 * 70) == 0
    assert n + (M29 << (29 * 70)) >= 1 << 2048                     # a 71st such digit does not fit
    digits = [(MODULI_64[4] >> (29 * j)) & M29 for j in range(71)]
    assert sum(1 for d in digits if d == 0) == 68


# ---- fsdkr_mta_respond --------------------------------------------------------------
def respond_want(ns, inst):
    """a^b (1 + beta' N) r^N mod N^2 by pow; r^N once per (r, N): r = 1 and r = N - 1 recur."""
    rn, out = {}, []
    for a, b, bp, r, m in inst:
        N = ns[m]
        if (r, N) not in rn:
            rn[(r, N)] = pow(r, N, N * N)
        out.append(pow(a, b, N * N) * (1 + bp * N) * rn[(r, N)] % (N * N))
    return out


@pytest.fixture(scope="module")
def respond64():
    """90 responses over the nine moduli interleaved: every modulus meets every edge of
    b, and a in {0, 1, N^2 - 1, N, random}, r in {1, N - 1, random}, beta' in {0, 1,
    N - 1, random} cycle against them."""
    inst = respond_instances(MODULI_64, 90, "structured-nl64")
    for m in range(len(MODULI_64)):
        assert {0, 1, 15, 16, (1 << 256) - 1, 0xF << 252} <= {b for _, b, _, _, k in inst if k == m}
    return inst, respond_want(MODULI_64, inst)


@pytest.fixture(scope="module")
def respond96():
    """27 responses over three key rows (2^3072 - 1 twice: with three rows the cycle of b
    brings all nine edges to every row within 27 instances)."""
    inst = respond_instances(ROWS_96, 27, "structured-nl96")
    for m in range(len(ROWS_96)):
        assert {0, 1, 15, 16, (1 << 256) - 1, 0xF << 252} <= {b for _, b, _, _, k in inst if k == m}
    return inst, respond_want(ROWS_96, inst)


def _respond(ctx, ns, inst, nl, fused):
    A, B, BP, R, I = (list(x) for x in zip(*inst))
    return ctx.mta_respond(A, B, BP, R, ns, I, nl, fused=fused)


def _mismatches(got, want, inst, key_col):
    return [(j, inst[j][key_col]) for j, (g, w) in enumerate(zip(got, want)) if g != w]


@gpu
@pytest.mark.parametrize("fused", [True, False])
def test_respond_2048_structured(gpu_ctx, respond64, fused):
    inst, want = respond64
    got = _respond(gpu_ctx, MODULI_64, inst, 64, fused)
    assert len(got) == len(want) and _mismatches(got, want, inst, 4) == []   # (instance, modulus)


@gpu
@pytest.mark.parametrize("fused", [True, False])
def test_respond_3072_structured(gpu_ctx, respond96, fused):
    inst, want = respond96
    got = _respond(gpu_ctx, ROWS_96, inst, 96, fused)
    assert len(got) == len(want) and _mismatches(got, want, inst, 4) == []


# ---- fsdkr_pedersen_commit_ct -------------------------------------------------------
def _keys(moduli, tag):
    """(N~, h1, h2) per modulus: the bases cycle through 1, N~ - 1, 2 and a random value
    below N~, h2 one step ahead of h1 and another after four moduli."""
    rng = Rng(("structured-bases", tag))
    keys = []
    for m, nt in enumerate(moduli):
        pick = [1, nt - 1, 2, rng.sample_below(nt)]
        keys.append((nt, pick[m % 4], pick[(m + 1 + m // 4) % 4]))
    assert all(0 <= h < nt for nt, h1, h2 in keys for h in (h1, h2))
    return keys


def _commit_want(keys, inst):
    return [pow(keys[k][1], x, keys[k][0]) * pow(keys[k][2], y, keys[k][0]) % keys[k][0] for x, y, k in inst]


@pytest.fixture(scope="module")
def commit64():
    keys = _keys(MODULI_64, "nl64")
    made = {}
    for widths in ((8, 72), (24, 88)):
        inst = commit_instances(len(keys), 70, widths[0], widths[1], "structured-nl64")
        made[widths] = (inst, _commit_want(keys, inst))
    return keys, made


@gpu
@pytest.mark.parametrize("count", [17, 70])
@pytest.mark.parametrize("widths", [(8, 72), (24, 88)])
def test_commit_2048_structured(gpu_ctx, commit64, widths, count):
    keys, made = commit64
    inst, want = made[widths]
    X, Y, I = (list(v) for v in zip(*inst[:count]))
    got = gpu_ctx.pedersen_commit(X, Y, keys, I, 64, xl=widths[0], yl=widths[1])
    assert len(got) == count and _mismatches(got, want[:count], inst, 2) == []


@gpu
def test_commit_3072_structured(gpu_ctx):
    keys = _keys(MODULI_96, "nl96")
    inst = commit_instances(len(keys), 17, 24, 120, "structured-nl96")
    want = _commit_want(keys, inst)
    X, Y, I = (list(v) for v in zip(*inst))
    got = gpu_ctx.pedersen_commit(X, Y, keys, I, 96, xl=24, yl=120)
    assert len(got) == len(want) and _mismatches(got, want, inst, 2) == []
