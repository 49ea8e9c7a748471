"""CPU checks of the one-call MtA provers (fsdkr.mta.generate_bob / generate_alice
with one_call=True, fsdkr_bob_prove / fsdkr_alice_prove):
  - the output-width rule limbs(e x + y) = max(xl + 8, yl) + 1 against the extreme
    values of every row in Python integers: 25 and 33 limbs for s1, nl + 17 for t1,
    nl + 25 for s2 and t2, in both width classes, as the Python binding and the C
    header fsdkr/csrc/prove_geom.hpp state them;
  - the packing header under AddressSanitizer and UBSan: a stand-alone program
    (tests/native/prove_geom_host.cpp) built with g++ alone and run on its own;
  - the ValueErrors of one_call=True, raised before any device call: a stub context
    fails on every call."""
import os
import subprocess

import pytest

from oracle.paillier import EncryptionKey
from oracle.rng import Rng
from oracle.zk_paillier import DLogStatement

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_MAX = (1 << 256) - 1


def _ones(limbs):
    return (1 << (32 * limbs)) - 1


def _limbs(v):
    return max(1, (v.bit_length() + 31) // 32)


@pytest.mark.parametrize("nl", [64, 96])
def test_output_widths_hold_the_extreme_rows(nl):
    from fsdkr import _native
    win, wout = _native.bob_prove_widths(nl)
    assert (wout["s1"], wout["s2"], wout["t1"], wout["t2"]) == (25, nl + 25, nl + 17, nl + 25)
    for out, x, y in (("s1", "b", "alpha"), ("s2", "ro", "ro_prim"), ("t1", "beta_prim", "gamma"), ("t2", "sigma", "tau")):
        assert wout[out] == max(win[x] + 8, win[y]) + 1
        top = E_MAX * _ones(win[x]) + _ones(win[y])
        # the extreme value fits its row, and (where the product decides the width) needs its top limb's neighbour
        assert _limbs(top) <= wout[out]
        assert _limbs(top) >= wout[out] - 1
    ain, aout = _native.alice_prove_widths(nl)
    assert (aout["s1"], aout["s2"]) == (33, nl + 25)
    for out, x, y in (("s1", "a", "alpha"), ("s2", "ro", "gamma")):
        assert aout[out] == max(ain[x] + 8, ain[y]) + 1
        assert _limbs(E_MAX * _ones(ain[x]) + _ones(ain[y])) <= aout[out]
    # equal widths of e x and y: the carry can reach the extra limb
    assert _limbs(E_MAX * _ones(16)) == 24 and _limbs(E_MAX * _ones(16) + _ones(24)) == 25


@pytest.fixture(scope="module")
def host_prog(tmp_path_factory):
    out = tmp_path_factory.mktemp("pg") / "prove_geom_host"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(REPO, "fs-dkr_amd", "csrc"),
                    os.path.join(REPO, "tests", "native", "prove_geom_host.cpp"), "-o", str(out)], check=True)
    return str(out)


@pytest.mark.parametrize("count", [1, 5, 64])
def test_packing_header_under_sanitizers(host_prog, count):
    from fsdkr import _native
    r = subprocess.run([host_prog, str(count)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.split("\n")
    assert lines[-2] == "ok"
    want = []
    for nl in (64, 96):
        b, a = _native.bob_prove_widths(nl)[1], _native.alice_prove_widths(nl)[1]
        want.append(f"bob {nl} {nl + 16} {nl + 24} {b['s1']} {b['s2']} {b['t1']} {b['t2']}")
        want.append(f"alice {nl} 24 {nl + 24} {a['s1']} {a['s2']}")
    assert lines[:4] == want


class _NoDevice:
    """Any attribute is a call that fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"device call {name} before the argument checks")


@pytest.fixture(scope="module")
def item():
    # small odd moduli: nothing here reaches a device
    ek = EncryptionKey.from_n((1 << 521) - 1)
    st = DLogStatement((1 << 607) - 1, 3, 5)
    return (12345, 67890, 7, 11, ek, st, 13)


@pytest.mark.parametrize("change", ["check", "b_neg", "b_wide", "beta_prim_neg", "beta_prim_N", "a_enc_NN", "a_enc_neg"])
def test_one_call_value_errors_before_any_device_call(item, change):
    from fsdkr import mta
    a_enc, m, b, bp, ek, st, r = item
    kw = dict(one_call=True)
    if change == "check":
        kw["check"] = True
    b = {"b_neg": -1, "b_wide": 1 << 256}.get(change, b)
    bp = {"beta_prim_neg": -1, "beta_prim_N": ek.n}.get(change, bp)
    a_enc = {"a_enc_NN": ek.nn, "a_enc_neg": -1}.get(change, a_enc)
    rng = Rng("no-draws")
    with pytest.raises(ValueError):
        mta.generate_bob([(a_enc, m, b, bp, ek, st, r)], rng, ctx=_NoDevice(), **kw)
    # refused before the draws: the stream is untouched
    assert rng.sample_below(1 << 64) == Rng("no-draws").sample_below(1 << 64)


def test_one_call_alice_value_error_before_any_device_call(item):
    from fsdkr import mta
    _, cipher, _, _, ek, st, r = item
    with pytest.raises(ValueError):
        mta.generate_alice([(1 << 768, cipher, ek, st, r)], Rng("x"), ctx=_NoDevice(), one_call=True)
    assert mta.generate_alice([], Rng("x"), ctx=_NoDevice(), one_call=True) == []
    assert mta.generate_bob([], Rng("x"), ctx=_NoDevice(), one_call=True) == []
