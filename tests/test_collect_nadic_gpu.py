"""collect() with GA's head in half-width N-adic form (the default for 2048-bit
receivers) against the full-width head (FSDKR_CFG_GA_FULLWIDTH) and the oracle:
the 2048-bit golden transcript (t = 1, n = 3) and one synthetic n = 5, t = 2
batch, each clean, with a tampered PDL s2 and with a tampered Alice s (the two
bases of GA's chains).  Both settings must give the same verdict vector, first
error and LocalKey, equal to the oracle's."""
import copy
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import codec  # noqa: E402
import tamper  # noqa: E402

pytestmark = pytest.mark.gpu

KB = 2048
FIELDS = ("feldman", "pdl", "range", "ped", "ck")


def _run(ctx, msgs, lk, dk, fullwidth):
    """(verdict vector, first error, collect() outcome, LocalKey after) under one setting:
    the verdicts through prepare's own GA (no prestart), the outcome through
    refresh.collect (prestarted GA)"""
    from fsdkr import refresh
    from fsdkr._native import FSDKR_CFG_GA_FULLWIDTH
    from fsdkr.batch import CollectBatch
    old = ctx.set_flags((ctx.flags | FSDKR_CFG_GA_FULLWIDTH) if fullwidth else (ctx.flags & ~FSDKR_CFG_GA_FULLWIDTH))
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


def _check(ctx, msgs, lk, dk, spec, clean_key):
    """both settings agree with each other and with the oracle (tamper.expected for
    the tampered pair and the first error; clean_key: the oracle's LocalKey)"""
    R = n = len(msgs)
    m2, _ = tamper.inject(msgs, [], spec)
    pairs, mres, jres, first = tamper.expected(m2, [], lk, spec, KB)
    nad = _run(ctx, m2, lk, dk, False)
    full = _run(ctx, m2, lk, dk, True)
    for f in FIELDS:
        assert np.array_equal(nad[0][f], full[0][f]), f
    assert nad[1] == full[1] == first
    assert nad[2] == full[2] == first
    assert _key(nad[3]) == _key(full[3])
    for v in (nad, full):
        tamper.check_verdicts(type("V", (), {**v[0], "dlog": np.zeros(0, np.uint8)}), R, 0, n, pairs, mres, jres)
    if spec:
        assert first is not None and first[0] in ("PDLwSlackProof", "RangeProof")
    else:
        assert first is None and _key(nad[3])[:3] == clean_key[:3] and _key(nad[3])[3] == clean_key[3]


SPECS = ([], [("pdl_s2", 1, 2)], [("range_s", 2, 0)])


def test_golden_n3_nadic_vs_fullwidth(gpu_ctx):
    raw = codec.load_raw("transcript_t1_n3_kb2048.json.gz")
    cls = codec.product_classes()
    d = {k: codec.dec(raw[k], cls) for k in ("keys", "dks", "msgs", "joins", "expect")}
    assert raw["meta"]["key_bits"] == KB and not d["joins"]
    e = d["expect"][0]
    want = e["key_after"]   # frozen from the oracle's collect
    clean_key = (want["x_i"], want["y"], want["pk_vec"], want["paillier_n"])
    for spec in SPECS:
        _check(gpu_ctx, d["msgs"], d["keys"][e["party"]], d["dks"][e["party"]], spec, clean_key)


def test_synthetic_n5_t2_nadic_vs_fullwidth(gpu_ctx):
    from fsdkr import synth
    from oracle import protocol
    from oracle.rng import Rng
    msgs, joins, lk, dk = synth.synth_sessions(gpu_ctx, 1, n=5, t=2, seed=707, key_bits=KB)[0]
    assert not joins
    ko = copy.deepcopy(lk)
    protocol.collect(tamper.to_oracle(msgs), ko, dk, [], Rng("a8"), KB)
    for spec in ([], [("pdl_s2", 3, 1)], [("range_s", 0, 4)]):
        _check(gpu_ctx, msgs, lk, dk, spec, _key(ko))
