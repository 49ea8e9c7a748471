"""The one-call MtA provers (fsdkr_bob_prove, fsdkr_alice_prove) against the paths of
the same build that compose the prover from component entries, in one process on the
same inputs:

  (1) fsdkr.mta.generate_bob(one_call=True) against generate_bob(fused=True): wall time
      of the whole Python call (draws, packing, unpacking included), `--count` proofs
      under one key and `--keys` proofs under `--keys` keys;
  (2) the same for generate_alice(one_call=True) against generate_alice();
  (3) fsdkr_bob_prove alone, from packed limbs to packed proofs (what a C or Rust
      caller sees), against the sum of the component entries fused=True issues from
      packed limbs: fsdkr_pedersen_commit_ct (4 n instances), fsdkr_bob_commit_v and
      fsdkr_modexp_batch (r^e, the exponents being the proofs' challenges);
  (4) HIP-event times of the challenge launch, the r^e launch and the response
      launches inside one fsdkr_bob_prove call (Context.kernel_time).

The moduli are random odd values of full width (the device's work does not depend on
their factors).  Both paths must agree before anything is timed.  Per path: `--warmup`
calls, then `--reps` timed calls, interleaved A/B per repeat; reported: the median and
the spread (max - min), and whether the difference exceeds the two spreads combined.
One JSON line per measurement.

  python tools/bench_mta_prove.py
  python tools/bench_mta_prove.py --bits 3072"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "fs-dkr_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from fsdkr import Context, _native, mta  # noqa: E402
from fsdkr._native import _ptr, ints_to_limbs, limbs_to_ints  # noqa: E402
from fsdkr.refresh import Q  # noqa: E402
from fsdkr.types import DLogStatement  # noqa: E402
from oracle.paillier import EncryptionKey  # noqa: E402
from oracle.rng import Rng  # noqa: E402

EVENTS = ("prove_challenge", "prove_re", "prove_resp", "prod3", "commit_ct", "bob_v_tail_ct", "modexp")


def odd(rng, bits):
    return rng.bits(bits) | (1 << (bits - 1)) | 1


def spread(v):
    return max(v) - min(v)


def build_keys(rng, n_keys, bits):
    keys = []
    for _ in range(n_keys):
        ek = EncryptionKey.from_n(odd(rng, bits))
        nt = odd(rng, bits)
        h1 = pow(rng.sample_below(nt), 2, nt)
        keys.append((ek, DLogStatement(nt, h1, pow(h1, rng.sample_below(nt), nt))))
    return keys


def bob_items(proofs, n_keys, bits):
    rng = Rng(("bench-mta-prove-bob", bits, n_keys))
    keys = build_keys(rng, n_keys, bits)
    items = []
    for k in range(proofs):
        ek, st = keys[k % n_keys]
        items.append((rng.sample_below(ek.nn), rng.sample_below(ek.nn), rng.bits(256), rng.sample_below(ek.n), ek, st,
                      rng.sample_below(ek.n)))
    return items


def alice_items(proofs, n_keys, bits):
    rng = Rng(("bench-mta-prove-alice", bits, n_keys))
    keys = build_keys(rng, n_keys, bits)
    items = []
    for k in range(proofs):
        ek, st = keys[k % n_keys]
        items.append((rng.sample_below(Q), rng.sample_below(ek.nn), ek, st, rng.sample_below(ek.n)))
    return items


def report(what, extra, wall, names):
    a, b = names
    ma, mb = statistics.median(wall[a]), statistics.median(wall[b])
    sa, sb = spread(wall[a]), spread(wall[b])
    print(json.dumps(dict(extra, what=what,
                          **{a: {"wall_ms": ma * 1e3, "spread_ms": sa * 1e3}, b: {"wall_ms": mb * 1e3, "spread_ms": sb * 1e3}},
                          wall_ratio=ma / mb, difference_exceeds_both_spreads=bool(abs(ma - mb) > sa + sb))), flush=True)


def bench_python(a, who, proofs, n_keys):
    ctx = Context()
    if who == "bob":
        items, other = bob_items(proofs, n_keys, a.bits), "fused"
        run = {"one_call": lambda r: mta.generate_bob(items, r, ctx=ctx, one_call=True),
               "fused": lambda r: mta.generate_bob(items, r, ctx=ctx, fused=True)}
    else:
        items, other = alice_items(proofs, n_keys, a.bits), "default"
        run = {"one_call": lambda r: mta.generate_alice(items, r, ctx=ctx, one_call=True),
               "default": lambda r: mta.generate_alice(items, r, ctx=ctx)}
    seed = ("bench-mta-prove-draws", who, proofs, n_keys)
    first, wall = {}, {k: [] for k in run}
    for k, f in run.items():
        for _ in range(a.warmup):
            first[k] = f(Rng(seed))
    assert first["one_call"] == first[other]
    for _ in range(a.reps):
        for k, f in run.items():
            t0 = time.perf_counter()
            f(Rng(seed))
            wall[k].append(time.perf_counter() - t0)
    report(f"generate_{who}", dict(proofs=proofs, keys=n_keys, bits=a.bits, reps=a.reps), wall, ("one_call", other))
    ctx.close()


def bench_c_abi(a, proofs):
    """(3) and (4): packed limbs in, packed limbs out, one key."""
    nl = a.bits // 32
    rng = Rng(("bench-mta-prove-c", a.bits))
    N, Nt = odd(rng, a.bits), odd(rng, a.bits)
    h1 = pow(rng.sample_below(Nt), 2, Nt)
    h2 = pow(h1, rng.sample_below(Nt), Nt)
    win, wout = _native.bob_prove_widths(nl)
    dist = 8
    vals = {f: [rng.bits(32 * l - 1) for _ in range(dist)] for f, l in win.items()}
    for f in ("r", "beta", "beta_prim"):
        vals[f] = [rng.sample_below(N) for _ in range(dist)]
    vals["gamma_mod_n"] = [g % N for g in vals["gamma"]]
    a_enc, m = [rng.sample_below(N * N) for _ in range(dist)], [rng.sample_below(N * N) for _ in range(dist)]
    idx = [i % dist for i in range(proofs)]
    S = {f: ints_to_limbs([vals[f][i] for i in idx], win[f]) for f in win}
    A, M = ints_to_limbs([a_enc[i] for i in idx], 2 * nl), ints_to_limbs([m[i] for i in idx], 2 * nl)
    K = [ints_to_limbs([v], nl) for v in (N, Nt, h1, h2)]
    I = np.zeros(proofs, dtype=np.uint32)
    O = {f: np.zeros((proofs, w), dtype=np.uint32) for f, w in wout.items()}
    b, o = _native.BobProveC(), _native.BobProofsC()
    b.count, b.n_keys, b.nl = proofs, 1, nl
    b.N, b.Ntilde, b.h1, b.h2, b.key_idx, b.a_enc, b.mta = [_ptr(x) for x in K + [I, A, M]]
    for f in win:
        setattr(b, f, _ptr(S[f]))
    for f in wout:
        setattr(o, f, _ptr(O[f]))
    # the component entries' operands, packed once: the comb's interleaved rows, v's rows, r^e's
    xl, yl = nl + 16, nl + 24
    X, Y = np.zeros((4 * proofs, xl), dtype=np.uint32), np.zeros((4 * proofs, yl), dtype=np.uint32)
    for s, (fx, fy) in enumerate((("b", "ro"), ("alpha", "ro_prim"), ("beta_prim", "sigma"), ("gamma", "tau"))):
        X[s::4, :win[fx]] = S[fx]
        Y[s::4, :win[fy]] = S[fy]
    I4 = np.zeros(4 * proofs, dtype=np.uint32)
    CM, V, RE = (np.zeros((4 * proofs, nl), dtype=np.uint32), np.zeros((proofs, 2 * nl), dtype=np.uint32),
                 np.zeros((proofs, nl), dtype=np.uint32))

    def one(ctx):
        ctx.check(ctx._lib.fsdkr_bob_prove(ctx.handle, ctypes.byref(b), ctypes.byref(o)))

    def parts(ctx):
        L, h = ctx._lib, ctx.handle
        ctx.check(L.fsdkr_pedersen_commit_ct(h, nl, 4 * proofs, _ptr(X), xl, _ptr(Y), yl, _ptr(I4), _ptr(K[1]), _ptr(K[2]),
                                             _ptr(K[3]), 1, _ptr(CM)))
        ctx.check(L.fsdkr_bob_commit_v(h, nl, proofs, _ptr(A), _ptr(S["alpha"]), _ptr(S["gamma_mod_n"]), _ptr(S["beta"]),
                                       _ptr(I), _ptr(K[0]), 1, _ptr(V)))
        ctx.check(L.fsdkr_modexp_batch(h, nl, proofs, _ptr(S["r"]), _ptr(O["e"]), 8, _ptr(I), _ptr(K[0]), 1, _ptr(RE)))

    ctx = Context()
    run, wall = {"bob_prove": one, "components": parts}, {"bob_prove": [], "components": []}
    for _ in range(a.warmup):
        one(ctx)      # fills O["e"], the exponents of the components' r^e
        parts(ctx)
    es, ss, res = limbs_to_ints(O["e"][:dist]), limbs_to_ints(O["s"][:dist]), limbs_to_ints(RE[:dist])
    assert limbs_to_ints(CM[0:4 * dist:4]) == limbs_to_ints(O["z"][:dist])
    assert [x * be % N for x, be in zip(res, vals["beta"])] == ss
    assert limbs_to_ints(O["s1"][:dist]) == [e * x + y for e, x, y in zip(es, vals["b"], vals["alpha"])]
    for _ in range(a.reps):
        for k, f in run.items():
            t0 = time.perf_counter()
            f(ctx)
            wall[k].append(time.perf_counter() - t0)
    report("fsdkr_bob_prove", dict(proofs=proofs, keys=1, bits=a.bits, reps=a.reps), wall, ("bob_prove", "components"))
    ctx.close()
    ev = Context(timing=True)
    one(ev)
    ev.kernel_time_reset()
    for _ in range(a.reps):
        one(ev)
    print(json.dumps({"what": "fsdkr_bob_prove events", "proofs": proofs, "bits": a.bits, "reps": a.reps,
                      "event_ms": {k: ev.kernel_time(k)[0] / a.reps for k in EVENTS}}), flush=True)
    ev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=4096, help="proofs under one key")
    ap.add_argument("--keys", type=int, default=64, help="that many proofs under that many keys")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bits", type=int, choices=(2048, 3072), default=2048, help="size of N and N~")
    ap.add_argument("--only", choices=("bob", "alice", "c"), default=None)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("at least 5 timed runs per path")
    for who in ("bob", "alice"):
        if a.only in (None, who):
            bench_python(a, who, a.count, 1)
            bench_python(a, who, a.keys, a.keys)
    if a.only in (None, "c"):
        bench_c_abi(a, a.count)


if __name__ == "__main__":
    main()
