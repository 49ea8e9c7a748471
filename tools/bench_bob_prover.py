"""Bob's MtA prover on the constant-time entries against the composed paths, in one
process on the same inputs:

  (a) fsdkr_bob_commit_v (ONE chain of bits(N) squarings per v: the
      sliding-window head of beta^N, then the 768-squaring constant-time joint tail)
      against fsdkr_bob_commit_v_unfused (a_enc^alpha through the regular-access
      modexp, beta^N as fsdkr_paillier_encrypt runs it, one prod3), `--count`
      instances under one key;
  (b) fsdkr.mta.generate_bob(fused=True) (one pedersen_commit call of 4 n comb
      instances, one bob_commit_v call) against fused=False (eight regular-access
      modexps mod N~ and one mod N^2 per proof, host products), `--count` proofs under
      one key and `--keys` proofs under `--keys` keys; wall time of the whole Python
      call, draws and packing included (the same for both paths).

`--bits 3072` runs the 6144-bit chain of (a): both width classes have the fused
shape, and (b) differs by it and by the comb.  The moduli are random odd values of full width (the
device's work does not depend on their factors); the batch of (a) is `--distinct`
instances repeated.  Both paths must agree (with pow for (a), with each other for
(b)) before anything is timed.  Per path: `--warmup` calls, then `--reps` timed calls,
interleaved A/B per repeat; reported: the median, the spread (max - min), and for
(a) the HIP-event time of the launches by kind.  One JSON line per measurement.

  python tools/bench_bob_prover.py
  python tools/bench_bob_prover.py --bits 3072"""
import argparse
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

from fsdkr import Context, mta  # noqa: E402
from fsdkr._native import _ptr, ints_to_limbs, limbs_to_ints  # noqa: E402
from fsdkr.types import DLogStatement  # noqa: E402
from oracle.paillier import EncryptionKey  # noqa: E402
from oracle.rng import Rng  # noqa: E402

EVENTS = ("modexp", "bob_v_tail_ct", "binom_ct", "prod3")


def odd(rng, bits):
    return rng.bits(bits) | (1 << (bits - 1)) | 1


def build_v(count, distinct, bits):
    rng = Rng(("bench-bob-v", bits))
    N = odd(rng, bits)
    NN, nl = N * N, bits // 32
    ex = [(rng.sample_below(NN), rng.bits(768), rng.sample_below(N), rng.sample_below(N)) for _ in range(distinct)]
    want = [pow(a, al, NN) * (1 + ga * N) * pow(be, N, NN) % NN for a, al, ga, be in ex]
    k = [i % distinct for i in range(count)]
    arrays = [ints_to_limbs([ex[i][f] for i in k], w) for f, w in ((0, 2 * nl), (1, 24), (2, nl), (3, nl))]
    arrays += [np.zeros(count, dtype=np.uint32), ints_to_limbs([N], nl)]
    return nl, arrays, [want[i] for i in k]


def call_v(ctx, nl, count, arrays, out, fused):
    A, Al, Ga, Be, I, Nn = arrays
    fn = ctx._lib.fsdkr_bob_commit_v if fused else ctx._lib.fsdkr_bob_commit_v_unfused
    ctx.check(fn(ctx.handle, nl, count, _ptr(A), _ptr(Al), _ptr(Ga), _ptr(Be), _ptr(I), _ptr(Nn), 1, _ptr(out)))


def spread(v):
    return max(v) - min(v)


def bench_v(a):
    wall_ctx, ev_ctx = Context(), Context(timing=True)
    nl, arrays, want = build_v(a.count, a.distinct, a.bits)
    out = np.zeros((a.count, 2 * nl), dtype=np.uint32)
    wall = {True: [], False: []}
    for fused in (True, False):
        for _ in range(a.warmup):
            out[:] = 0
            call_v(wall_ctx, nl, a.count, arrays, out, fused)
            assert limbs_to_ints(out) == want
    for _ in range(a.reps):
        for fused in (True, False):
            t0 = time.perf_counter()
            call_v(wall_ctx, nl, a.count, arrays, out, fused)   # returns after the stream's synchronise
            wall[fused].append(time.perf_counter() - t0)
    ev = {}
    for fused in (True, False):
        call_v(ev_ctx, nl, a.count, arrays, out, fused)
        ev_ctx.kernel_time_reset()
        for _ in range(a.reps):
            call_v(ev_ctx, nl, a.count, arrays, out, fused)
        ev[fused] = {k: ev_ctx.kernel_time(k)[0] / a.reps for k in EVENTS}
    wf, wu = statistics.median(wall[True]), statistics.median(wall[False])
    sf, su = spread(wall[True]), spread(wall[False])
    print(json.dumps({
        "what": "bob_commit_v", "count": a.count, "bits": a.bits, "reps": a.reps,
        "fused": {"wall_ms": wf * 1e3, "per_s": a.count / wf, "spread_ms": sf * 1e3, "event_ms": ev[True]},
        "unfused": {"wall_ms": wu * 1e3, "per_s": a.count / wu, "spread_ms": su * 1e3, "event_ms": ev[False]},
        "wall_ratio_fused_over_unfused": wf / wu,
        "event_ratio_fused_over_unfused": sum(ev[True].values()) / sum(ev[False].values()),
        "difference_exceeds_both_spreads": bool(abs(wu - wf) > su + sf),
    }), flush=True)
    wall_ctx.close()
    ev_ctx.close()


def build_items(proofs, n_keys, bits):
    rng = Rng(("bench-bob-prover", bits, n_keys))
    keys = []
    for _ in range(n_keys):
        ek = EncryptionKey.from_n(odd(rng, bits))
        nt = odd(rng, bits)
        h1 = pow(rng.sample_below(nt), 2, nt)
        keys.append((ek, DLogStatement(nt, h1, pow(h1, rng.sample_below(nt), nt))))
    items = []
    for k in range(proofs):
        ek, st = keys[k % n_keys]
        items.append((rng.sample_below(ek.nn), rng.sample_below(ek.nn), rng.bits(256), rng.sample_below(ek.n), ek, st,
                      rng.sample_below(ek.n)))
    return items


def bench_prover(a, proofs, n_keys):
    ctx = Context()
    items = build_items(proofs, n_keys, a.bits)
    seed = ("bench-bob-prover-draws", proofs, n_keys)
    wall = {True: [], False: []}
    first = {}
    for fused in (True, False):
        for _ in range(a.warmup):
            first[fused] = mta.generate_bob(items, Rng(seed), ctx=ctx, fused=fused)
    assert first[True] == first[False]
    for _ in range(a.reps):
        for fused in (True, False):
            t0 = time.perf_counter()
            mta.generate_bob(items, Rng(seed), ctx=ctx, fused=fused)
            wall[fused].append(time.perf_counter() - t0)
    wf, wu = statistics.median(wall[True]), statistics.median(wall[False])
    sf, su = spread(wall[True]), spread(wall[False])
    print(json.dumps({
        "what": "generate_bob", "proofs": proofs, "keys": n_keys, "bits": a.bits, "reps": a.reps,
        "fused": {"wall_ms": wf * 1e3, "per_s": proofs / wf, "spread_ms": sf * 1e3},
        "unfused": {"wall_ms": wu * 1e3, "per_s": proofs / wu, "spread_ms": su * 1e3},
        "wall_ratio_fused_over_unfused": wf / wu,
        "difference_exceeds_both_spreads": bool(abs(wu - wf) > su + sf),
    }), flush=True)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=4096, help="instances of (a), proofs of (b) under one key")
    ap.add_argument("--keys", type=int, default=64, help="(b): that many proofs under that many keys")
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bits", type=int, choices=(2048, 3072), default=2048, help="size of N and N~")
    ap.add_argument("--only", choices=("v", "prover"), default=None)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("at least 5 timed runs per path")
    if a.only != "prover":
        bench_v(a)
    if a.only != "v":
        bench_prover(a, a.count, 1)
        bench_prover(a, a.keys, a.keys)


if __name__ == "__main__":
    main()
