"""Bob's MtA response, responses/s: fsdkr_mta_respond (ONE chain of bits(N)
squarings per response: the sliding-window head of r^N, then the constant-time
joint tail that carries a_enc^b and takes 1 + beta' N at its exit)
against fsdkr_mta_respond_unfused (a_enc^b through the regular-access modexp, r^N
as fsdkr_paillier_encrypt runs it, one prod3), in one process, on the same packed
batch of `--count` responses under one key of `--bits` 2048 or 3072 (the 4096-bit
or the 6144-bit chain: both width classes have the fused shape).

The batch is `--distinct` exchanges (random a_enc, b, beta', r) repeated to
`--count`: the device's work per response does not depend on the values.  Both
paths must return pow's values for the distinct exchanges.  Per path: `--warmup`
calls, then `--reps` timed calls, interleaved A/B per repeat.  Reported per path:
the median wall time of the C call (host packing of descriptors, upload, kernels,
readback, the scrub of the secret buffers), the spread (max - min) of its timed
calls, and the HIP-event time of its launches by kind (a timing context).

  python tools/bench_mta_respond.py
  python tools/bench_mta_respond.py --bits 3072"""
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

from fsdkr import Context, keygen  # noqa: E402
from fsdkr._native import _ptr, ints_to_limbs, limbs_to_ints  # noqa: E402
from oracle.rng import Rng  # noqa: E402

EVENTS = ("modexp", "mta_tail_ct", "binom_ct", "prod3")


def build(ctx, count, distinct, bits):
    rng = Rng(("bench-mta-respond", bits))
    N = keygen.keypairs_with_modulus_size(ctx, rng, bits, 1)[0][0].n
    NN, nl = N * N, bits // 32
    ex = [(rng.sample_below(NN), rng.bits(256), rng.sample_below(N), rng.sample_below(N)) for _ in range(distinct)]
    want = [pow(a, b, NN) * (1 + bp * N) * pow(r, N, NN) % NN for a, b, bp, r in ex]
    k = [i % distinct for i in range(count)]
    arrays = [ints_to_limbs([ex[i][f] for i in k], w) for f, w in ((0, 2 * nl), (1, 8), (2, nl), (3, nl))]
    arrays += [np.zeros(count, dtype=np.uint32), ints_to_limbs([N], nl)]
    return nl, arrays, [want[i] for i in k]


def call(ctx, nl, count, arrays, out, fused):
    A, B, Bp, R, I, Nn = arrays
    fn = ctx._lib.fsdkr_mta_respond if fused else ctx._lib.fsdkr_mta_respond_unfused
    ctx.check(fn(ctx.handle, nl, count, _ptr(A), _ptr(B), _ptr(Bp), _ptr(R), _ptr(I), _ptr(Nn), 1, _ptr(out)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=4096)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bits", type=int, choices=(2048, 3072), default=2048, help="size of N")
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("at least 5 timed runs per path")
    wall_ctx, ev_ctx = Context(), Context(timing=True)
    nl, arrays, want = build(wall_ctx, a.count, a.distinct, a.bits)
    out = np.zeros((a.count, 2 * nl), dtype=np.uint32)
    wall = {True: [], False: []}
    for fused in (True, False):
        for _ in range(a.warmup):
            out[:] = 0
            call(wall_ctx, nl, a.count, arrays, out, fused)
            assert limbs_to_ints(out) == want
    for _ in range(a.reps):
        for fused in (True, False):
            t0 = time.perf_counter()
            call(wall_ctx, nl, a.count, arrays, out, fused)   # returns after the stream's synchronise
            wall[fused].append(time.perf_counter() - t0)
    ev = {}
    for fused in (True, False):
        call(ev_ctx, nl, a.count, arrays, out, fused)
        ev_ctx.kernel_time_reset()
        for _ in range(a.reps):
            call(ev_ctx, nl, a.count, arrays, out, fused)
        ev[fused] = {k: ev_ctx.kernel_time(k)[0] / a.reps for k in EVENTS}
    wf, wu = statistics.median(wall[True]), statistics.median(wall[False])
    sf, su = max(wall[True]) - min(wall[True]), max(wall[False]) - min(wall[False])
    print(json.dumps({
        "count": a.count, "bits": a.bits, "reps": a.reps,
        "fused": {"wall_ms": wf * 1e3, "responses_per_s": a.count / wf, "spread_ms": sf * 1e3, "event_ms": ev[True]},
        "unfused": {"wall_ms": wu * 1e3, "responses_per_s": a.count / wu, "spread_ms": su * 1e3, "event_ms": ev[False]},
        "wall_ratio_fused_over_unfused": wf / wu,
        "event_ratio_fused_over_unfused": sum(ev[True].values()) / sum(ev[False].values()),
        "fused_lower_by_more_than_unfused_spread": bool(wu - wf > su),
    }))


if __name__ == "__main__":
    main()
