"""Bob's range-proof verification, proofs/s: fsdkr_bob_verify (the mod-N^2 product
a_enc^s1 * s^N * mta^-e as ONE split chain with the three-base tail) against
fsdkr_bob_verify_unfused (the same pipeline with that product as three separate
chains of kernels that predate the tail: the keyed s^N, a_enc^s1, mta^e and its
inverse), in one process, on the same packed batch of one verifier key of
`--bits` 2048 (width class 64 limbs) or 3072 (96 limbs: the 6144-bit chain).

The batch is `--distinct` honest proofs from generate_bob (plain, or extended
with --ext) repeated to `--count`: the device's work per proof does not depend
on the proofs being distinct.  The last proof is tampered, so both paths must
return the same mixed verdicts.  Per path: `--warmup`
calls, then `--reps` timed calls, interleaved A/B per repeat.  Reported per path:
the median wall time of the C call (host pre-pass, upload, kernels, readback) and
the HIP-event time of its modexp launches (a timing context), and the ratios.

  python tools/bench_mta.py --count 4096
  python tools/bench_mta.py --count 4096 --bits 3072"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "fs-dkr_amd"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from fsdkr import Context, keygen, mta  # noqa: E402
from oracle.rng import Rng  # noqa: E402
import mta_oracle as mo  # noqa: E402
from oracle import secp256k1 as ec  # noqa: E402


def build(ctx, count, distinct, ext, bits=2048):
    rng = Rng(("bench-mta", ext) if bits == 2048 else ("bench-mta", ext, bits))
    (ek, _), (ekt, dkt) = keygen.keypairs_with_modulus_size(ctx, rng, bits, 2)
    st = mo.dlog_statement(ekt.n, dkt.p, dkt.q, rng)
    items = []
    for _ in range(distinct):
        a_enc, m, b, beta_prim, r = mo.mta_scenario(ek, rng)
        items.append((a_enc, m, b, beta_prim, ek, st, r))
    proofs = mta.generate_bob(items, rng, ctx=ctx, check=ext)
    k = [i % distinct for i in range(count)]
    pf = [proofs[i] for i in k]
    a_encs, mtas = [items[i][0] for i in k], [items[i][1] for i in k]
    X = [ec.mul(ec.G, it[2]) for it in items]
    mtas[-1] += 1   # one rejected proof
    pp = mta.prepass(pf, a_encs, mtas, [ek] * count, [st] * count, [X[i] for i in k] if ext else None)
    assert pp["nl"] == bits // 32
    batch, keep = mta._batch(pp, a_encs, mtas, pf, [X[i] for i in k] if ext else None)
    return batch, keep, [1] * (count - 1) + [0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=4096)
    ap.add_argument("--distinct", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ext", action="store_true", help="BobProofExt (adds the curve equation)")
    ap.add_argument("--bits", type=int, choices=(2048, 3072), default=2048, help="size of N and N~")
    a = ap.parse_args()
    wall_ctx, ev_ctx = Context(), Context(timing=True)
    batch, keep, want = build(wall_ctx, a.count, a.distinct, a.ext, a.bits)
    wall = {True: [], False: []}
    for fused in (True, False):
        for _ in range(a.warmup):
            assert list(wall_ctx.bob_verify(batch, a.count, fused=fused)) == want
    for _ in range(a.reps):
        for fused in (True, False):
            t0 = time.perf_counter()
            v = wall_ctx.bob_verify(batch, a.count, fused=fused)
            wall[fused].append(time.perf_counter() - t0)
            assert list(v) == want
    ev = {}
    for fused in (True, False):
        ev_ctx.bob_verify(batch, a.count, fused=fused)
        ev_ctx.kernel_time_reset()
        for _ in range(a.reps):
            ev_ctx.bob_verify(batch, a.count, fused=fused)
        ev[fused] = {k: ev_ctx.kernel_time(k)[0] / a.reps for k in ("modexp", "inverse", "bob_hash", "ec")}
    wf, wu = statistics.median(wall[True]), statistics.median(wall[False])
    print(json.dumps({
        "count": a.count, "bits": a.bits, "ext": a.ext, "reps": a.reps,
        "fused": {"wall_ms": wf * 1e3, "proofs_per_s": a.count / wf, "event_ms": ev[True]},
        "unfused": {"wall_ms": wu * 1e3, "proofs_per_s": a.count / wu, "event_ms": ev[False]},
        "wall_ratio_fused_over_unfused": wf / wu,
        "modexp_event_ratio_fused_over_unfused": ev[True]["modexp"] / ev[False]["modexp"],
        "wall_spread_fused": (max(wall[True]) - min(wall[True])) / wf,
        "wall_spread_unfused": (max(wall[False]) - min(wall[False])) / wu,
    }))
    del keep


if __name__ == "__main__":
    main()
