"""Pedersen-style commitments h1^x h2^y mod N~ with secret exponents, and Alice's
MtA messages built on them, on one MI355X.

Commit rows: fsdkr_pedersen_commit_ct (ONE constant-time two-base comb per
commitment, csrc/comb_ct.hip) against the composed path that generate_bob uses
today: two fsdkr_modexp_batch_ct calls (h1^x, h2^y through the regular-access
square-and-multiply kernel) and the product modulo N~ on the host.  Both start from
packed limb rows and end with Python ints.  Sizes: (xl, yl) limbs of x and y, the
instances and the keys of the call (instances spread evenly over the keys).  The
moduli are random odd integers of full width (the work does not depend on their
factors); the first `--check` instances of every row must equal pow's values on
both paths.

MtA rows: mta.initiate (Enc(a; r), the commitments, Enc(alpha; beta), r^e: the
whole call, host draws and hashing included) and mta.verify_alice over 4096
exchanges of one device-generated 2048-bit key set; the proofs must all verify.

Per row: `--warmup` calls, then `--reps` timed calls, interleaved new / composed per
repeat; reported are the medians, the spreads (max - min), the ratio composed /
new and, for the new path, the HIP-event time of its table launches and of
commit_ct_kernel (a timing context).  One JSON line per row.

  python tools/bench_commit_ct.py
  python tools/bench_commit_ct.py --rows commit      # the commit rows only"""
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

from fsdkr import Context, keygen, mta  # noqa: E402
from fsdkr._native import _ptr, ints_to_limbs, limbs_to_ints  # noqa: E402
from oracle.rng import Rng  # noqa: E402

COMMIT_ROWS = [(64, 8, 72, 4096, 1), (64, 8, 72, 64, 64), (64, 8, 72, 1, 1),
               (64, 24, 88, 4096, 1), (64, 24, 88, 64, 64), (64, 24, 88, 1, 1),
               (96, 24, 120, 4096, 1)]


def build(nl, xl, yl, count, n_keys):
    rng = Rng(("bench-commit-ct", nl, xl, yl, count, n_keys))
    keys = []
    for _ in range(n_keys):
        nt = rng.bits(32 * nl) | (1 << (32 * nl - 1)) | 1
        keys.append((nt, rng.sample_below(nt), rng.sample_below(nt)))
    xs = [rng.bits(32 * xl) for _ in range(count)]
    ys = [rng.bits(32 * yl) for _ in range(count)]
    idx = [i % n_keys for i in range(count)]
    arr = dict(X=ints_to_limbs(xs, xl), Y=ints_to_limbs(ys, yl), I=np.asarray(idx, dtype=np.uint32),
               Nt=ints_to_limbs([k[0] for k in keys], nl), H1=ints_to_limbs([k[1] for k in keys], nl),
               H2=ints_to_limbs([k[2] for k in keys], nl),
               B1=ints_to_limbs([keys[i][1] for i in idx], nl), B2=ints_to_limbs([keys[i][2] for i in idx], nl))
    return keys, xs, ys, idx, arr


def commit_new(ctx, nl, xl, yl, count, n_keys, a):
    out = np.zeros((count, nl), dtype=np.uint32)
    ctx.check(ctx._lib.fsdkr_pedersen_commit_ct(ctx.handle, nl, count, _ptr(a["X"]), xl, _ptr(a["Y"]), yl, _ptr(a["I"]),
                                                _ptr(a["Nt"]), _ptr(a["H1"]), _ptr(a["H2"]), n_keys, _ptr(out)))
    return limbs_to_ints(out)


def commit_composed(ctx, nl, xl, yl, count, n_keys, a, mods):
    o1 = np.zeros((count, nl), dtype=np.uint32)
    o2 = np.zeros((count, nl), dtype=np.uint32)
    fn = ctx._lib.fsdkr_modexp_batch_ct
    ctx.check(fn(ctx.handle, nl, count, _ptr(a["B1"]), _ptr(a["X"]), xl, _ptr(a["I"]), _ptr(a["Nt"]), n_keys, _ptr(o1)))
    ctx.check(fn(ctx.handle, nl, count, _ptr(a["B2"]), _ptr(a["Y"]), yl, _ptr(a["I"]), _ptr(a["Nt"]), n_keys, _ptr(o2)))
    return [p * q % m for p, q, m in zip(limbs_to_ints(o1), limbs_to_ints(o2), mods)]


def timed(fns, warmup, reps):
    """medians and spreads (ms) of `reps` interleaved calls of every fn"""
    for fn in fns:
        for _ in range(warmup):
            fn()
    t = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            t[k].append((time.perf_counter() - t0) * 1e3)
    return [(statistics.median(v), max(v) - min(v)) for v in t]


def commit_row(ctx, ev_ctx, row, a):
    nl, xl, yl, count, n_keys = row
    keys, xs, ys, idx, arr = build(nl, xl, yl, count, n_keys)
    mods = [keys[i][0] for i in idx]
    chk = min(a.check, count)
    want = [pow(keys[idx[i]][1], xs[i], mods[i]) * pow(keys[idx[i]][2], ys[i], mods[i]) % mods[i] for i in range(chk)]
    new = lambda: commit_new(ctx, nl, xl, yl, count, n_keys, arr)
    old = lambda: commit_composed(ctx, nl, xl, yl, count, n_keys, arr, mods)
    assert new()[:chk] == want and old()[:chk] == want
    (mn, sn), (mo, so) = timed([new, old], a.warmup, a.reps)
    # HIP-event time of the new path's launches (a timing context): the chains and
    # tables of the call's keys, and commit_ct_kernel
    commit_new(ev_ctx, nl, xl, yl, count, n_keys, arr)
    ev_ctx.kernel_time_reset()
    for _ in range(a.reps):
        commit_new(ev_ctx, nl, xl, yl, count, n_keys, arr)
    ev = {k: ev_ctx.kernel_time(k)[0] / a.reps for k in ("commit_tables", "commit_ct")}
    return {"row": "commit", "new_event_ms": ev, "nl": nl, "xl": xl, "yl": yl, "instances": count, "keys": n_keys, "reps": a.reps,
            "new_ms": mn, "new_spread_ms": sn, "composed_ms": mo, "composed_spread_ms": so,
            "composed_over_new": mo / mn, "new_faster_by_more_than_both_spreads": bool(mo - mn > sn + so)}


def mta_rows(ctx, a):
    from oracle.paillier import EncryptionKey
    from fsdkr.types import DLogStatement
    rng = Rng("bench-commit-ct-mta")
    (ek, _), (ekt, dkt) = keygen.keypairs_with_modulus_size(ctx, rng, 2048, 2)
    h1 = rng.sample_below(ekt.n)
    st = DLogStatement(ekt.n, h1, pow(h1, rng.sample_below((dkt.p - 1) * (dkt.q - 1)), ekt.n))
    ek = EncryptionKey.from_n(ek.n)
    n = a.exchanges
    as_ = [rng.sample_below(mta.Q) for _ in range(n)]
    eks, sts = [ek] * n, [st] * n
    seeds = iter(range(1 << 30))
    last = {}

    def initiate():
        last["v"] = mta.initiate(as_, eks, sts, Rng(("bench-initiate", next(seeds))), ctx=ctx)

    (mi, si), = timed([initiate], a.warmup, a.reps)
    a_encs, _, proofs = last["v"]

    def verify():
        last["ok"] = mta.verify_alice(proofs, a_encs, eks, sts, ctx=ctx)

    (mv, sv), = timed([verify], a.warmup, a.reps)
    assert list(last["ok"]) == [1] * n
    return [{"row": "initiate", "exchanges": n, "keys": 1, "reps": a.reps, "ms": mi, "spread_ms": si,
             "exchanges_per_s": n / mi * 1e3},
            {"row": "verify_alice", "proofs": n, "keys": 1, "reps": a.reps, "ms": mv, "spread_ms": sv,
             "proofs_per_s": n / mv * 1e3}]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", choices=("all", "commit", "mta"), default="all")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--check", type=int, default=4, help="instances per row compared with pow")
    ap.add_argument("--exchanges", type=int, default=4096)
    a = ap.parse_args()
    if a.reps < 5:
        ap.error("at least 5 timed runs per path")
    ctx, ev_ctx = Context(), Context(timing=True)
    if a.rows in ("all", "commit"):
        for row in COMMIT_ROWS:
            print(json.dumps(commit_row(ctx, ev_ctx, row, a)), flush=True)
    if a.rows in ("all", "mta"):
        for rec in mta_rows(ctx, a):
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
