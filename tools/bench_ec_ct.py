"""Secret-scalar secp256k1 on one MI355X: the constant-time entries against the
public-scalar fsdkr_ec_msm they replace on the prover side, in one process, on
the same scalars, the batch packed once.

  mul_g   fsdkr_ec_mul_g_ct (four-lane nibble comb) vs fsdkr_ec_msm with G, at
          641 scalars (a distribute at n = 256, t = 128: 2n + t + 1) and 65 536
  msm     fsdkr_ec_msm_ct (masked windows, no GLV) vs fsdkr_ec_msm, 641 x 1 term
          on a point other than G

Per path: `--warmup` calls, then `--reps` timed calls, interleaved A/B per
repeat.  Reported per path: the median wall time of the C call (upload, kernels,
readback), its spread (max - min) / median, the HIP-event time of the kernels
from a timing context, and the ratios.  Both paths must return the same points.

--distribute N adds whole distribute() calls at n = N, t = N / 2 on a synthetic
2048-bit key set, the same draws each time: as it stands, and with
Context.ec_mul_g routed through fsdkr_ec_msm with G (what distribute() did
before the constant-time entry), interleaved.

  python tools/bench_ec_ct.py
  python tools/bench_ec_ct.py --distribute 64"""
import argparse
import copy
import json
import os
import random
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "fs-dkr_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from fsdkr import Context  # noqa: E402
from fsdkr._native import _ptr, ints_to_limbs  # noqa: E402
from oracle import secp256k1 as ec  # noqa: E402
from oracle.rng import Rng  # noqa: E402


def _point_rows(pt, count):
    v = pt[0] | (pt[1] << 256)
    return np.ascontiguousarray(np.tile(ints_to_limbs([v], 16), (count, 1)))


def _stats(ts):
    med = statistics.median(ts)
    return {"wall_ms": med * 1e3, "spread": (max(ts) - min(ts)) / med}


def ab(ctx, ev_ctx, count, pt, fixed_base, reps, warmup):
    """A = the constant-time entry, B = fsdkr_ec_msm, on `count` random scalars times pt."""
    rnd = random.Random(count)
    Sc = ints_to_limbs([rnd.randrange(2 ** 256) for _ in range(count)], 8)
    Pt = _point_rows(pt, count)
    outs = {"ct": np.zeros((count, 16), dtype=np.uint32), "msm": np.zeros((count, 16), dtype=np.uint32)}

    def call(c, path):
        L, O = c._lib, outs[path]
        if path == "msm":
            c.check(L.fsdkr_ec_msm(c._h, count, 1, _ptr(Pt), _ptr(Sc), _ptr(O)))
        elif fixed_base:
            c.check(L.fsdkr_ec_mul_g_ct(c._h, count, _ptr(Sc), _ptr(O)))
        else:
            c.check(L.fsdkr_ec_msm_ct(c._h, count, 1, _ptr(Pt), _ptr(Sc), _ptr(O)))

    wall = {"ct": [], "msm": []}
    for _ in range(warmup):
        for path in ("ct", "msm"):
            call(ctx, path)
    assert np.array_equal(outs["ct"], outs["msm"])
    for _ in range(reps):
        for path in ("ct", "msm"):
            t0 = time.perf_counter()
            call(ctx, path)
            wall[path].append(time.perf_counter() - t0)
    ev = {}
    for path, name in (("ct", "ec_ct"), ("msm", "ec")):
        call(ev_ctx, path)
        ev_ctx.kernel_time_reset()
        for _ in range(reps):
            call(ev_ctx, path)
        ev[path] = ev_ctx.kernel_time(name)[0] / reps
    res = {"count": count, "fixed_base": fixed_base}
    for path in ("ct", "msm"):
        res[path] = dict(_stats(wall[path]), event_ms=ev[path])
    res["wall_ratio_ct_over_msm"] = res["ct"]["wall_ms"] / res["msm"]["wall_ms"]
    res["event_ratio_ct_over_msm"] = ev["ct"] / ev["msm"]
    return res


class _ViaMsm(Context):
    """distribute() as it ran before fsdkr_ec_mul_g_ct: G times every scalar through fsdkr_ec_msm."""

    def ec_mul_g(self, scalars):
        return self.ec_msm([[ec.G]] * len(scalars), [[k] for k in scalars])


def distribute_ab(n, reps, warmup):
    from fsdkr import distribute, synth
    ctxs = {"ct": Context(), "msm": _ViaMsm()}
    t = n // 2
    lk = synth.synth_collect(ctxs["ct"], 1, 0, t, 7, n_recv=n)[2]
    wall = {"ct": [], "msm": []}
    enc = {}
    for rep in range(warmup + reps):
        for path in ("ct", "msm"):
            key = copy.deepcopy(lk)
            t0 = time.perf_counter()
            msg, _ = distribute.distribute(key.i, key, n, Rng("bench-ec-ct"), ctx=ctxs[path])
            if rep >= warmup:
                wall[path].append(time.perf_counter() - t0)
            enc[path] = (msg.points_committed_vec, msg.coefficients_committed_vec.commitments)
    assert enc["ct"] == enc["msm"]
    res = {"n": n, "t": t, "ct": _stats(wall["ct"]), "msm": _stats(wall["msm"])}
    res["delta_ms_ct_minus_msm"] = res["ct"]["wall_ms"] - res["msm"]["wall_ms"]
    res["msm_spread_ms"] = res["msm"]["spread"] * res["msm"]["wall_ms"]
    for c in ctxs.values():
        c.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--counts", type=int, nargs="*", default=[641, 65536])
    ap.add_argument("--msm-count", type=int, default=641)
    ap.add_argument("--distribute", type=int, default=0, help="also time whole distribute() at this n")
    a = ap.parse_args()
    ctx, ev_ctx = Context(), Context(timing=True)
    out = {"reps": a.reps, "warmup": a.warmup,
           "mul_g": [ab(ctx, ev_ctx, c, ec.G, True, a.reps, a.warmup) for c in a.counts],
           "msm": ab(ctx, ev_ctx, a.msm_count, ec.mul(ec.G, 0xC0FFEE), False, a.reps, a.warmup)}
    ctx.close()
    ev_ctx.close()
    if a.distribute:
        out["distribute"] = distribute_ab(a.distribute, a.reps, a.warmup)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
