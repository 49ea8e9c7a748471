"""CPU check of bench.py --dump-outputs: the LocalKey written as DIR/<name>.npy
reads back to the same integers (32-bit limbs, exact in float64)."""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "fs-dkr_amd")]

import bench  # noqa: E402
from fsdkr.types import DecryptionKey, EncryptionKey, LocalKey, VerifiableSS  # noqa: E402


def _ints(arr):
    return [sum(int(v) << (32 * k) for k, v in enumerate(row)) for row in arr]


def test_dump_outputs_round_trip(tmp_path):
    big = (1 << 2048) - 159
    pts = [(3, (1 << 256) - 1), None, ((1 << 255) + 7, 1 << 32)]
    key = LocalKey(paillier_dk=DecryptionKey(3, 5), pk_vec=pts, x_i=(1 << 256) - 2, y=pts[0],
                   paillier_key_vec=[EncryptionKey(big, big * big), EncryptionKey(15, 225)], y_sum_s=None,
                   h1_h2_n_tilde_vec=[], vss_scheme=VerifiableSS(1, 3), i=1, t=1, n=3)
    out = tmp_path / "dump"
    bench.dump_outputs(str(out), key, 2048)
    got = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert sorted(got) == ["paillier_key_vec_n", "pk_vec", "x_i", "y"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert _ints(got["x_i"]) == [key.x_i]
    assert _ints(got["paillier_key_vec_n"]) == [big, 15]
    assert got["pk_vec"].shape == (3, 16) and got["y"].shape == (1, 16)
    assert [(_ints(r[None, :8])[0], _ints(r[None, 8:])[0]) for r in got["pk_vec"]] == \
        [pts[0], (0, 0), pts[2]]
    assert np.array_equal(got["y"][0], got["pk_vec"][0])
