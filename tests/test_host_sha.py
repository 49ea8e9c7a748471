"""The streaming SHA-256 of fs-dkr_amd/csrc/sha256.hpp (host + device code,
curv to_bytes absorption incl. unaligned word appends) against hashlib, on CPU."""
import hashlib
import os
import random
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sha_exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("sha") / "sha_host"
    subprocess.run(["hipcc", "-O1", "-std=c++17", "-I", os.path.join(REPO, "fs-dkr_amd", "csrc"),
                    os.path.join(REPO, "tests", "native", "sha_host.cpp"), "-o", str(out)], check=True)
    return str(out)


def _to_bytes(v):
    return v.to_bytes(max(1, (v.bit_length() + 7) // 8), "big")


def test_sha_matches_hashlib(sha_exe):
    rnd = random.Random(1)
    for trial in range(40):
        vals = []
        for _ in range(rnd.randint(1, 12)):
            bits = rnd.choice([0, 1, 7, 8, 9, 31, 32, 33, 255, 256, 257, 1000, 2048, 4096])
            vals.append(rnd.getrandbits(bits) if bits else 0)
        limbs = []
        for v in vals:
            n = max(1, (v.bit_length() + 31) // 32) + rnd.randint(0, 2)   # zero-padded widths
            limbs.append([(v >> (32 * j)) & 0xFFFFFFFF for j in range(n)])
        inp = f"{len(vals)} " + " ".join(f"{len(l)} " + " ".join(map(str, l)) for l in limbs)
        out = subprocess.run([sha_exe], input=inp, capture_output=True, text=True, check=True).stdout.split()
        got = sum(int(x) << (32 * i) for i, x in enumerate(out))
        want = int.from_bytes(hashlib.sha256(b"".join(_to_bytes(v) for v in vals)).digest(), "big")
        assert got == want, (trial, vals)


def _digest(sha_exe, vals, pad=None):
    """SHA-256 over to_bytes of vals through the header; pad[k] extra zero limbs on value k."""
    limbs = []
    for k, v in enumerate(vals):
        n = max(1, (v.bit_length() + 31) // 32) + (pad[k] if pad else 0)
        limbs.append([(v >> (32 * j)) & 0xFFFFFFFF for j in range(n)])
    inp = f"{len(vals)} " + " ".join(f"{len(l)} " + " ".join(map(str, l)) for l in limbs)
    out = subprocess.run([sha_exe], input=inp, capture_output=True, text=True, check=True).stdout.split()
    return sum(int(x) << (32 * i) for i, x in enumerate(out))


def _want(vals):
    return int.from_bytes(hashlib.sha256(b"".join(_to_bytes(v) for v in vals)).digest(), "big")


def _exact(rnd, nbytes):
    """A value of exactly nbytes bytes."""
    return rnd.getrandbits(8 * nbytes) | (1 << (8 * nbytes - 1))


def test_sha_word_and_finish_table(sha_exe):
    """word() at every misalignment and finish_le() at every pending length: a first
    value of 1 to 4 bytes sets the offset at which the words of a 41-byte value
    start (no block boundary yet), and a third value brings the total to every
    residue mod 64 -- its words cross the block boundary at alignment total % 4, so
    every rollover w[0] = x << (32 - 8 off) is taken, and finish_le() sees 0 .. 63
    pending bytes (55: the last that pads within the block; 0: a bare padding block)."""
    rnd = random.Random(2)
    seen = set()
    for start in (1, 2, 3, 4):
        for total in range(70, 134):
            vals = [_exact(rnd, start), _exact(rnd, 41), _exact(rnd, total - start - 41)]
            assert sum(len(_to_bytes(v)) for v in vals) == total
            seen.add((start % 4, total % 64))
            pad = [rnd.randint(0, 2) for _ in vals]
            assert _digest(sha_exe, vals, pad) == _want(vals), (start, total, vals)
    assert seen == {(s, r) for s in range(4) for r in range(64)}


def test_sha_zero_and_limb_edges(sha_exe):
    """0 (one 0x00 byte), 2^32k (a lone top byte over k zero words) and 2^32k - 1 (no
    partial top word) at every start offset."""
    for start in (1, 2, 3, 4):
        for k in (1, 2, 3, 16, 17):
            vals = [(1 << (8 * start)) - 1, 0, 1 << (32 * k), (1 << (32 * k)) - 1, 0, 1 << (32 * k), 0]
            assert _digest(sha_exe, vals, [0, 2, 1, 1, 0, 0, 3]) == _want(vals), (start, k)
    assert _digest(sha_exe, [0]) == _want([0])
