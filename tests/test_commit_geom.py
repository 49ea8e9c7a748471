"""The launch geometry of fsdkr_pedersen_commit_ct (fs-dkr_amd/csrc/commit_geom.hpp:
commit_choose_b, commit_padded_lanes, commit_ct_ipb) on the CPU, compiled with g++
alone: every row of the shape table that tests/test_commit_ct_shapes_gpu.py runs
lands in the class it is in the table for (a small column count, a top block that is
partly padding, the 16- or the 64-instance block), by the compiled functions and not
by a restatement of them; and one key's tables stay within the 512 KiB budget, so
that the device's memory cap (16 GiB here) cannot change b on a real device."""
import os
import subprocess

import pytest

import commit_ct_shapes as shapes

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def geometry(tmp_path_factory):
    """(b, vx, vy, ipb) per row name, from the compiled header."""
    out = tmp_path_factory.mktemp("cg") / "commit_geom_host"
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", os.path.join(REPO, "fs-dkr_amd", "csrc"),
                    os.path.join(REPO, "tests", "native", "commit_geom_host.cpp"), "-o", str(out)], check=True)
    inp = "".join(shapes.geometry_input(r) + "\n" for r in shapes.ROWS)
    lines = subprocess.run([str(out)], input=inp, capture_output=True, text=True, check=True).stdout.split("\n")
    assert len([ln for ln in lines if ln]) == len(shapes.ROWS)
    return {r.name: tuple(int(v) for v in ln.split()) for r, ln in zip(shapes.ROWS, lines)}


def test_row_names_are_unique():
    assert len({r.name for r in shapes.ROWS}) == len(shapes.ROWS)
    assert {r.want for r in shapes.ROWS} == {"b<=8", "b==1", "b==16", "padded", "ipb==16", "ipb==64"}


@pytest.mark.parametrize("row", shapes.ROWS, ids=[r.name for r in shapes.ROWS])
def test_row_is_in_its_class(geometry, row):
    b, vx, vy, ipb = geometry[row.name]
    print(f"{row.name}: b={b} vx={vx} vy={vy} ipb={ipb}")
    assert shapes.in_class(row, b, vx, vy, ipb), (row, b, vx, vy, ipb)
    assert ipb in (16, 64)
    # one key's tables are within the budget: the device's cap (far above 512 KiB a key) cannot bind
    assert (vx + vy) * 16 * shapes.ENTRY_BYTES[row.nl] <= shapes.KEY_BUDGET
