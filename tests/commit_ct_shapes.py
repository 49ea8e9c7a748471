"""Launch shapes of fsdkr_pedersen_commit_ct that the production batch sizes select
and tests/test_commit_ct_gpu.py does not reach, shared by the CPU check of the
geometry (tests/test_commit_geom.py: the compiled commit_geom.hpp puts every row in
its class) and the GPU run of the same rows (tests/test_commit_ct_shapes_gpu.py).

A row: the width class nl, the exponent widths (xl, yl), the instances per key of
the call (a key with 0 takes part in n_keys only), the number of distinct
instances the count is reached from by repetition, and the class the row is in the
table for:
  "b<=8", "b==1", "b==16"   small column counts (the most table blocks per key)
  "padded"                  4 b does not divide 32 xl or 32 yl: the top block of the
                            comb is partly padding past the exponent's top limb
  "ipb==16", "ipb==64"      the small launch's block at its upper bound, the full block
"""
from collections import namedtuple

Row = namedtuple("Row", "name nl xl yl per distinct want")

ROWS = [
    Row("b8-8x72", 64, 8, 72, (304,), 48, "b<=8"),
    Row("b8-24x88", 64, 24, 88, (304,), 48, "b<=8"),
    Row("b1-1x1", 64, 1, 1, (304,), 16, "b==1"),
    Row("b16-3072", 96, 24, 120, (64,), 24, "b==16"),
    Row("b8-two-keys", 64, 8, 72, (300, 300), 48, "b<=8"),
    Row("pad-128x128-48", 64, 128, 128, (48,), 16, "padded"),
    Row("pad-128x128-304", 64, 128, 128, (304,), 16, "padded"),
    Row("pad-8x73", 64, 8, 73, (16,), 16, "padded"),
    Row("pad-7x100-single", 64, 7, 100, (1,), 1, "padded"),
    Row("pad-128x1", 64, 128, 1, (64,), 16, "padded"),
    Row("pad-7x100-3072", 96, 7, 100, (16,), 16, "padded"),
    Row("block-16384", 64, 8, 72, (16384,), 48, "ipb==16"),
    Row("block-16385", 64, 8, 72, (16385,), 48, "ipb==64"),
    Row("block-three-keys", 64, 8, 72, (16300, 1, 65, 0), 48, "ipb==64"),
]

KEY_BUDGET = 512 << 10                 # kCommitKeyBudget: one key's tables
ENTRY_BYTES = {64: 72 * 4, 96: 108 * 4}   # a table row: 72 / 108 digits of 29 bits


def in_class(row, b, vx, vy, ipb):
    """Is the geometry (b, v_x, v_y, ipb) in the class the row stands for?"""
    if (vx, vy) != (-(-8 * row.xl // b), -(-8 * row.yl // b)):
        return False
    if row.want == "b<=8":
        return 1 <= b <= 8
    if row.want == "b==1":
        return b == 1
    if row.want == "b==16":
        return b == 16 and row.nl == 96
    if row.want == "padded":
        return (32 * row.xl) % (4 * b) != 0 or (32 * row.yl) % (4 * b) != 0
    if row.want in ("ipb==16", "ipb==64"):
        return ipb == int(row.want[5:])
    raise ValueError(row.want)


def geometry_input(row):
    """The row as commit_geom_host reads it: nl xl yl count n_keys per-key-counts."""
    return " ".join(map(str, (row.nl, row.xl, row.yl, sum(row.per), len(row.per)) + tuple(row.per)))
