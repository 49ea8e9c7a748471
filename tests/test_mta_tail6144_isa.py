"""The constant-time tails of Bob's two mod-N^2 chains for 3072-bit keys
(csrc/mta_ct.hip mta_tail_ct6144_kernel, bob_v_tail_ct6144_kernel) in the gfx950
disassembly of the built libfsdkr.so, by the scan of tests/test_mta_respond_isa.py:
after a kernel's first vector load there is no branch on a vector condition (VCC or
EXEC), so no lane's data (b / alpha, beta' / gamma, r / beta) can steer the
instruction stream; every backward branch runs on a scalar counter (SCC) or is
unconditional."""
import pytest

from test_mta_respond_isa import _tool, kernels, vector_branches_after_first_load  # noqa: F401

KERNELS = ("mta_tail_ct6144_kernel", "bob_v_tail_ct6144_kernel")


@pytest.mark.parametrize("kernel", KERNELS)
def test_no_vector_branch_after_first_load(kernels, kernel):  # noqa: F811
    assert kernel in kernels, sorted(k for k in kernels if "tail" in k)
    found = vector_branches_after_first_load(kernels[kernel])
    assert found is not None, "no vector load found"
    assert found == []


@pytest.mark.parametrize("kernel", KERNELS)
def test_loops_run_on_scalar_counters(kernels, kernel):  # noqa: F811
    t = _tool()
    ins = kernels[kernel]
    back = [ins[e][1] for _, e in t.loops(ins)]   # every backward branch: SCC, or unconditional
    assert any(op in ("s_cbranch_scc0", "s_cbranch_scc1") for op in back), back
    assert all(op in ("s_cbranch_scc0", "s_cbranch_scc1", "s_branch") for op in back), back
