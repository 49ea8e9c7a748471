"""The constant-time two-base comb (csrc/comb_ct.hip) in the gfx950 disassembly of
the built libfsdkr.so, by the scan of tests/test_mta_respond_isa.py: after a
kernel's first vector load there is no branch on a vector condition (VCC or EXEC),
so no lane's data (the digits of x and y) can steer the instruction stream, and the
loops' back-edges run on scalar counters (SCC).  The same scan finds such branches
in comb_exp_kernel, the public-exponent comb it was made from, so it can see what
it looks for."""
import importlib.util
import os
import shutil

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "fs-dkr_amd", "fsdkr", "libfsdkr.so")
LOADS = ("global_load_", "flat_load_", "buffer_load_", "scratch_load_")
VECTOR_BRANCHES = ("s_cbranch_vccz", "s_cbranch_vccnz", "s_cbranch_execz", "s_cbranch_execnz")
CT_KERNELS = ("commit_ct_kernel<72, 4, 64>", "commit_ct_kernel<108, 4, 96>")
PUBLIC_COMBS = ("comb_exp_kernel<72, 4, 64, true>", "comb_exp_kernel<108, 4, 96, true>")


def _tool():
    spec = importlib.util.spec_from_file_location("mac_share", os.path.join(REPO, "tools", "mac_share.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(LIB) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-objdump") or not shutil.which("c++filt"):
        pytest.skip("needs the built library and the ROCm llvm-objdump")
    t = _tool()
    funcs = t.disassemble(LIB)
    dm = t.demangle(list(funcs))
    return {t.short(dm[k]): v for k, v in funcs.items() if v}


def vector_branches_after_first_load(ins):
    """(mnemonic, line) of every VCC / EXEC branch after the first vector load; None without a load"""
    first = next((k for k, (_, op, _) in enumerate(ins) if op.startswith(LOADS)), None)
    if first is None:
        return None
    return [(op, line.strip()) for _, op, line in ins[first + 1:] if op in VECTOR_BRANCHES]


@pytest.mark.parametrize("kernel", CT_KERNELS)
def test_no_vector_branch_after_first_load(kernels, kernel):
    assert kernel in kernels, sorted(k for k in kernels if "commit" in k or "comb" in k)
    found = vector_branches_after_first_load(kernels[kernel])
    assert found is not None, "no vector load found"
    assert found == []


@pytest.mark.parametrize("kernel", CT_KERNELS)
def test_loops_run_on_scalar_counters(kernels, kernel):
    t = _tool()
    ins = kernels[kernel]
    back = [ins[e][1] for _, e in t.loops(ins)]   # every backward branch: SCC, or unconditional
    assert any(op in ("s_cbranch_scc0", "s_cbranch_scc1") for op in back), back
    assert all(op in ("s_cbranch_scc0", "s_cbranch_scc1", "s_branch") for op in back), back


@pytest.mark.parametrize("kernel", PUBLIC_COMBS)
def test_scan_sees_the_public_comb_branches(kernels, kernel):
    assert kernel in kernels, sorted(k for k in kernels if k.startswith("comb_exp"))
    found = vector_branches_after_first_load(kernels[kernel])
    assert found
