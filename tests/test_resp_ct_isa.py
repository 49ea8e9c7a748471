"""The provers' response kernel (csrc/resp_ct.hip) in the gfx950 disassembly of the
built libfsdkr.so, by the scan of tests/test_commit_ct_isa.py: after the kernel's
first vector load there is no branch on a vector condition (VCC or EXEC), so no
lane's data (the limbs of x and y) can steer the instruction stream, and the loops'
back-edges run on scalar counters (SCC).  The same scan finds such branches in
bob_challenge_kernel, which hashes public values with data-dependent lengths, so it
can see what it looks for."""
import importlib.util
import os
import shutil

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "fs-dkr_amd", "fsdkr", "libfsdkr.so")
LOADS = ("global_load_", "flat_load_", "buffer_load_", "scratch_load_")
VECTOR_BRANCHES = ("s_cbranch_vccz", "s_cbranch_vccnz", "s_cbranch_execz", "s_cbranch_execnz")
KERNEL = "resp_ct_kernel"
PUBLIC = "bob_challenge_kernel"


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


def test_no_vector_branch_after_first_load(kernels):
    assert KERNEL in kernels, sorted(k for k in kernels if "resp" in k)
    found = vector_branches_after_first_load(kernels[KERNEL])
    assert found is not None, "no vector load found"
    assert found == []


def test_no_vector_branch_at_all(kernels):
    """the loops before the first load (the staging of x) are scalar too"""
    assert [op for _, op, _ in kernels[KERNEL] if op in VECTOR_BRANCHES] == []


def test_loops_run_on_scalar_counters(kernels):
    t = _tool()
    ins = kernels[KERNEL]
    back = [ins[e][1] for _, e in t.loops(ins)]   # every backward branch: SCC, or unconditional
    assert any(op in ("s_cbranch_scc0", "s_cbranch_scc1") for op in back), back
    assert all(op in ("s_cbranch_scc0", "s_cbranch_scc1", "s_branch") for op in back), back


def test_scan_sees_the_public_hash_branches(kernels):
    assert PUBLIC in kernels, sorted(k for k in kernels if "challenge" in k)
    assert vector_branches_after_first_load(kernels[PUBLIC])
