"""The constant-time kernels of Bob's MtA response (csrc/mta_ct.hip) in the gfx950
disassembly of the built libfsdkr.so, by the scan of tests/test_ec_ct_isa.py:
after a kernel's first vector load there is no branch on a vector condition (VCC
or EXEC), so no lane's data (b, beta', r) can steer the instruction stream; the
loops' back-edges run on scalar counters (SCC).  The same scan finds such
branches in modexp_tail_kernel, the public-exponent joint tail, so it can see
what it looks for."""
import importlib.util
import os
import shutil

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(REPO, "fs-dkr_amd", "fsdkr", "libfsdkr.so")
LOADS = ("global_load_", "flat_load_", "buffer_load_", "scratch_load_")
VECTOR_BRANCHES = ("s_cbranch_vccz", "s_cbranch_vccnz", "s_cbranch_execz", "s_cbranch_execnz")
CT_KERNELS = ("mta_tail_ct_kernel", "binom_ct_kernel<64>", "binom_ct_kernel<96>")
PUBLIC_TAIL = "modexp_tail_kernel<144, 8, 128, true, false, false>"


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
    assert kernel in kernels, sorted(k for k in kernels if "mta" in k or "binom" in k)
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


def test_scan_sees_the_public_tail_branches(kernels):
    assert PUBLIC_TAIL in kernels, sorted(k for k in kernels if k.startswith("modexp_tail"))
    found = vector_branches_after_first_load(kernels[PUBLIC_TAIL])
    assert found
