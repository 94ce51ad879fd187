"""The mirrored combine kernels (csrc/midyn_combine_mirror.h) in the code object of libmidyn.so (no GPU needed).

combine_mirror_kernel keeps the combination of 32 L rows, two sets of 16-instance accumulators, the transposed operand (the
state at the wave's own rows) and two steps of transposed partials in registers: no spill, no scratch, and the loads of a step
are issued one step ahead of their use -- no `s_waitcnt vmcnt(0)` inside the kk loop (the loop's inner back edge).
"""
import os

import pytest

from conftest import ROOT

import codeobj

LIB = os.path.join(ROOT, "qiskit_dynamics_amd", "libmidyn.so")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
VARIANTS = ((0, 1), (0, 2), (1, 0), (2, 0), (1, 1), (2, 2))


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(LIB):
        pytest.skip("libmidyn.so has not been built")
    return codeobj.library_kernels(LIB)


def test_mirror_kernels_exist_without_spills(kernels):
    names = [f"combine_mirror_kernelILi{r}ELi{i}EE" for r, i in VARIANTS] + [f"mirror_finish_kernelILi{e}EE" for e in range(5)]
    for frag in names:
        found = [n for n in kernels if frag in n]
        assert len(found) == 1, (frag, found)
        k = kernels[found[0]]
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".private_segment_fixed_size", 0) == 0, (frag, k)
    # (the contraction's own family keeps its size: the new kernels are not rhs_combine_kernel instantiations)
    assert not any("rhs_combine_kernel" in n and "mirror" in n for n in kernels)


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="llvm-objdump of the ROCm image not found")
def test_kk_loop_of_the_mirror_kernel_waits_for_no_drained_load(tmp_path):
    if not os.path.exists(LIB):
        pytest.skip("libmidyn.so has not been built")
    text = codeobj.disassembly(LIB, tmp_path, OBJDUMP)
    lines = text.split("\n")
    for r, i in VARIANTS:
        frag = f"combine_mirror_kernelILi{r}ELi{i}EE"
        start = next(j for j, l in enumerate(lines) if frag in l and l.rstrip().endswith(">:"))
        end = next(j for j in range(start + 1, len(lines)) if lines[j].rstrip().endswith(">:") or j == len(lines) - 1)
        # (instruction, address) pairs; the address is in the comment llvm-objdump prints after every instruction
        ops = []
        for l in lines[start + 1:end]:
            code, _, note = l.partition("//")
            if code.split() and ":" in note:
                ops.append((code.split(), int(note.split(":")[0], 16)))
        assert not any(o[0].startswith("scratch_") for o, _ in ops), frag
        base = ops[0][1]
        # the kk loop: the innermost loop that holds MFMAs -- a backward conditional branch (its target, from the `<symbol+0x..>`
        # note, lies before it) whose span [target, branch] holds MFMAs and is the shortest of those that do
        loops = []
        for j, l in enumerate(lines[start + 1:end]):
            code = l.split("//")[0].split()
            if code and code[0].startswith("s_cbranch") and "+0x" in l:
                here = int(l.split("//")[1].split(":")[0], 16)
                target = base + int(l.rsplit("+0x", 1)[1].rstrip(">").strip(), 16)
                if target < here:
                    body = [o for o, a in ops if target <= a <= here]
                    if any(o[0].startswith("v_mfma") for o in body):
                        loops.append((here - target, body))
        assert loops, frag
        body = min(loops, key=lambda x: x[0])[1]
        assert sum(o[0].startswith("v_mfma_f64_16x16x4") for o in body) == 4 * 2 * 2 * (r + i), frag
        waits = [" ".join(o) for o in body if o[0] == "s_waitcnt" and "vmcnt(0)" in " ".join(o)]
        assert not waits, (frag, waits)
        assert sum(o[0].startswith("v_permlane") for o in body) == 2 * 2 * 2 * 2 + 2 * 2 * 2, frag   # lo / hi words
