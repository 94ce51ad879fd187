"""The kk loop of the mirrored combine kernel after the stage input moved to LDS (csrc/midyn_combine_mirror.h; no GPU needed).

  * mirror_probe_kernel<1..3> (profiling only, ctx option mirror_ablate) exist once each, without spills or scratch;
  * in the innermost loop of combine_mirror_kernel<0, 2> that holds MFMAs (four kk steps) the vector instructions other than
    MFMA / v_fma*_f64 / v_permlane* / v_add_f64 number at most 16: the 8 of the kernel that loaded the stage input from global
    memory (read from its gfx950 listing) plus at most two LDS address computations per step;
  * that loop reads the stage input with ds_read_b128 and, of global loads, holds only the fragments' global_load_dwordx2,
    4 per step;
  * the probe without global loads in the loop keeps the loop's 32 MFMAs and 256 vector FMAs (its time is compared with the
    kernel's, so the compiler must not have hoisted the loop-invariant combination).
"""
import os
import re

import pytest

from conftest import ROOT

import codeobj

LIB = os.path.join(ROOT, "qiskit_dynamics_amd", "libmidyn.so")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


def test_probe_kernels_exist_without_spills():
    if not os.path.exists(LIB):
        pytest.skip("libmidyn.so has not been built")
    kernels = codeobj.library_kernels(LIB)
    for abl in (1, 2, 3):
        found = [n for n in kernels if f"mirror_probe_kernelILi{abl}EE" in n]
        assert len(found) == 1, (abl, found)
        k = kernels[found[0]]
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".private_segment_fixed_size", 0) == 0, (abl, k)
    assert len([n for n in kernels if "mirror_probe_kernel" in n]) == 3


def _kk_loop(lines, frag):
    """Instructions of the innermost loop with MFMAs of the kernel whose symbol contains `frag`: the shortest span
    [target, branch] of a backward conditional branch that holds MFMAs (as tests/test_codeobj_mirror.py finds it)."""
    start = next(j for j, l in enumerate(lines) if frag in l and l.rstrip().endswith(">:"))
    end = next(j for j in range(start + 1, len(lines)) if lines[j].rstrip().endswith(">:") or j == len(lines) - 1)
    ops = []
    for l in lines[start + 1:end]:
        code, _, note = l.partition("//")
        if code.split() and ":" in note:
            ops.append((code.split(), int(note.split(":")[0], 16), l))
    base = ops[0][1]
    loops = []
    for o, here, l in ops:
        if o[0].startswith("s_cbranch") and "+0x" in l:
            target = base + int(l.rsplit("+0x", 1)[1].rstrip(">").strip(), 16)
            if target < here:
                body = [x for x, a, _ in ops if target <= a <= here]
                if any(x[0].startswith("v_mfma") for x in body):
                    loops.append((here - target, body))
    assert loops, frag
    return min(loops, key=lambda x: x[0])[1]


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="llvm-objdump of the ROCm image not found")
def test_kk_loop_reads_the_stage_input_from_lds(tmp_path):
    if not os.path.exists(LIB):
        pytest.skip("libmidyn.so has not been built")
    lines = codeobj.disassembly(LIB, tmp_path, OBJDUMP).split("\n")
    body = _kk_loop(lines, "combine_mirror_kernelILi0ELi2EE")
    names = [o[0] for o in body]
    assert sum(n.startswith("v_mfma_f64_16x16x4") for n in names) == 32
    fma = re.compile(r"v_fma(c|ak|mk)?_f64")
    assert sum(bool(fma.match(n)) for n in names) == 256
    other = [n for n in names if n.startswith("v_") and not (n.startswith("v_mfma") or fma.match(n) or n.startswith("v_permlane")
                                                             or n.startswith("v_add_f64"))]
    assert len(other) <= 16, other
    assert sum(n.startswith("ds_read_b128") for n in names) == 2 * 4, names          # two 16-instance groups x four kk steps
    loads = [n for n in names if n.startswith(("global_load", "buffer_load", "flat_load"))]
    assert len(loads) == 4 * 4 and all(n.startswith("global_load_dwordx2") for n in loads), loads
    # the probe without global loads in the loop still runs the whole combination there
    probe = [o[0] for o in _kk_loop(lines, "mirror_probe_kernelILi1EE")]
    assert sum(n.startswith("v_mfma_f64_16x16x4") for n in probe) == 32
    assert sum(bool(fma.match(n)) for n in probe) == 256
    assert sum(n.startswith("v_permlane") for n in probe) == 24
    assert not [n for n in probe if n.startswith(("global_load", "buffer_load", "flat_load"))]
