"""Host side of the callable-generator route (include/midyn_gentable.h; no GPU needed): the header and the binding agree
and the library exports the entry points, sample validation, the readiness rule of streamed rows, and the code object of
the two new kernels."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

import codeobj
from qiskit_dynamics_amd import _lib
from qiskit_dynamics_amd import solvers
from qiskit_dynamics_amd._lib import DynamicsError

HEADER = os.path.join(ROOT, "include", "midyn_gentable.h")


def test_header_declares_exactly_the_bound_symbols_and_the_library_exports_them():
    declared = sorted(set(re.findall(r"\b(midyn_[a-z0-9_]+)\s*\(", open(HEADER).read())))
    assert declared == sorted(_lib.GENTABLE_SYMBOLS)
    assert not set(declared) & set(_lib.ABI_SYMBOLS)
    assert os.path.exists(_lib.LIB_PATH), "libmidyn.so not built: run __graft_entry__.build()"
    assert _lib.load() is not None
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} not exported by libmidyn.so"


def test_header_compiles_as_c99_and_cpp(tmp_path):
    c = tmp_path / "h.c"
    c.write_text('#include "%s"\nint main(void) { midyn_gentable* g = 0; return g != 0; }\n' % HEADER)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-o", str(tmp_path / "hc"), str(c)], check=True)
    cpp = tmp_path / "h.cpp"
    cpp.write_text('#include "%s"\nint main() { midyn_gentable* g = nullptr; return g != nullptr; }\n' % HEADER)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-o", str(tmp_path / "hpp"), str(cpp)], check=True)


def test_sample_validation():
    real = np.arange(9.0).reshape(3, 3)
    out = solvers.validate_generator_sample(real, 0.25, 3)
    assert out.dtype == np.complex128 and out.shape == (3, 3)
    np.testing.assert_array_equal(out.real, real)
    assert solvers.validate_generator_sample([[1j]], 0.0, 1).dtype == np.complex128
    with pytest.raises(DynamicsError, match=r"t=0\.75.*\(2, 3\)"):
        solvers.validate_generator_sample(np.zeros((2, 3)), 0.75, 3)
    with pytest.raises(DynamicsError, match=r"t=0\.5"):
        solvers.validate_generator_sample(np.zeros((3, 3, 1)), 0.5, 3)
    for bad in (np.nan, np.inf, complex(0, np.nan)):
        g = np.zeros((3, 3), dtype=complex)
        g[1, 2] = bad
        with pytest.raises(DynamicsError, match=r"t=1\.5.*non-finite"):
            solvers.validate_generator_sample(g, 1.5, 3)


def _schedules(golden):
    g = golden("fixed_step")
    cases = [([0.0, 1.0], None, 0.1), ([1.0, 0.0], [0.8, 0.2], 0.1),
             (list(g["sizes8_tspan"]), list(g["sizes8_teval"]), float(g["sizes8_maxdt"]))]
    points = [("rk4", solvers._rk4_points)] + [(("magnus", o), solvers._magnus_points(o)) for o in (1, 2, 3)]
    for ts, te, mdt in cases:
        for _tag, pts in points:
            yield (ts, te), solvers.FixedStepSchedule(ts, te, mdt, pts)


def test_readiness_rule_prefix_maximum(golden):
    """A step is ready once every row up to the prefix maximum of the step rows has been pushed: each step's rows are at
    or below its prefix maximum, the prefix maximum never decreases, and it reaches the last row."""
    reread = False
    for (ts, te), sched in _schedules(golden):
        rows = sched.step_rows
        pref = np.maximum.accumulate(rows.max(axis=1))
        assert np.all(rows <= pref[:, None])
        assert np.all(np.diff(pref) >= 0)
        assert pref[-1] == len(sched.times) - 1
        # a zero-length t_eval interval reads rows pushed for an earlier step again (RK4: (t, t, t)): it needs no new row
        reread |= bool(np.any(rows.max(axis=1)[1:] <= pref[:-1]))
    assert reread, "sizes8 (t_eval with a repeated time) should give a step that reads only earlier rows"


LIB = _lib.LIB_PATH


def test_code_object_holds_the_new_kernels_without_spills():
    if not os.path.exists(LIB):
        pytest.skip("libmidyn.so has not been built")
    kernels = codeobj.library_kernels(LIB)
    wanted = ["gentable_gather_kernel"] + [f"gen_chain_kernelILi{np_}ELi{c}EE" for np_ in (64, 128) for c in (1, 16)]
    for frag in wanted:
        hits = [name for name in kernels if frag in name]
        assert len(hits) == 1, (frag, hits)
        k = kernels[hits[0]]
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, hits[0]
        assert k.get(".private_segment_fixed_size", 0) == 0, hits[0]
        assert k.get(".group_segment_fixed_size", 0) <= 160 * 1024, hits[0]
