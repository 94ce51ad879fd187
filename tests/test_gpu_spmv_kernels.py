"""The gather kernels of the sparse-operator route at the C-ABI: ``SpmvStack`` built directly from a structure dict,
``eval_rhs`` / ``rk4_solve`` called with plain arrays, under the three settings of ``spmv_lanes``, every element the
schedule defines compared with the 80-bit reference of tests/spmv_reference.py.

The bound is absolute, ``max|device - ref| <= tolerance``, with tolerance = max(8 max|f64 - ref|, 32 eps max|ref|) from a
float64 NumPy restatement of the same case (never from the device): of order 1e-14 .. 1e-13 for the RK4 cases, and up to
about 1e-12 for a direct evaluation at t = 1000 (where rounding frame_im * t alone costs 2e-13).
tests/test_spmv_reference_host.py shows that this bound rejects every mutant of the restatement by a factor >= 100.
Every case prints its figures before it asserts (pytest -s: the rows of profiles/spmv_kernel_tests.md)."""
import numpy as np
import pytest

import spmv_reference as sr

pytestmark = pytest.mark.gpu

LANES = (0, 1, 2)


@pytest.fixture(scope="module")
def ctx():
    import qiskit_dynamics_amd as q

    return q.default_context()  # raises loudly when libmidyn / the GPU is missing


def _stack(ctx, struct):
    from qiskit_dynamics_amd._lib import SpmvStack

    packed = {f: struct[f] for f in ("n", "k", "width", "cols", "ops", "vals")}
    stack = SpmvStack(ctx, struct["n"], struct["k"], packed, struct["frame_im"])
    assert (stack.n, stack.k, stack.width, stack.has_frame) == (struct["n"], struct["k"], struct["width"],
                                                                 int(struct["frame_im"] is not None))
    assert stack.nnz == int(sr.row_lengths(struct).sum()) - _unused_inside(struct) and stack.n_pad == -(-struct["n"] // 64) * 64
    return stack


def _unused_inside(struct):
    """Slots that read as unused but lie before a row's last slot in use (none in these structures)."""
    n, k, w = struct["n"], struct["k"], struct["width"]
    unused = (struct["ops"] == k) & (struct["cols"] == np.arange(n)[:, None]) & (struct["vals"] == 0)
    return int(np.sum(unused & (np.arange(w)[None, :] < sr.row_lengths(struct)[:, None])))


def _record(name, lanes, spread, tol, err):
    """One row of profiles/spmv_kernel_tests.md (shown by pytest -s or on failure)."""
    print(f"| `{name}` | {lanes} | {spread:.2e} | {tol:.2e} | {err:.2e} |")


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("name", sr.RK4_CASES)
def test_rk4_solve_against_the_extended_precision_reference(ctx, name, lanes):
    c = sr.rk4_case(name)
    struct = c["struct"]
    stack = _stack(ctx, struct)
    try:
        with ctx.options(spmv_lanes=lanes):
            got = stack.rk4_solve(c["times"], c["S"], c["step_rows"], c["step_h"], c["step_save"], c["P"], c["y0"], c["B"],
                                  c["shared"])
    finally:
        stack.close()
    assert got.shape == (c["B"], c["P"], struct["n"], c["m"]) and got.dtype == np.complex128
    keep = c["slots"]
    want = np.broadcast_to(c["y0"], (c["B"], struct["n"], c["m"]))
    assert np.array_equal(got[:, 0], want), "slot 0 is y0, bit for bit"
    err = sr.max_abs_diff(got[:, keep], c["ref"][:, keep])
    _record(name, lanes, c["spread"], c["tol"], err)
    assert np.all(np.isfinite(got[:, keep]))
    if struct["width"] == 0:          # no slot at all: the state never moves, whatever the phases and the coefficients are
        for slot in np.flatnonzero(keep):
            assert np.array_equal(got[:, slot], want), f"slot {slot} differs from y0"
    assert err <= c["tol"], f"max|device - ref| = {err:.3e} > {c['tol']:.3e}"


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("name", sr.EVAL_CASES)
def test_eval_rhs_against_the_extended_precision_reference(ctx, name, lanes):
    c = sr.eval_case(name)
    stack = _stack(ctx, c["struct"])
    try:
        with ctx.options(spmv_lanes=lanes):
            got = [stack.eval_rhs(c["coef"], t, c["y"]) for t in sr.EVAL_TIMES]
    finally:
        stack.close()
    errs = []
    for g, ref in zip(got, c["ref"]):
        assert g.shape == c["y"].shape and g.dtype == np.complex128
        errs.append(sr.max_abs_diff(g, ref))
    for t, spread, tol, err in zip(sr.EVAL_TIMES, c["spread"], c["tol"], errs):
        _record(f"{name} t={t:g}", lanes, spread, tol, err)
    for t, tol, err in zip(sr.EVAL_TIMES, c["tol"], errs):
        assert err <= tol, f"t = {t}: max|device - ref| = {err:.3e} > {tol:.3e}"
