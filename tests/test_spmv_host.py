"""Host side of the sparse-operator route (include/midyn_spmv.h; no GPU needed): the header and the binding agree and the
library exports the entry points, the padded row structure ``pack_ell`` builds, the sparse workload builder, and the code
object of the gather kernels."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
from scipy import sparse

from conftest import ROOT

import codeobj
from qiskit_dynamics_amd import _lib, workloads
from qiskit_dynamics_amd._lib import DynamicsError, pack_ell

HEADER = os.path.join(ROOT, "include", "midyn_spmv.h")


def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(midyn_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_exactly_the_bound_symbols_and_the_library_exports_them():
    declared = _declared()
    assert declared == sorted(_lib.SPMV_SYMBOLS)
    assert not set(declared) & set(_lib.ABI_SYMBOLS)
    assert not set(declared) & set(_lib.GENTABLE_SYMBOLS)
    assert os.path.exists(_lib.LIB_PATH), "libmidyn.so not built: run __graft_entry__.build()"
    assert _lib.load() is not None
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} not exported by libmidyn.so"


def test_header_compiles_as_c99_and_cpp(tmp_path):
    c = tmp_path / "h.c"
    c.write_text('#include "%s"\nint main(void) { midyn_spmv* s = 0; return s != 0; }\n' % HEADER)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-o", str(tmp_path / "hc"), str(c)], check=True)
    cpp = tmp_path / "h.cpp"
    cpp.write_text('#include "%s"\nint main() { midyn_spmv* s = nullptr; return s != nullptr; }\n' % HEADER)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-o", str(tmp_path / "hpp"), str(cpp)], check=True)


# ---- pack_ell ----------------------------------------------------------------------------------------------------------
def _dense_from(cols, ops, vals, n, n_ops):
    """The n_ops + 1 dense matrices (static part last) a padded row structure (row-major view) describes."""
    out = np.zeros((n_ops + 1, n, n), dtype=complex)
    for r in range(n):
        for s in range(cols.shape[1]):
            out[ops[r, s], r, cols[r, s]] += vals[r, s]
    return out


def _small_stack():
    n = 7
    a0 = sparse.lil_matrix((n, n), dtype=complex)
    a0[0, 3], a0[0, 1], a0[2, 2], a0[6, 0] = 1 + 2j, -1j, 0.5, 3.0
    a1 = sparse.csr_matrix((n, n), dtype=complex)               # an operator with no entry at all
    a2 = sparse.lil_matrix((n, n), dtype=complex)
    a2[0, 0], a2[2, 5], a2[2, 1], a2[5, 5] = 2.0, 1j, -2.0, 0.25
    st = sparse.lil_matrix((n, n), dtype=complex)
    st[0, 6], st[3, 3], st[6, 6] = -1.0, 1j, 4.0
    return n, st.tocsr(), [a0.tocsr(), a1, a2.tocsr()]         # rows 1 and 4 are empty everywhere


def test_pack_ell_structure():
    n, st, ops = _small_stack()
    p = pack_ell(n, st, ops)
    k = 3
    assert (p["n"], p["k"], p["n_pad"]) == (n, k, 64)
    assert p["width"] == 4                                     # row 0: 2 + 0 + 1 slots of the operators and 1 of the static part
    assert p["cols"].dtype == np.int32 and p["ops"].dtype == np.int32 and p["vals"].dtype == np.complex128
    assert p["cols"].shape == p["ops"].shape == p["vals"].shape == (n, p["width"])
    assert p["cols_t"].shape == p["ops_t"].shape == p["vals_t"].shape == (p["width"], 64)
    for r in range(n):
        o = p["ops"][r]
        assert np.all(np.diff(o) >= 0), "slots of a row are grouped by operator index, padding (op = k) last"
        used = int(np.sum([m[r].nnz for m in ops + [st]]))
        assert np.all(p["cols"][r, used:] == r) and np.all(o[used:] == k) and np.all(p["vals"][r, used:] == 0)
    for r in (1, 4):                                           # empty rows: padding only
        assert np.all(p["ops"][r] == k) and np.all(p["vals"][r] == 0) and np.all(p["cols"][r] == r)
    assert not np.any(p["ops"] == 1)                           # the empty operator owns no slot
    assert 0 <= p["cols"].min() and p["cols"].max() < n
    assert 0 <= p["cols_t"].min() and p["cols_t"].max() < n and p["ops_t"].max() <= k
    want = np.stack([m.toarray() for m in ops + [st]])
    np.testing.assert_array_equal(_dense_from(p["cols"], p["ops"], p["vals"], n, k), want)
    np.testing.assert_array_equal(_dense_from(p["cols_t"][:, :n].T, p["ops_t"][:, :n].T, p["vals_t"][:, :n].T, n, k), want)
    assert np.all(p["vals_t"][:, n:] == 0) and np.all(p["ops_t"][:, n:] == k)


def test_pack_ell_duplicates_and_explicit_zeros():
    n = 4
    dup = sparse.coo_matrix((np.array([1.0, 2.0, 5.0, 0.0]), (np.array([1, 1, 2, 3]), np.array([2, 2, 0, 3]))), shape=(n, n))
    cancel = sparse.coo_matrix((np.array([1.5, -1.5, 1j]), (np.array([0, 0, 3]), np.array([1, 1, 0]))), shape=(n, n))
    p = pack_ell(n, None, [dup, cancel])
    assert p["width"] == 1                                     # (1,2) summed to one slot; the stored 0 and the cancelled pair dropped
    assert p["vals"][1, 0] == 3.0 and p["cols"][1, 0] == 2 and p["ops"][1, 0] == 0
    assert p["ops"][0, 0] == 2 and p["vals"][0, 0] == 0 and p["cols"][0, 0] == 0      # row 0: padding only
    assert (p["ops"][3, 0], p["cols"][3, 0], p["vals"][3, 0]) == (1, 0, 1j)
    np.testing.assert_array_equal(_dense_from(p["cols"], p["ops"], p["vals"], n, 2)[:2],
                                  np.stack([dup.toarray(), cancel.toarray()]))


def test_pack_ell_static_only_operators_only_and_empty():
    n, st, ops = _small_stack()
    p = pack_ell(n, st, None)
    assert p["k"] == 0 and np.all(p["ops"] == 0) and p["width"] == 1
    np.testing.assert_array_equal(_dense_from(p["cols"], p["ops"], p["vals"], n, 0)[0], st.toarray())
    p = pack_ell(n, None, ops)
    np.testing.assert_array_equal(_dense_from(p["cols"], p["ops"], p["vals"], n, 3)[:3], np.stack([m.toarray() for m in ops]))
    p = pack_ell(n, None, [sparse.csr_matrix((n, n))])
    assert p["width"] == 0 and p["cols"].shape == (n, 0) and p["cols_t"].shape == (0, 64)
    dense = np.arange(9.0).reshape(3, 3)                        # dense input is accepted
    np.testing.assert_array_equal(_dense_from(*(pack_ell(3, dense, [])[x] for x in ("cols", "ops", "vals")), 3, 0)[0], dense)


def test_pack_ell_refuses_bad_input():
    with pytest.raises(DynamicsError):
        pack_ell(4, None, [sparse.csr_matrix((4, 5))])          # not square
    with pytest.raises(DynamicsError):
        pack_ell(4, sparse.csr_matrix((3, 3)), [sparse.csr_matrix((4, 4))])   # another dimension
    with pytest.raises(DynamicsError):
        pack_ell(0, None, [])
    bad = sparse.csr_matrix(np.eye(4))
    bad.indices[2] = 9                                          # a column index outside [0, n)
    with pytest.raises(DynamicsError):
        pack_ell(4, None, [bad])
    bad = sparse.csr_matrix(np.eye(4))
    bad.indices[1] = -1
    with pytest.raises(DynamicsError):
        pack_ell(4, bad, [])


# ---- workloads ---------------------------------------------------------------------------------------------------------
def test_chain_hamiltonian_sparse_equals_the_dense_builder():
    h_d, ops, nu = workloads.chain_hamiltonian(6, 6)
    s_d, s_ops, s_nu = workloads.chain_hamiltonian_sparse(6, 6)
    assert sparse.issparse(s_d) and all(sparse.issparse(o) for o in s_ops) and len(s_ops) == 6
    np.testing.assert_array_equal(s_d.toarray(), h_d)
    for a, b in zip(s_ops, ops):
        np.testing.assert_array_equal(a.toarray(), b)
    np.testing.assert_array_equal(s_nu, nu)
    cfg, scfg = workloads.schrodinger_config(4, 3, 1.0, 0.01), workloads.schrodinger_config_sparse(4, 3, 1.0, 0.01)
    assert sorted(cfg) == sorted(scfg)
    np.testing.assert_array_equal(scfg["h_d"].toarray(), cfg["h_d"])
    np.testing.assert_array_equal(scfg["y0"], cfg["y0"])
    np.testing.assert_array_equal(scfg["carrier"], cfg["carrier"])


def test_chain_hamiltonian_sparse_at_14_qubits_stays_sparse():
    h_d, ops, _ = workloads.chain_hamiltonian_sparse(14, 2)
    assert h_d.shape == (1 << 14, 1 << 14) and h_d.nnz == (1 << 14) * 14      # diagonal + 13 XX couplings per row
    assert all(o.nnz == 1 << 14 for o in ops)


# ---- code object -------------------------------------------------------------------------------------------------------
def test_code_object_holds_the_gather_kernels_without_spills_or_scratch():
    assert os.path.exists(_lib.LIB_PATH), "libmidyn.so not built: run __graft_entry__.build()"
    kernels = codeobj.library_kernels(_lib.LIB_PATH)
    spmv = {name: k for name, k in kernels.items() if "spmv_" in name}
    for frag in ("spmv_cols_kernel", "spmv_rows_kernel"):
        assert len([name for name in spmv if frag in name]) == 5, (frag, sorted(spmv))     # stages 0 .. 4
    for frag in ("spmv_prep_kernel", "spmv_load_kernel"):
        assert len([name for name in spmv if frag in name]) == 1, (frag, sorted(spmv))
    for name, k in spmv.items():
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, name
        assert k.get(".private_segment_fixed_size", 0) == 0, name
