"""The edge-case zoo (tests/edge_cases.py) on the CPU: the builders' own claims checked in
numpy, the oracle's level kernels against exact int64 references bit for bit, exact fixed
points, poisoned columns -- and a sensitivity check that the references notice one changed
value, one dropped entry and one swapped column pair.  No GPU."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import edge_cases as E
from tests.edge_cases import bits

NAMES = E.zoo_names()
GS_BLOCKS = (64, 48, 17, 1)


def _orc(O, A):
    return O.Csr.from_arrays(A.shape[0], A.shape[1], A.indptr, A.indices, A.data)


def _same(a, b):
    return np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("name", NAMES)
def test_builder_claims(name):
    """Limits of every zoo matrix, and what its docstring derives: the block count under the
    restated cut rule, value-indexed blocks, templates, chain widths, slab widths."""
    c = E.zoo()[name]
    A = c.A
    n = A.shape[0]
    assert A.shape[0] == A.shape[1] and n <= 10000 and A.nnz <= 300000
    assert c.doc and "block" in c.doc
    if A.nnz:
        E._int(A.data)
        assert np.abs(A.data).max() <= 1 << 11
    ln = np.diff(A.indptr)
    for i in np.flatnonzero(ln > 1):
        assert np.all(np.diff(A.indices[A.indptr[i]:A.indptr[i + 1]]) > 0)
    if c.full_diag:
        d = E._int(A.diagonal())
        assert np.all(d > 0) and np.all(d & (d - 1) == 0)
    min_rows = int(c.env.get("AMG_TPL_MIN_ROWS", 16384))
    tplf, ntpl, trows = E.row_templates(A, min_rows)
    blocks = E.cut_blocks(A, c.lw, tplf)
    assert len(blocks) == c.n_blocks, (len(blocks), blocks[:12])
    assert all(E.block_lines(A, b, c.lw) <= E.CAP // c.lw or b[1] - b[0] == 1 for b in blocks)
    if c.n_vi_blocks is not None:
        assert E.vi_blocks(A, blocks) == c.n_vi_blocks
    if c.n_templates is not None:
        assert (ntpl, trows) == (c.n_templates, c.template_rows)
    if c.gs_width is not None:
        assert E.chain_widths(A, 64) == (c.gs_width, c.gs_width) and n % 64 != 0
    if c.ell_wide:
        slabs, cells = E.ell_slabs(A, 64)
        assert cells >= E.GS_WIDE * slabs and ln.min() >= 130
    if c.n_values is not None:
        assert len(np.unique(bits(A.data))) == c.n_values
    nz = [int(A.indptr[b[1]] - A.indptr[b[0]]) for b in blocks]
    if name == "cap_nnz_exact":
        assert nz == [E.CAP, E.CAP] and set(ln) == {8}
    if name == "cap_nnz_plus1":
        assert blocks == [(0, 255), (255, 511), (511, 512)] and nz[1] == E.CAP
    if name == "cap_nnz_long_rows":
        assert [int(ln[r]) for r in (0, 1000, 2000, 3000, 4199)] == [2047, 2048, 2049, 4096, 4097]
        assert blocks[0] == (0, 2) and nz[0] == E.CAP and E.block_lines(A, blocks[0]) == 256
        assert all((r, r + 1) in blocks for r in (1000, 2000, 3000, 4199))
    if name == "cap_rows_gaps":
        assert nz[1] == 0 and nz[2] == 0 and nz[0] > 0
    if name == "cap_rows_nnz0":
        assert A.nnz == 0
    if name in ("cap_lines_256", "cap_lines_512"):
        assert blocks[0] == (0, 8) and E.block_lines(A, (0, 8), c.lw) == E.CAP // c.lw
        assert E.block_lines(A, (0, 9), c.lw) == E.CAP // c.lw + 1
    if name in ("cap_lines_257", "cap_lines_513"):
        assert blocks[0] == (0, 7) and E.block_lines(A, (0, 8), c.lw) == E.CAP // c.lw + 1
    if name == "cap_lines_long_row":
        assert (1200, 1201) in blocks and ln[1200] == 300 and E.block_lines(A, (1200, 1201)) == 300
        assert set(np.diff(A.indices[A.indptr[1200]:A.indptr[1201]])) == {8}
    if name == "vi_255_256_257":
        assert [E.block_values(A, b) for b in blocks] == [255, 256, 257]
    if name == "vi_signed_zero":
        assert [E.block_values(A, b) for b in blocks] == [256, 257]
        for b in blocks:
            v = A.data[A.indptr[b[0]]:A.indptr[b[1]]]
            z = bits(v[v == 0.0])
            assert set(z.tolist()) == {0, 1 << 63}
            assert len(np.unique(v)) == E.block_values(A, b) - 1  # equal as doubles
    if name == "vi_next_to_stream":
        assert E.block_values(A, blocks[0]) == 16 and E.block_values(A, blocks[1]) > 256
    if name == "odd_offsets":
        rp = A.indptr
        assert A.nnz % 2 == 1 and all(rp[g] % 2 == 1 for g in (256, 512, 768))
        assert all(x % 2 == 1 for x in ln[1:])
        for g in (256, 512):  # the 2048-entry chunk boundary of a full group falls inside a row
            edge = (rp[g] & ~1) + E.CAP
            assert rp[g + 256] > edge and edge not in set(rp.tolist())
    if name == "tpl_len_63_64_65":
        assert sorted(set(ln.tolist())) == [1, 63, 64, 65]
        assert tplf[:640].all() and not tplf[640:950].any() and tplf[950:].all()
    if name == "tpl_entries_1024":
        assert tplf[:512].all() and not tplf[512:].any()
    if name == "tpl_entries_1025":
        assert tplf[:512].all() and not tplf[512:].any() and set(ln[512:544]) == {64}
    if name == "tpl_shapes_300":
        assert tplf[:1020].all() and not tplf[1020:].any()


@pytest.mark.parametrize("name", NAMES)
def test_oracle_vs_exact_integers(oracle, name):
    """The oracle's spmv, spmv_add, residual, jacobi(0.5), norm and A @ A equal the int64
    references bit for bit."""
    c = E.zoo()[name]
    A, Ao = c.A, _orc(oracle, c.A)
    n = A.shape[0]
    x, y0, b = E.int_vectors(n, 7)
    assert _same(Ao.spmv(x), E.exact_spmv(A, x))
    assert _same(Ao.spmv_add(x, y0), E.exact_spmv_add(A, x, y0))
    assert _same(Ao.residual(x, b), E.exact_residual(A, x, b))
    rn, re = oracle.norm2(Ao.residual(x, b)), E.exact_residual_norm(A, x, b)
    assert abs(rn - re) <= 1e-12 * re
    if c.full_diag:
        assert _same(Ao.jacobi(x, b, 0.5), E.exact_jacobi(A, x, b))
    C = (Ao @ Ao).to_scipy()
    C.sort_indices()
    S = E.structural_product(A, A)
    assert np.array_equal(C.indptr, S.indptr) and np.array_equal(C.indices, S.indices)
    assert _same(C.data, E.exact_matmat(A, A, C).data.astype(np.float64))


@pytest.mark.parametrize("name", [m for m in NAMES if E.zoo()[m].full_diag])
def test_oracle_fixed_points(oracle, name):
    """b = A x in int64: jacobi and both hybrid GS sweeps return x bit for bit."""
    c = E.zoo()[name]
    Ao = _orc(oracle, c.A)
    x, _, _ = E.int_vectors(c.A.shape[0], 9)
    b = E.b_for_fixed_point(c.A, x)
    assert _same(Ao.jacobi(x, b, 2.0 / 3.0), x)
    for B in GS_BLOCKS:
        assert _same(Ao.hybrid_gs(x, b, B), x), B
        assert _same(Ao.hybrid_gs_backward(x, b, B), x), B


@pytest.mark.parametrize("name", NAMES)
def test_oracle_poisoned_columns(oracle, name):
    """x[c] = inf / nan: the rows that store no entry in column c keep the bits they have with
    x[c] = 0 (and the exact integers')."""
    c = E.zoo()[name]
    A, Ao = c.A, _orc(oracle, c.A)
    x, y0, b = E.int_vectors(A.shape[0], 11)
    for col in E.poison_columns(A):
        keep = E.rows_without(A, col)
        x0 = x.copy()
        x0[col] = 0.0
        want = (Ao.spmv(x0), Ao.spmv_add(x0, y0), Ao.residual(x0, b))
        assert _same(want[0], E.exact_spmv(A, x0))
        for bad in (np.inf, np.nan):
            xp = x.copy()
            xp[col] = bad
            got = (Ao.spmv(xp), Ao.spmv_add(xp, y0), Ao.residual(xp, b))
            for g, w in zip(got, want):
                assert _same(g[keep], w[keep]), (col, bad)
            if not keep.all():
                assert not np.isfinite(got[0][~keep]).any()


def _mutate(A, how):
    """(A', affected row): one value + 1, one entry dropped, or the values of two neighbouring
    entries of a row swapped (= their columns swapped), in a row of >= 3 entries."""
    A = A.copy()
    ln = np.diff(A.indptr)
    r = int(np.flatnonzero(ln >= 3)[len(np.flatnonzero(ln >= 3)) // 2])
    k = A.indptr[r] + 1
    if A.indices[k] == r:  # leave the diagonal alone
        k += 1
    if how == "value":
        A.data[k] += 1.0
    elif how == "swap":
        k2 = k + 1 if k + 1 < A.indptr[r + 1] and A.indices[k + 1] != r else k - 1
        assert A.data[k] != A.data[k2]
        A.data[[k, k2]] = A.data[[k2, k]]
    else:
        keep = np.ones(A.nnz, bool)
        keep[k] = False
        rp = A.indptr.copy()
        rp[r + 1:] -= 1
        A = sp.csr_matrix((A.data[keep], A.indices[keep], rp), shape=A.shape)
    return A, r


@pytest.mark.parametrize("how", ["value", "drop", "swap"])
@pytest.mark.parametrize("name", ["cap_nnz_plus1", "vi_255_256_257", "gs_chain_63", "odd_offsets"])
def test_references_have_teeth(oracle, name, how):
    """An operator that differs from the zoo's in one value, one entry or one swapped pair
    fails every matching exact check in the affected row (and only there)."""
    A = E.zoo()[name].A
    Am, r = _mutate(A, how)
    Ao = _orc(oracle, Am)
    n = A.shape[0]
    x, y0, b = E.int_vectors(n, 7)
    others = np.arange(n) != r
    for got, want in ((Ao.spmv(x), E.exact_spmv(A, x)),
                      (Ao.spmv_add(x, y0), E.exact_spmv_add(A, x, y0)),
                      (Ao.residual(x, b), E.exact_residual(A, x, b)),
                      (Ao.jacobi(x, b, 0.5), E.exact_jacobi(A, x, b))):
        assert bits(got)[r] != bits(want)[r]
        assert _same(got[others], want[others])
    bf = E.b_for_fixed_point(A, x)
    assert not _same(Ao.jacobi(x, bf, 2.0 / 3.0), x)
    for B in GS_BLOCKS:
        assert not _same(Ao.hybrid_gs(x, bf, B), x)
        assert not _same(Ao.hybrid_gs_backward(x, bf, B), x)
    C = (Ao @ Ao).to_scipy()
    C.sort_indices()
    S = E.structural_product(A, A)
    same_pattern = np.array_equal(C.indptr, S.indptr) and np.array_equal(C.indices, S.indices)
    assert not (same_pattern and _same(C.data, E.exact_matmat(A, A, C).data.astype(np.float64)))
