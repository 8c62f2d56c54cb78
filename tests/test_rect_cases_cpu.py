"""The rectangular zoo (tests/rect_cases.py) on the CPU: every case's hand-derived claims against
the restated build rules, the oracle's spmv / spmv_add on rectangular input against exact int64
references bit for bit, poisoned columns, and a sensitivity check that the references notice one
changed value, one dropped entry and one column moved across a band edge.  No GPU."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import edge_cases as E
from tests import rect_cases as R
from tests.edge_cases import bits

NAMES = R.zoo_names()


def _orc(O, A):
    return O.Csr.from_arrays(A.shape[0], A.shape[1], A.indptr, A.indices, A.data)


def _same(a, b):
    return np.array_equal(bits(a), bits(b))


def _vectors(A, seed):
    """Integer-valued x (n_cols) and y0 (n_rows)."""
    return E.int_vectors(A.shape[1], seed)[0], E.int_vectors(A.shape[0], seed + 1)[1]


@pytest.mark.parametrize("name", NAMES)
def test_builder_claims(name):
    """What each builder's docstring derives by hand, against plan()'s restatement of
    par_matrix.hip: rows per block, tile or gather, line width, block count, entries and bands
    per block, value-indexed blocks, column codes."""
    c = R.zoo()[name]
    A = c.A
    nr, nc = A.shape
    assert nr != nc and c.doc and "block" in c.doc.lower()
    if A.nnz:
        E._int(A.data)
        assert np.abs(A.data).max() <= 1 << 11
        assert A.indices.max() < nc
    ln = np.diff(A.indptr)
    for i in np.flatnonzero(ln > 1):
        assert np.all(np.diff(A.indices[A.indptr[i]:A.indptr[i + 1]]) > 0)
    p = R.plan(A, c.env)
    assert p["rpb"] == c.rpb == (4 if A.nnz <= 4 * nr else 1)
    assert p["tiled"] == c.tiled and p["tile_line_bytes"] == c.tile_line_bytes
    assert len(p["blocks"]) == c.n_blocks, (len(p["blocks"]), p["blocks"][:12])
    assert p["n_vi"] == c.n_vi_blocks
    assert p["c16"] == c.c16
    if c.block_nnz is not None:
        assert p["nnz"] == c.block_nnz
    if c.bands is not None:
        assert p["bands"] == c.bands
    # every block respects the caps of its path, or is a single row
    for b, z, lines in zip(p["blocks"], p["nnz"], p["lines"]):
        assert b[1] - b[0] <= 256 * c.rpb
        assert z <= E.CAP or b[1] - b[0] == 1
        assert not c.tiled or lines <= E.CAP // p["lw"] or b[1] - b[0] == 1
    if nc > 1 and A.nnz and c.group not in ("tile_width", "bands", "long"):
        assert A.indices.max() == nc - 1, "the last column is used"
    # what each group is about
    if name == "slots_512_to_2048":
        assert p["slots"] == [2, 4, 4, 8, 8] and A.indices[-1] == nc - 1
        assert [R.gather_slots(z) for z in (512, 513, 1024, 1025, 2048)] == [2, 4, 4, 8, 8]
    if name == "rpb4_rows":
        assert [b[1] - b[0] for b in p["blocks"]] == [1023, 1024, 1024, 512, 1024, 1]
        assert set(ln.tolist()) == {0, 1, 4} and set(ln[3071:3583].tolist()) == {4}
    if c.group == "empty" and name != "empty_nnz0":
        q = p["blocks"][1]
        assert p["nnz"][1] == 0 and q[1] - q[0] == 256 * c.rpb and p["nnz"][0] > 0 and p["nnz"][2] > 0
    if name == "empty_nnz0":
        assert A.nnz == 0
    if c.group == "long":
        for r in c.long_rows:
            assert (r, r + 1) in p["blocks"]
        if name != "long_untiled_row":
            assert [int(ln[r]) for r in c.long_rows] == [2049, 4097]
            assert len(R.block_bands(A, (513, 514))) == 5   # skipped by the rule: over 2048 entries
        else:
            q = p["blocks"].index((256, 257))
            assert p["nnz"][q] == 257 and p["lines"][q] == 257
    if name == "long_gather":
        assert all(0 < t <= 4 for t, z in zip(p["bands"], p["nnz"]) if z <= E.CAP)
    if c.group == "bands":
        b0 = R.block_bands(A, p["blocks"][0])
        cols0 = A.indices[:A.indptr[256]]
        if name == "bands_offset_16383":
            assert b0 == [1000] and cols0.max() - 1000 == R.BAND - 1
        if name == "bands_offset_16384":
            assert b0 == [1000, 1000 + R.BAND]
        if name in ("bands_four", "bands_five"):
            assert all(b + R.BAND - 1 in cols0 for b in b0[:4]) and cols0.min() == 0
            assert A.indices.max() == nc - 1
    if name == "vi_slots":
        assert [R.n_values(A, b) for b in p["blocks"]] == [255, 257, 256] * 3 + [1]
        assert p["slots"] == [2] * 3 + [4] * 3 + [8] * 3 + [2]
        for q in (2, 5, 8):
            b = p["blocks"][q]
            v = A.data[A.indptr[b[0]]:A.indptr[b[1]]]
            assert set(bits(v[v == 0.0]).tolist()) == {0, 1 << 63}
    if c.group == "tile_rule":
        s8 = R.cut(A, 256 * c.rpb, 8, True)
        lines = sum(min(x, 257) for _, x in s8)
        assert (2 * lines == A.nnz) if c.tiled else (2 * lines == A.nnz + 2)
    if c.group == "tile_width":
        s8 = R.cut(A, 256 * c.rpb, 8, True)
        lines = sum(x for _, x in s8)
        assert 4 * lines == 3 * 256 * len(s8) - (0 if c.tile_line_bytes == 32 else 4)
        if c.tile_line_bytes == 32:
            assert p["lines"][0] == 512
            assert len(set(R.line_of(A.indices[:A.indptr[513]], nc, 4).tolist())) == 513
    if name == "tile_rpb4_caps":
        assert [b[1] - b[0] for b in p["blocks"]] == [256, 1024, 512, 10]
        assert p["lines"] == [256, 128, 129, 2]
    if c.group == "narrow":
        assert nc in (1, 2, 3, 7, 9, 257) and p["blocks"] == [(0, 1024), (1024, 1030)]


def test_plan_environment_knobs():
    """AMG_RECT_TILE forces the choice both ways and AMG_GATHER_C16=0 clears the codes; the
    forced plans are what the GPU tests assert under those knobs."""
    c = R.zoo()["slots_512_to_2048"]
    assert not R.plan(c.A, {"AMG_GATHER_C16": "0"})["c16"]
    t = R.plan(c.A, {"AMG_RECT_TILE": "1"})
    assert t["tiled"] and not t["c16"] and t["tile_line_bytes"] in (32, 64)
    assert all(x <= E.CAP // t["lw"] for x in t["lines"])
    n = R.zoo()["narrow_9"]
    g = R.plan(n.A, {"AMG_RECT_TILE": "0"})
    assert not g["tiled"] and g["c16"] and g["blocks"] == [(0, 1024), (1024, 1030)]


@pytest.mark.parametrize("name", NAMES)
def test_oracle_vs_exact_integers(oracle, name):
    """The oracle's spmv and spmv_add on rectangular input equal the int64 references bit for
    bit; an empty row gives +0.0 and leaves y0's bits."""
    A = R.zoo()[name].A
    Ao = _orc(oracle, A)
    assert Ao.shape == A.shape
    x, y0 = _vectors(A, 7)
    y, ya = Ao.spmv(x), Ao.spmv_add(x, y0)
    assert _same(y, E.exact_spmv(A, x))
    assert _same(ya, E.exact_spmv_add(A, x, y0))
    empty = np.diff(A.indptr) == 0
    assert np.all(bits(y)[empty] == 0) and _same(ya[empty], y0[empty])


@pytest.mark.parametrize("name", NAMES)
def test_oracle_poisoned_columns(oracle, name):
    """x[c] = inf / nan: rows without an entry in column c keep the bits they have with
    x[c] = 0 (the exact integers')."""
    c = R.zoo()[name]
    A, Ao = c.A, _orc(oracle, c.A)
    x, y0 = _vectors(A, 11)
    for col in R.poison_columns(c):
        keep = E.rows_without(A, col)
        x0 = x.copy()
        x0[col] = 0.0
        want = (E.exact_spmv(A, x0), E.exact_spmv_add(A, x0, y0))
        for bad in (np.inf, np.nan):
            xp = x.copy()
            xp[col] = bad
            got = (Ao.spmv(xp), Ao.spmv_add(xp, y0))
            for g, w in zip(got, want):
                assert _same(g[keep], w[keep]), (col, bad)
            hit = ~keep & (np.asarray(abs(A).tocsc()[:, col].todense()).ravel() > 0)
            assert not np.isfinite(got[0][hit]).any()


TEETH = [("slots_512_to_2048", "value"), ("slots_512_to_2048", "drop"), ("rpb4_rows", "value"),
         ("rpb4_rows", "drop"), ("bands_four", "value"), ("bands_four", "drop"), ("bands_four", "band"),
         ("bands_offset_16383", "band")]


@pytest.mark.parametrize("name,how", TEETH)
def test_references_have_teeth(oracle, name, how):
    """An operator that differs from the zoo's in one value, one entry or one column moved across
    a band edge differs from the exact references in the affected row, and only there."""
    A = R.zoo()[name].A
    Am, r = R.mutate(A, how)
    Ao = _orc(oracle, Am)
    x, y0 = _vectors(A, 7)
    others = np.arange(A.shape[0]) != r
    for got, want in ((Ao.spmv(x), E.exact_spmv(A, x)), (Ao.spmv_add(x, y0), E.exact_spmv_add(A, x, y0))):
        assert bits(got)[r] != bits(want)[r]
        assert _same(got[others], want[others])
    if how == "band":   # the moved column opens one more band in its block
        assert len(R.block_bands(Am, (0, 256))) == len(R.block_bands(A, (0, 256))) + 1


def test_rank_case_claims(oracle):
    """The several-rank operators: partitions, halo sizes, the band that straddles the local |
    halo boundary, the block that fills a tile with local and halo lines, the missing owners --
    and each rank's local view times its [local | halo] x equals the serial result's slice."""
    Z = R.rank_cases()
    for c in Z.values():
        assert c.doc and c.row_starts[-1] == c.A.shape[0] and c.col_starts[-1] == c.A.shape[1]
        x = oracle.vec_uniform(c.A.shape[1], 5)
        want = _orc(oracle, c.A).spmv(x)
        for r in range(len(c.row_starts) - 1):
            G, L, ncl, halo, cls = R.local_view(c, r)
            xl = np.concatenate([x[c.col_starts[r]:c.col_starts[r + 1]], x[halo]])
            assert _same(_orc(oracle, L).spmv(xl), want[c.row_starts[r]:c.row_starts[r + 1]])
    c = Z["band_across_halo"]
    for r, nh in ((0, 1), (1, 2)):
        G, L, ncl, halo, cls = R.local_view(c, r)
        p = R.plan(L, {}, ncl, cls)
        assert ncl % 2 == 1 and halo.size == nh and p["rpb"] == 1 and not p["tiled"] and p["c16"]
        assert p["blocks"] == [(0, 256), (256, 512)] and not cls[:256].any() and cls[256:].all()
        base = R.block_bands(L, (256, 512))
        cols = L.indices[L.indptr[256]:]
        assert len(base) == 2 and base[1] < ncl <= cols.max() == ncl + nh - 1 < base[1] + R.BAND
    c = Z["tiled_halo_tail"]
    for r in (0, 1):
        G, L, ncl, halo, cls = R.local_view(c, r)
        p = R.plan(L, {}, ncl, cls)
        assert ncl % 8 in (1, 7) and p["tiled"] and p["tile_line_bytes"] == 64 and p["rpb"] == 1
        assert p["blocks"] == [(0, 256), (256, 384), (384, 385)] and p["lines"] == [64, 256, 3]
        lines = R.line_of(L.indices[L.indptr[256]:L.indptr[384]], ncl, 8)
        hl0 = -(-ncl // 8)
        assert (lines < hl0).any() and lines.max() == hl0 + 127 and lines[lines >= hl0].min() == hl0
        last = L.indices[L.indptr[384]:]
        assert ncl - 1 in last and ncl + 1024 in last
    c = Z["missing_owners"]
    v = [R.local_view(c, r) for r in range(3)]
    assert v[0][2] == 0 and v[0][0].shape[0] == 300 and v[0][4].all()      # rows, no columns
    assert v[2][0].shape[0] == 0 and v[2][2] == 500 and v[2][3].size == 0  # columns, no rows
    assert v[1][3].size > 0 and v[1][4].all()                              # both, every row reads the halo
