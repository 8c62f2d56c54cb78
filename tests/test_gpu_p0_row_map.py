"""Segment row map of P_0's cycle copy: where the cycle runs level 1 in brick
order and level 0 in the hierarchy's order, P_0 is stored with its rows in S x 8 x 8 bricks of
the rank's grid and reads / writes y through a per-block list of segment rows.  The map is a
storage detail: `P_cycle` takes and returns level-0 rows in vector order, every row keeps its
entries in the hierarchy's order, so every result is what it was bit for bit.  Checked for every
S (AMG_P0_ROWMAP) and both x-tile line widths: y += P e and y = P e against AMG_P0_ROWMAP=0 and
the oracle CSR, three cycles and an 8-iteration PCG against the oracle hierarchy,
AMG_P0_ROWMAP=0 and AMG_CYCLE_ORDER=0, and the host and device format builders' digests."""
import numpy as np
import pytest

from tests.test_gpu_cycle_order import _cycles
from tests.util import oracle_levels, to_dev, to_host

pytestmark = pytest.mark.gpu

DEFAULT_S = 16  # CycleOrder::kP0Seg

# case -> (stencil, dims, coarsening); x extents: 32 (every S), 48 (8 and 16), 30 (none), 160 (every S)
CASES = {
    "7pt-pmis-32x24x24": ("7pt", (32, 24, 24), "pmis"),   # last block partial
    "7pt-pmis-48x40x36": ("7pt", (48, 40, 36), "pmis"),   # z = 36: half-height bricks; S = 32 falls back
    "7pt-pmis-30x26x22": ("7pt", (30, 26, 22), "pmis"),   # no S divides 30: P_0 as without the map
    "7pt-sa-48x40x36": ("7pt", (48, 40, 36), "sa"),       # longer P rows, one row per lane
    "5pt-rs-160x144": ("5pt", (160, 144), "rs"),          # bricks of 8 x 8 x 1
}


def _solver(ra, coarsen, **kw):
    if coarsen == "sa":
        return ra.ParSmoothedAggregationSolver(smoother="jacobi", **kw)
    return ra.ParRugeStubenSolver(coarsen=coarsen, **kw)


def _expected_seg(dims, S):
    return S if S and dims[0] % S == 0 else 0


def _frozen(a):
    a = np.array(a)
    a.setflags(write=False)
    return a


_ORACLE = {}


def _oracle_ref(O, case, ml, b):
    """Three oracle cycles on the hierarchy's exported operators: once per case (the hierarchy
    does not depend on the storage knobs), shared by the line widths."""
    if case not in _ORACLE:
        H = O.Hierarchy(None, levels=oracle_levels(O, ml))
        xs, x = [], np.zeros(b.size)
        for _ in range(3):
            x = H.cycle(x, b)
            xs.append(_frozen(x))
        _ORACLE[case] = xs
    return _ORACLE[case]


def _apply_both(ctx, P, e, y0):
    """(y0 + P e, P e) from the device, y prefilled with y0."""
    dy = to_dev(ctx, y0)
    P.mult_add(to_dev(ctx, e), dy)
    dz = to_dev(ctx, y0)  # mult overwrites every row: a skipped row keeps its y0 value
    P.mult(to_dev(ctx, e), dz)
    return to_host(ctx, dy), to_host(ctx, dz)


@pytest.mark.parametrize("line", ["4", "8"], ids=["lines32", "lines64"])
@pytest.mark.parametrize("case", list(CASES))
def test_p0_row_map_bit_identical(ctx, oracle, monkeypatch, case, line):
    import raptor_amd as ra

    O = oracle
    kind, dims, coarsen = CASES[case]
    monkeypatch.setenv("AMG_TILE_LINE", line)
    A = ra.par_stencil_grid(ctx, kind, dims)
    n = A.local_rows
    b = O.vec_uniform(n, 31)
    db = to_dev(ctx, b)

    def setup(S):
        if S is None:
            monkeypatch.delenv("AMG_P0_ROWMAP", raising=False)
        else:
            monkeypatch.setenv("AMG_P0_ROWMAP", str(S))
        return _solver(ra, coarsen).setup(A)

    # today's form: the reference of every comparison below
    ml0 = setup(0)
    assert ml0.level_matrix(1, "A").local_rows >= 4096  # level 1 runs in brick order
    P0 = ml0.level_matrix(0, "P_cycle")
    assert P0.info["row_seg"] == 0
    m1 = P0.info["n_local_cols"]
    e, y0 = O.vec_uniform(m1, 7), O.vec_uniform(n, 8)
    assert np.unique(y0).size == n  # distinct prefill: a row written twice or skipped shows
    ex0 = P0.export()
    Pe = O.Csr.from_arrays(n, m1, *ex0).spmv(e)
    add0, mul0 = _apply_both(ctx, P0, e, y0)
    assert np.array_equal(add0, y0 + Pe) and np.array_equal(mul0, Pe)
    dig0 = P0.format_digest()
    xs0 = _cycles(ctx, ml0, db, n, 3)

    for S in (None, 8, 16, 32):
        ml = setup(S)
        P = ml.level_matrix(0, "P_cycle")
        inf = P.info
        assert inf["row_seg"] == _expected_seg(dims, DEFAULT_S if S is None else S), (S, inf["row_seg"])
        assert inf["tile_line_bytes"] == 8 * int(line)
        # the map is a storage detail: the operator's rows are the vector's for every caller
        ex = P.export()
        assert all(np.array_equal(u, v) for u, v in zip(ex, ex0)), S
        add, mul = _apply_both(ctx, P, e, y0)
        assert np.array_equal(add, add0) and np.array_equal(add, y0 + Pe), ("mult_add", S)
        assert np.array_equal(mul, mul0) and np.array_equal(mul, Pe), ("mult", S)
        if inf["row_seg"] == 0:  # fallback: P_0 is built as without the knob
            assert P.format_digest() == dig0, S
            assert inf["mult_add_bytes"] == P0.info["mult_add_bytes"]
        if S is not None:
            continue
        # the default S: cycles and PCG against the oracle, today's form and the natural order
        xs = _cycles(ctx, ml, db, n, 3)
        xo = _oracle_ref(O, case, ml, b)
        for k in range(3):
            assert np.array_equal(xs[k], xo[k]), ("oracle cycle", k)
            assert np.array_equal(xs[k], xs0[k]), ("AMG_P0_ROWMAP=0", k)
        monkeypatch.setenv("AMG_CYCLE_ORDER", "0")
        mln = _solver(ra, coarsen).setup(A)
        monkeypatch.delenv("AMG_CYCLE_ORDER")
        assert mln.level_matrix(0, "P_cycle").info["row_seg"] == 0
        for k, x in enumerate(_cycles(ctx, mln, db, n, 3)):
            assert np.array_equal(x, xs[k]), ("AMG_CYCLE_ORDER=0", k)
        runs = []
        for m in (ml, ml0, mln):
            x = ctx.zeros(n)
            _, h = m.pcg(x, db, max_iter=8)
            runs.append((to_host(ctx, x), h))
        for x, h in runs[1:]:
            assert np.array_equal(x, runs[0][0]) and np.array_equal(h, runs[0][1])
        # host and device format builders: the same bytes, the segment rows included
        if inf["row_seg"]:
            digs = []
            for dev in ("1", "0"):
                monkeypatch.setenv("AMG_DEVICE_FORMATS", dev)
                Pd = setup(None).level_matrix(0, "P_cycle")
                assert Pd.info["row_seg"] == inf["row_seg"]
                digs.append(Pd.format_digest())
            monkeypatch.delenv("AMG_DEVICE_FORMATS")
            assert digs[0] == digs[1]


@pytest.mark.parametrize("line", ["4", "8"], ids=["lines32", "lines64"])
def test_p0_row_map_two_ranks(ctx, monkeypatch, line):
    """Two loopback ranks (z-slabs of 32 x 24 x 16), each ordering its own rows of P_0: every
    rank's slice of three V-cycles equals the one-rank iterate."""
    import raptor_amd as ra
    from tests.test_gpu_multirank import run_ranks
    from tests.util import loopback_ctx

    monkeypatch.setenv("AMG_TILE_LINE", line)
    dims = (32, 24, 32)
    A = ra.par_stencil_grid(ctx, "7pt", dims)
    n = A.local_rows
    ml = ra.ParRugeStubenSolver(coarsen="pmis").setup(A)
    assert ml.level_matrix(0, "P_cycle").info["row_seg"] == DEFAULT_S
    b = np.random.default_rng(3).uniform(-1.0, 1.0, n)
    ref = _cycles(ctx, ml, to_dev(ctx, b), n, 3)

    def body(r, nr, world):
        c = loopback_ctx(r, nr, world)
        Ar = ra.par_stencil_grid(c, "7pt", dims)
        f, m = Ar.first_row, Ar.local_rows
        # level 1 (about half the points) stays distributed, so it runs in brick order
        mr = ra.ParRugeStubenSolver(coarsen="pmis", replicate_below=4096).setup(Ar)
        seg = mr.level_matrix(0, "P_cycle").info["row_seg"]
        return f, m, seg, _cycles(c, mr, to_dev(c, b[f:f + m]), m, 3)

    for f, m, seg, xs in run_ranks(2, body):
        assert seg == DEFAULT_S
        for k in range(3):
            assert np.array_equal(xs[k], ref[k][f:f + m]), ("cycle", k, f)
