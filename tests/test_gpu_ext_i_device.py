"""Extended+i interpolation built on the device (setup_device.hip interp_ext_kernel and its
scratch form) and on any number of ranks: every level's A, P, R and split against the serial
oracle on bit patterns, on the PMIS operators of tests/setup_edge_cases.py, the capacity and
P_max gadgets of tests/ext_i_cases.py (proven on the CPU by tests/test_ext_i_cases_cpu.py) and
two stencils; the level query says the device path ran; cycles equal the oracle's bit for bit
and solve histories agree within the 1e-10 relative of DESIGN.md 3.

Cycles run on every operator but no_diagonal_neighbour, whose rows without a stored diagonal
make Jacobi divide by zero: it is set up and compared, never smoothed (as in
tests/test_gpu_setup_edges.py).  level_ext_stats tells how many rows took the global-scratch
path and how many launches a level needed, so the capacity and launch limits are observed."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import ext_i_cases as X
from tests import setup_edge_cases as E
from tests.setup_edge_cases import bits, same_bits
from tests.test_gpu_multirank import run_ranks
from tests.util import loopback_ctx, to_dev, to_host

pytestmark = pytest.mark.gpu

STENCILS = {"7pt_40x36x33": ("7pt", (40, 36, 33)), "27pt_20x18x22": ("27pt", (20, 18, 22)),
            "7pt_24x24x64": ("7pt", (24, 24, 64))}
STENCIL_OPTS = dict(strong_threshold=0.25, max_coarse=64)
_OPS = {}
_REF = {}


def operator(O, name):
    """(scipy A, pmis options, cuts) of a zoo case, an ext_i case or a stencil; built once."""
    if name not in _OPS:
        if name in STENCILS:
            kind, dims = STENCILS[name]
            A = sp.csr_matrix({"7pt": O.gen_7pt, "27pt": O.gen_27pt}[kind](*dims).to_scipy())
            n = A.shape[0]
            cuts = {ws: [0] + [n * (r + 1) // ws - 5 * (ws - 1 - r) for r in range(ws - 1)] for ws in (2, 3)}
            _OPS[name] = (A, STENCIL_OPTS, cuts)
        else:
            c = X.cases()[name] if name in X.cases() else E.zoo()[name]
            _OPS[name] = (c.A, c.pmis, c.cuts)
    return _OPS[name]


def _orc(O, M):
    M = sp.csr_matrix(M)
    return O.Csr.from_arrays(M.shape[0], M.shape[1], M.indptr, M.indices, M.data)


def reference(O, name, p_max):
    """The oracle's extended+i hierarchy, computed once and shared (read-only)."""
    key = (name, p_max)
    if key not in _REF:
        A, opts, _ = operator(O, name)
        H = O.Hierarchy(_orc(O, A), interp=O.INTERP_EXT_I, p_max=p_max, **opts)
        levels = []
        for l in range(H.num_levels):
            lev = {"A": H.matrix(l, "A")}
            if l + 1 < H.num_levels:
                lev.update(P=H.matrix(l, "P"), R=H.matrix(l, "R"), split=H.split(l))
            levels.append(lev)
        _REF[key] = (H, levels)
    return _REF[key]


def _dev(ra, ctx, M, lo=0, hi=None):
    hi = M.shape[0] if hi is None else hi
    L = M[lo:hi]
    return ra.ParCSRMatrix.from_csr(ctx, M.shape[0], lo, L.indptr, L.indices, L.data)


def _solver(ra, opts, p_max, **kw):
    return ra.ParMultilevel(coarsen="pmis", smoother="jacobi", interp="ext+i", p_max=p_max, **dict(opts, **kw))


def _levels_of(ml):
    out = []
    for l in range(ml.num_levels):
        d = {}
        for w in ("APR" if l + 1 < ml.num_levels else "A"):
            M = ml.level_matrix(l, w)
            d[w] = (M.first_row, M.to_scipy_local())
        if l + 1 < ml.num_levels:
            d["split"] = ml.level_split(l)
            d["dev"] = ml.level_setup_on_device(l)
        out.append(d)
    return out


def _check_levels(got, levels, tag, on_device):
    assert len(got) == len(levels), (tag, len(got), len(levels))
    for l, d in enumerate(got):
        for w in ("APR" if "P" in d else "A"):
            f, M = d[w]
            assert same_bits(M, levels[l][w][f:f + M.shape[0]]), (tag, l, w)
        if "split" in d:
            f, M = d["A"]
            assert np.array_equal(d["split"], levels[l]["split"][f:f + M.shape[0]]), (tag, l, "split")
            assert d["dev"] == on_device, (tag, l, "level_setup_on_device")


ONE_RANK = E.names("pmis") + X.names() + ["7pt_40x36x33", "27pt_20x18x22"]


@pytest.mark.parametrize("p_max", [4, 0])
@pytest.mark.parametrize("name", ONE_RANK)
def test_ext_i_one_rank(ctx, oracle, monkeypatch, name, p_max):
    """setup_device 1 (every level's strength, PMIS and extended+i on the device: the level
    query says so) and 0 (host): all levels' A, P, R and split equal the oracle's."""
    import raptor_amd as ra

    monkeypatch.delenv("AMG_INTERP_WAVE_NPR", raising=False)
    A, opts, _ = operator(oracle, name)
    _, levels = reference(oracle, name, p_max)
    dA = _dev(ra, ctx, A)
    for m in (1, 0):
        ml = _solver(ra, opts, p_max, setup_device=m, use_graph=False).setup(dA)
        _check_levels(_levels_of(ml), levels, (name, m), 1 if m == 1 else 0)
        del ml


def test_level_query_rejects_the_coarsest_level(ctx, oracle):
    import raptor_amd as ra

    A, opts, _ = operator(oracle, "ext_pmax_edge")
    ml = _solver(ra, opts, 4).setup(_dev(ra, ctx, A))
    assert ml.num_levels >= 2 and ml.level_setup_on_device(0) == 1
    with pytest.raises(ra.AmgError):
        ml.level_setup_on_device(ml.num_levels - 1)
    rs = ra.ParMultilevel(coarsen="rs", smoother="jacobi", interp="ext+i", **opts).setup(_dev(ra, ctx, A))
    assert rs.num_levels >= 2 and rs.level_setup_on_device(0) == 0


@pytest.mark.parametrize("name", ["ext_capacity", "ext_pmax_edge", "hub"])
def test_scratch_path_takes_the_rows_over_the_capacity(ctx, oracle, name):
    """The device reports how many rows of level 0 it built through global scratch: exactly
    the rows with more than K_EXT_CAP members of C^_i or strong neighbours, read off the oracle's
    strength and split (one for ext_capacity: the 257-member hub; none for ext_pmax_edge; the
    long hub rows of the zoo's hub operator).  A changed kernel capacity fails here."""
    import raptor_amd as ra

    O = oracle
    A, opts, _ = operator(O, name)
    Ao = _orc(O, A)
    S = O.strength_classical(Ao, opts["strong_threshold"])
    cf = O.pmis_split(S, 0x5EED)
    want = X.scratch_rows(A, S.to_scipy(), cf)
    assert (len(want) > 0) == (name != "ext_pmax_edge")
    ml = _solver(ra, opts, 4, use_graph=False).setup(_dev(ra, ctx, A))
    st = ml.level_ext_stats(0)
    assert st["scratch_rows"] == len(want), (st, want)
    assert st["launches"] == 1
    host = _solver(ra, opts, 4, setup_device=0, use_graph=False).setup(_dev(ra, ctx, A))
    assert host.level_ext_stats(0) == {"scratch_rows": 0, "launches": 0}


def test_rows_beyond_one_launch(ctx, oracle):
    """7-pt 72 x 64 x 64 (294,912 rows): the wave-per-row kernel takes level 0 in more than one
    launch (a grid dimension cannot hold 64 threads for each of 2^26 rows, so launches cover a
    fixed number of rows); the rows of every launch equal the oracle's."""
    import raptor_amd as ra

    O = oracle
    Ao = O.gen_7pt(72, 64, 64)
    A = sp.csr_matrix(Ao.to_scipy())
    Ho = O.Hierarchy(Ao, interp=O.INTERP_EXT_I, p_max=4, **STENCIL_OPTS)
    ml = _solver(ra, STENCIL_OPTS, 4, use_graph=False).setup(_dev(ra, ctx, A))
    st = ml.level_ext_stats(0)
    assert st["launches"] >= 2 and st["scratch_rows"] == 0, st
    assert ml.num_levels == Ho.num_levels
    for l in range(Ho.num_levels - 1):
        assert ml.level_setup_on_device(l) == 1
        for w in "APR":
            assert same_bits(ml.level_matrix(l, w).to_scipy_local(), Ho.matrix(l, w)), (l, w)
        assert np.array_equal(ml.level_split(l), Ho.split(l)), l


# every one-rank operator but no_diagonal_neighbour: its rows without a stored diagonal make
# Jacobi divide by zero, so it is set up and compared above, never smoothed (as in
# tests/test_gpu_setup_edges.py)
CYCLES = [n for n in ONE_RANK if n != "no_diagonal_neighbour"]


@pytest.mark.parametrize("p_max", [4, 0])
@pytest.mark.parametrize("name", CYCLES)
def test_ext_i_cycles_one_rank(ctx, oracle, name, p_max):
    """Three cycles bit-identical to the oracle's on its own hierarchy; an 8-cycle history
    within 1e-10 relative."""
    import raptor_amd as ra

    O = oracle
    A, opts, _ = operator(O, name)
    Ho, levels = reference(O, name, p_max)
    ml = _solver(ra, opts, p_max).setup(_dev(ra, ctx, A))
    _check_levels(_levels_of(ml), levels, name, 1)
    n = A.shape[0]
    b = _orc(O, A).spmv(O.vec_uniform(n, 42))
    db, dx, xo = to_dev(ctx, b), ctx.zeros(n), np.zeros(n)
    for it in range(3):
        ml.cycle(dx, db)
        xo = Ho.cycle(xo, b)
        assert np.array_equal(bits(to_host(ctx, dx)), bits(xo)), it
    _, hist = ml.solve(ctx.zeros(n), db, max_iter=8)
    _, hist_o = Ho.solve(np.zeros(n), b, max_iter=8)
    assert hist.size == hist_o.size == 9
    assert np.all(np.abs(hist - hist_o) <= 1e-10 * hist_o)


RANKS = [(n, nr) for n in ["mixed_600", "mixed_2500", "negative_diagonal", "sk_zero", "hub"] + X.names() +
         ["7pt_40x36x33", "27pt_20x18x22"] for nr in (2, 3)]


def _rank_body(ra, O, name, starts, b, grid=None):
    A, opts, _ = operator(O, name)

    def rank(r, nr, world):
        ctx = loopback_ctx(r, nr, world)
        dA = ra.par_stencil_grid(ctx, *grid) if grid else _dev(ra, ctx, A, starts[r], starts[r + 1])
        f, m = dA.first_row, dA.local_rows
        out = {}
        for rep, mode in ((0, 1), (0, 0), (800, 1), (10 ** 9, 1)):
            ml = _solver(ra, opts, 4, setup_device=mode, replicate_below=rep, use_graph=False).setup(dA)
            xs = []
            if mode == 1:
                db, dx = to_dev(ctx, b[f:f + m]), ctx.zeros(m)
                for _ in range(2):
                    ml.cycle(dx, db)
                    xs.append(to_host(ctx, dx))
            out[(rep, mode)] = (_levels_of(ml), xs)
            del ml
        return f, m, out

    return rank


def _check_ranks(res, Ho, levels, b, name):
    xo, ref_x = np.zeros(b.size), []
    for _ in range(2):
        xo = Ho.cycle(xo, b)
        ref_x.append(xo)
    for r, (f, m, out) in enumerate(res):
        for (rep, mode), (got, xs) in out.items():
            _check_levels(got, levels, (name, r, rep, mode), 1 if mode == 1 else 0)
            for it, x in enumerate(xs):
                assert np.array_equal(bits(x), bits(ref_x[it][f:f + m])), (name, r, rep, it)
        # the device path equals the host path
        for d1, d0 in zip(out[(0, 1)][0], out[(0, 0)][0]):
            for w in ("APR" if "P" in d1 else "A"):
                assert same_bits(d1[w][1], d0[w][1])


@pytest.mark.parametrize("name,nranks", RANKS, ids=[f"{n}-{nr}" for n, nr in RANKS])
def test_ext_i_loopback_ranks(oracle, name, nranks):
    """2 and 3 loopback ranks on ragged cuts (through hub neighbourhoods and gadgets: ghost
    strong F neighbours whose strong C neighbours lie two halos deep), replicate_below 0, 800
    and 1e9: each rank's slice of every level equals the oracle's, the device path equals the
    host path, and two cycles are bit-identical to the oracle's."""
    import raptor_amd as ra

    O = oracle
    A, opts, cuts = operator(O, name)
    Ho, levels = reference(O, name, 4)
    n = A.shape[0]
    starts = list(cuts[nranks]) + [n]
    b = _orc(O, A).spmv(O.vec_uniform(n, 42))
    res = run_ranks(nranks, _rank_body(ra, O, name, starts, b))
    _check_ranks(res, Ho, levels, b, name)


def test_ext_i_eight_loopback_ranks(oracle):
    """Eight z-slabs of 7-pt 24 x 24 x 64 (the multi-GPU configuration's partition shape)."""
    import raptor_amd as ra

    O = oracle
    name = "7pt_24x24x64"
    A, opts, _ = operator(O, name)
    Ho, levels = reference(O, name, 4)
    b = _orc(O, A).spmv(O.vec_uniform(A.shape[0], 42))
    res = run_ranks(8, _rank_body(ra, O, name, None, b, grid=STENCILS[name]))
    _check_ranks(res, Ho, levels, b, name)
