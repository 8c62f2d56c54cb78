"""The rectangular-operator paths of csr_block_kernel on operators that sit exactly on their
limits (tests/rect_cases.py), built through amg_par_csr_create_rect and checked as the square
zoo is (tests/test_gpu_kernel_edges.py): the path each case names asserted through
ParCSRMatrix.info, then mult and mult_add against the CPU oracle, against exact int64
arithmetic and with poisoned columns -- every comparison on bit patterns.

Per case the storage formats auto, blocks and csr run on one handle, under the case's own
environment and -- unless the case is about the automatic choice -- with the 16-bit column
codes off (AMG_GATHER_C16=0) and the tile-or-gather choice forced both ways (AMG_RECT_TILE);
under a forced knob the expected path is rect_cases.plan's, the restated build rules that
tests/test_rect_cases_cpu.py checks the hand-derived claims against."""
import numpy as np
import pytest

from tests import edge_cases as E
from tests import rect_cases as R
from tests.edge_cases import bits
from tests.test_gpu_multirank import run_ranks
from tests.util import loopback_ctx, native_mode, to_dev, to_host

pytestmark = pytest.mark.gpu

NAMES = R.zoo_names()
FORMATS = ("auto", "blocks", "csr")
ZOO_RUNS = [(name, e) for name in NAMES for e in R.run_envs(R.zoo()[name])]
KV_GATHER, KV_C16 = 4, 256
AMG_ERR_INVALID = 1


def _same(a, b):
    return np.array_equal(bits(a), bits(b))


def _diff(a, b):
    return np.flatnonzero(bits(a) != bits(b))


def _orc(O, A):
    return O.Csr.from_arrays(A.shape[0], A.shape[1], A.indptr, A.indices, A.data)


def _dev(ra, ctx, A):
    """One rank: every row and every column is local."""
    return ra.ParCSRMatrix.from_csr_rect(ctx, A.shape, 0, 0, A.shape[1], A.indptr, A.indices, A.data)


def _up(ctx, a):
    return to_dev(ctx, np.array(a, np.float64))


def _setenv(monkeypatch, *envs):
    for env in envs:
        for k, v in env.items():
            monkeypatch.setenv(k, v)


_REFS = {}


def _refs(O, name):
    """Per case, computed once and shared (read-only): the oracle's results on vec_uniform data,
    the exact int64 results on int_vectors data, and the oracle's results per poisoned column."""
    if name in _REFS:
        return _REFS[name]
    c = R.zoo()[name]
    A, Ao = c.A, _orc(O, c.A)
    nr, nc = A.shape
    u = dict(x=O.vec_uniform(nc, 3), y0=O.vec_uniform(nr, 5))
    u.update(mult=Ao.spmv(u["x"]), mult_add=Ao.spmv_add(u["x"], u["y0"]))
    ix, iy0 = E.int_vectors(nc, 7)[0], E.int_vectors(nr, 8)[1]
    e = dict(x=ix, y0=iy0, mult=E.exact_spmv(A, ix), mult_add=E.exact_spmv_add(A, ix, iy0))
    px, py0 = O.vec_uniform(nc, 11), O.vec_uniform(nr, 13)
    poison = []
    for col in R.poison_columns(c):
        for bad in (np.inf, np.nan):
            xp = px.copy()
            xp[col] = bad
            poison.append((col, bad, xp, Ao.spmv(xp), Ao.spmv_add(xp, py0), E.rows_without(A, col)))
    ref = dict(Ao=Ao, oracle=u, exact=e, poison=poison, py0=py0, empty=np.diff(A.indptr) == 0)
    for d in (u, e):
        for v in d.values():
            v.setflags(write=False)
    _REFS[name] = ref
    return ref


def _mults(ctx, A, x, y0):
    nr = y0.size
    dx, out = _up(ctx, x), ctx.empty(nr)
    got = {"mult": to_host(ctx, A.mult(dx, out))}
    got["mult_add"] = to_host(ctx, A.mult_add(dx, _up(ctx, y0)))
    return got


def _assert_path(ra, A, c, p, fmt):
    """The operator took the path the case names (p: the claims or the restated plan)."""
    nr, nc = c.A.shape
    inf = A.info
    assert inf["format"] == {"auto": ra.AMG_FORMAT_AUTO, "csr": ra.AMG_FORMAT_CSR, "blocks": ra.AMG_FORMAT_BLOCKS}[fmt]
    assert (inf["n_global_rows"], inf["n_global_cols"], inf["n_local_cols"], inf["nnz_local"]) == (nr, nc, nc, c.A.nnz)
    assert inf["n_halo"] == 0 and inf["template_rows"] == 0 and inf["deferred"] == 0
    assert inf["n_blocks"] == p["n_blocks"], (inf["n_blocks"], p["n_blocks"])
    assert inf["n_vi_blocks"] == p["n_vi"], (inf["n_vi_blocks"], p["n_vi"])
    assert inf["tile_line_bytes"] == (0 if fmt == "csr" else p["tile_line_bytes"])
    assert bool(inf["kernel_variant"] & KV_GATHER) == (not p["tiled"])
    assert bool(inf["kernel_variant"] & KV_C16) == p["c16"], hex(inf["kernel_variant"])
    assert inf["residual_bytes"] == 0 and inf["jacobi_bytes"] == 0
    if fmt == "csr":
        assert inf["csr_bytes"] == 12 * c.A.nnz + 4 * (nr + 1) + 8 * (nr + nc) == inf["spmv_bytes"]


def _expected(c, env_name, env):
    p = R.plan(c.A, env)
    want = dict(n_blocks=len(p["blocks"]), n_vi=p["n_vi"], tiled=p["tiled"], c16=p["c16"],
                tile_line_bytes=p["tile_line_bytes"])
    if env_name == "own":   # the hand-derived claims themselves
        claims = dict(n_blocks=c.n_blocks, n_vi=c.n_vi_blocks, tiled=c.tiled, c16=c.c16,
                      tile_line_bytes=c.tile_line_bytes)
        assert claims == want
    return want


# ---- the zoo ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,env_name", ZOO_RUNS, ids=[f"{n}-{e}" for n, e in ZOO_RUNS])
def test_rect_zoo(ctx, oracle, monkeypatch, name, env_name):
    """Path, oracle, exact integers, poisoned columns and export, in every storage format."""
    import raptor_amd as ra

    c = R.zoo()[name]
    env = R.run_envs(c)[env_name]
    ref = _refs(oracle, name)
    want = _expected(c, env_name, env)
    _setenv(monkeypatch, env)
    A = _dev(ra, ctx, c.A)
    nr = c.A.shape[0]
    for fmt in FORMATS:
        A.set_format(fmt)
        _assert_path(ra, A, c, want, fmt)                                        # 1. the path
        for kind in ("oracle", "exact"):                                         # 2. oracle  3. exact integers
            r = ref[kind]
            got = _mults(ctx, A, r["x"], r["y0"])
            for mode in ("mult", "mult_add"):
                assert _same(got[mode], r[mode]), (fmt, kind, mode, _diff(got[mode], r[mode])[:8])
            # an empty row: mult writes +0.0, mult_add leaves y's bits
            assert np.all(bits(got["mult"])[ref["empty"]] == 0), (fmt, kind)
            assert _same(got["mult_add"][ref["empty"]], r["y0"][ref["empty"]]), (fmt, kind)
        out = ctx.empty(nr)
        for col, bad, xp, w0, w1, keep in ref["poison"]:                         # 4. poisoned columns
            dx = _up(ctx, xp)
            g0 = to_host(ctx, A.mult(dx, out))
            g1 = to_host(ctx, A.mult_add(dx, _up(ctx, ref["py0"])))
            for k, (g, w) in enumerate(((g0, w0), (g1, w1))):
                d = np.flatnonzero(bits(g)[keep] != bits(w)[keep])
                assert d.size == 0, (fmt, col, bad, k, np.flatnonzero(keep)[d][:8])
    rp, col, val = A.export()                                                    # 6. export
    assert np.array_equal(rp, c.A.indptr) and np.array_equal(col, c.A.indices) and _same(val, c.A.data)


@pytest.mark.parametrize("name", NAMES)
def test_rect_device_formats_equal_host_builders(ctx, monkeypatch, name):
    """5. formats.hip's packed indices, codes' operands and row ends equal the host builders'
    bytes on rectangular input."""
    import raptor_amd as ra

    c = R.zoo()[name]
    _setenv(monkeypatch, c.env)
    digest = {}
    for dev in ("1", "0"):
        monkeypatch.setenv("AMG_DEVICE_FORMATS", dev)
        A = _dev(ra, ctx, c.A)
        assert A.info["n_blocks"] == c.n_blocks and A.info["n_vi_blocks"] == c.n_vi_blocks
        digest[dev] = A.format_digest()
    assert digest["1"] == digest["0"]


@pytest.mark.parametrize("name", ["slots_512_to_2048", "bands_four", "rpb4_rows"])
def test_rect_checks_notice_one_changed_entry(ctx, oracle, monkeypatch, name):
    """7. With 1 added to one stored value of the uploaded operator, mult and mult_add differ from
    the exact references in that row and in no other."""
    import raptor_amd as ra

    c = R.zoo()[name]
    e = _refs(oracle, name)["exact"]
    _setenv(monkeypatch, c.env)
    Am, r = R.mutate(c.A, "value")
    A = _dev(ra, ctx, Am)
    assert A.info["n_blocks"] == c.n_blocks
    got = _mults(ctx, A, e["x"], e["y0"])
    for mode in ("mult", "mult_add"):
        assert _diff(got[mode], e[mode]).tolist() == [r], mode


# ---- what a rectangular handle refuses ---------------------------------------------------------------
def _canary(n):
    return np.full(n, np.float64(-12345.5))


@pytest.mark.parametrize("name", ["narrow_9", "slots_512_to_2048"])
def test_rect_square_only_calls_rejected(ctx, oracle, monkeypatch, name):
    """8. Every call that needs a diagonal or builds a solver returns AMG_ERR_INVALID, names the
    reason, writes nothing; a mult afterwards still gives the right bits."""
    import raptor_amd as ra

    c = R.zoo()[name]
    u = _refs(oracle, name)["oracle"]
    _setenv(monkeypatch, c.env)
    A = _dev(ra, ctx, c.A)
    nr, nc = c.A.shape
    dx, db = _up(ctx, u["x"]), _up(ctx, u["y0"])
    out, xio = _up(ctx, _canary(nr)), _up(ctx, u["x"])
    calls = {
        "residual": lambda: A.residual(dx, db, out),
        "jacobi": lambda: A.jacobi(dx, db, out, 0.5),
        "chebyshev_step": lambda: A.chebyshev_step(dx, None, db, out, 0.25, 0.5),
        "hybrid_gs": lambda: A.hybrid_gs(dx, db, out, 64),
        "hybrid_gs_backward": lambda: A.hybrid_gs(dx, db, out, 64, backward=True),
        "residual_norm": lambda: A.residual_norm(dx, db),
        "colour": lambda: A.colour(),
        "mc_gs": lambda: A.mc_gs(xio, db),
        "reorder": lambda: A.reorder(),
        "solver_setup": lambda: ra.ParRugeStubenSolver(coarsen="pmis").setup(A),
    }
    for call, fn in calls.items():
        with pytest.raises(ra.AmgError) as ei:
            fn()
        assert ei.value.code == AMG_ERR_INVALID, call
        assert "square" in str(ei.value) and call in str(ei.value), (call, str(ei.value))
    assert _same(to_host(ctx, out), _canary(nr)) and _same(to_host(ctx, xio), u["x"])
    assert _same(to_host(ctx, A.mult(dx, out)), u["mult"])
    assert A.info["n_blocks"] == c.n_blocks


def test_rect_bad_input_rejected(ctx, oracle):
    """9. The constructor validates like the square one, and the column range like the row range;
    unsorted rows give the sorted operator's bits."""
    import raptor_amd as ra

    A = R.zoo()["narrow_9"].A
    nr, nc = A.shape
    rp, col, val = A.indptr.astype(np.int64), A.indices.astype(np.int64), A.data.copy()

    def make(shape=(nr, nc), first_row=0, first_col=0, ncl=nc, rp=rp, col=col, val=val):
        return ra.ParCSRMatrix.from_csr_rect(ctx, shape, first_row, first_col, ncl, rp, col, val)

    k = int(rp[5])   # row 5 stores columns 5 and 8
    assert rp[6] - k == 2
    bad = {}
    c1 = col.copy()
    c1[k + 1] = nc
    bad["column id out of range"] = dict(col=c1)
    c2 = col.copy()
    c2[k] = c2[k + 1]
    bad["duplicate column"] = dict(col=c2)
    c3 = col.copy()
    c3[k] = -1
    bad["column id out of range "] = dict(col=c3)
    bad["column counts do not sum"] = dict(ncl=nc - 1)
    bad["first_col inconsistent"] = dict(first_col=1, ncl=nc - 1)
    bad["bad column range"] = dict(first_col=1)
    bad["row counts do not sum"] = dict(shape=(nr + 1, nc))
    r1 = rp.copy()
    r1[0] = 1
    bad["row_ptr[0]"] = dict(rp=r1)
    for msg, kw in bad.items():
        with pytest.raises(ra.AmgError) as ei:
            make(**kw)
        assert ei.value.code == AMG_ERR_INVALID and msg.strip() in str(ei.value), (msg, str(ei.value))
    # unsorted: every row of two entries reversed
    cu, vu = col.copy(), val.copy()
    two = np.flatnonzero(np.diff(rp) == 2)
    cu[rp[two]], cu[rp[two] + 1] = col[rp[two] + 1], col[rp[two]]
    vu[rp[two]], vu[rp[two] + 1] = val[rp[two] + 1], val[rp[two]]
    B = make(col=cu, val=vu)
    x = oracle.vec_uniform(nc, 3)
    want = _orc(oracle, A).spmv(x)
    assert _same(to_host(ctx, B.mult(_up(ctx, x), ctx.empty(nr))), want)
    e = B.export()
    assert np.array_equal(e[1], col) and _same(e[2], val)


# ---- guard bands ---------------------------------------------------------------------------------------
GUARD = ([("slots_512_to_2048", "own"), ("rpb4_rows", "own")] +
         [(m, "own") for m in R.zoo_names("empty") + R.zoo_names("long")] +
         [(m, e) for m in R.zoo_names("narrow") for e in ("own", "gather")])


@pytest.mark.skipif(native_mode(), reason="arena views are torch tensors")
@pytest.mark.parametrize("name,env_name", GUARD, ids=[f"{n}-{e}" for n, e in GUARD])
def test_rect_guard_bands(ctx, oracle, monkeypatch, name, env_name):
    """The vector-contract arena (tests/vector_contract_cases.py) around x of n_cols and y of
    n_rows at every operand parity: the unconditional re-reads of a block's last entry, a lane's
    absent rows and the 16-byte x loads at n - 2 stay inside the vectors."""
    import raptor_amd as ra
    from tests import test_gpu_vector_contract as VC

    c = R.zoo()[name]
    env = R.run_envs(c)[env_name]
    want = _expected(c, env_name, env)
    _setenv(monkeypatch, env)
    A = _dev(ra, ctx, c.A)
    _assert_path(ra, A, c, want, "auto")
    ref = VC._refs(oracle, ("rect", name), c.A, False)
    VC._run_all_placements(ctx, A, ref, VC._modes(ref))


# ---- several ranks ---------------------------------------------------------------------------------------
RANK_ENVS = {"own": {}, "gather": {"AMG_RECT_TILE": "0"}, "tile": {"AMG_RECT_TILE": "1"}}
RANK_POISON = {"band_across_halo": 30_000, "tiled_halo_tail": 2049, "missing_owners": 999}


@pytest.mark.parametrize("env_name", list(RANK_ENVS))
@pytest.mark.parametrize("name", list(R.rank_cases()))
def test_rect_ranks(oracle, monkeypatch, name, env_name):
    """Independent row and column partitions on 2 and 3 loopback ranks, slice by slice against
    the serial oracle: mult with one x, then with another on the same handle (a stale halo
    buffer or a missing wait shows as the first x's values), mult_add, and a poisoned halo
    column."""
    import raptor_amd as ra

    O = oracle
    c = R.rank_cases()[name]
    env = RANK_ENVS[env_name]
    _setenv(monkeypatch, env)
    nr, nc = c.A.shape
    Ao = _orc(O, c.A)
    x1, x2, y0 = O.vec_uniform(nc, 3), O.vec_uniform(nc, 4), O.vec_uniform(nr, 5)
    pc = RANK_POISON[name]
    xp = x1.copy()
    xp[pc] = np.inf
    want = dict(m1=Ao.spmv(x1), m2=Ao.spmv(x2), add=Ao.spmv_add(x2, y0), poison=Ao.spmv(xp))
    assert not _same(want["m1"], want["m2"])
    keep = E.rows_without(c.A, pc)
    nranks = len(c.row_starts) - 1

    def rank(r, n, world):
        ctx = loopback_ctx(r, n, world)
        G, L, ncl, halo, cls = R.local_view(c, r)
        f, fc = c.row_starts[r], c.col_starts[r]
        A = ra.ParCSRMatrix.from_csr_rect(ctx, (nr, nc), f, fc, ncl, G.indptr, G.indices, G.data)
        m = G.shape[0]
        out = ctx.empty(m)
        got = {}
        for key, x in (("m1", x1), ("m2", x2), ("poison", xp)):
            got[key] = to_host(ctx, A.mult(_up(ctx, x[fc:fc + ncl]), out))
        got["add"] = to_host(ctx, A.mult_add(_up(ctx, x2[fc:fc + ncl]), _up(ctx, y0[f:f + m])))
        return f, m, got, A.info, R.plan(L, env, ncl, cls), halo.size, ncl

    res = run_ranks(nranks, rank)
    assert sum(m for _, m, *_ in res) == nr
    for r, (f, m, got, inf, p, nh, ncl) in enumerate(res):
        assert (inf["n_local_rows"], inf["n_local_cols"], inf["n_halo"]) == (m, ncl, nh), r
        assert (inf["first_row"], inf["first_col"]) == (f, c.col_starts[r])
        assert inf["n_blocks"] == len(p["blocks"]) and inf["n_vi_blocks"] == p["n_vi"], r
        assert inf["tile_line_bytes"] == p["tile_line_bytes"], r
        assert bool(inf["kernel_variant"] & KV_GATHER) == (not p["tiled"]), r
        assert bool(inf["kernel_variant"] & KV_C16) == p["c16"], r
        for key in ("m1", "m2", "add"):
            assert _same(got[key], want[key][f:f + m]), (r, key, _diff(got[key], want[key][f:f + m])[:8])
        k = keep[f:f + m]
        assert _same(got["poison"][k], want["poison"][f:f + m][k]), r
        assert not np.isfinite(got["poison"][~k]).any(), r
    # the poisoned column is a halo column of a rank that reads it
    owner = int(np.searchsorted(c.col_starts, pc, side="right") - 1)
    readers = [r for r, (f, m, *_) in enumerate(res) if not keep[f:f + m].all()]
    assert any(r != owner for r in readers)
