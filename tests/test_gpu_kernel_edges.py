"""The level kernels on operators that sit exactly on the storage formats' limits
(tests/edge_cases.py), checked three ways that do not go through the CPU oracle -- exact
int64 arithmetic, exact fixed points, poisoned columns -- and against the oracle bit for bit.

Every case asserts through ParCSRMatrix.info that it reached the limit it names (the block
count its docstring derives by hand, value-indexed blocks, templates, x-tile line width, split
sweep and chain width), so none passes vacuously.  Every comparison is on bit patterns
(edge_cases.bits); the fused norm alone is compared within 1e-12 relative."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import edge_cases as E
from tests.edge_cases import bits
from tests.util import to_dev, to_host

pytestmark = pytest.mark.gpu

NAMES = E.zoo_names()
DIAG_NAMES = [m for m in NAMES if E.zoo()[m].full_diag]
GS_BLOCKS = (64, 48, 17, 1)
# storage format, AMG_KERNEL_VARIANT (74 / 66: the persistent x-tile kernel with / without VI)
CONFIGS = [("auto", None), ("blocks", None), ("csr", None), ("blocks", "74"), ("blocks", "66")]
GS_PATHS = {"default": {},
            "generic": {"AMG_TPL_MASTER": "0"},
            "ell": {"AMG_GS_TEMPLATES": "0", "AMG_GS_SPLIT": "0"},
            "split": {"AMG_GS_SPLIT_NPR": "0"}}


def _same(a, b):
    return np.array_equal(bits(a), bits(b))


def _orc(O, A):
    return O.Csr.from_arrays(A.shape[0], A.shape[1], A.indptr, A.indices, A.data)


def _dev(ra, ctx, A):
    return ra.ParCSRMatrix.from_csr(ctx, A.shape[0], 0, A.indptr, A.indices, A.data)


def _up(ctx, a):
    """A device copy (of a private host copy: the shared references are read-only)."""
    return to_dev(ctx, np.array(a, np.float64))


def _setenv(monkeypatch, *envs):
    for env in envs:
        for k, v in env.items():
            monkeypatch.setenv(k, v)


_REFS = {}


def _refs(O, name):
    """Per case, computed once and shared (read-only): the oracle's results on vec_uniform
    data, the exact int64 results on int_vectors data, and the fixed-point right-hand side."""
    if name in _REFS:
        return _REFS[name]
    c = E.zoo()[name]
    A, Ao = c.A, _orc(O, c.A)
    n = A.shape[0]
    u = dict(x=O.vec_uniform(n, 3), b=O.vec_uniform(n, 4), y0=O.vec_uniform(n, 5))
    u.update(mult=Ao.spmv(u["x"]), mult_add=Ao.spmv_add(u["x"], u["y0"]),
             residual=Ao.residual(u["x"], u["b"]))
    u["norm"] = O.norm2(u["residual"])
    ix, iy0, ib = E.int_vectors(n, 7)
    e = dict(x=ix, b=ib, y0=iy0, mult=E.exact_spmv(A, ix), mult_add=E.exact_spmv_add(A, ix, iy0),
             residual=E.exact_residual(A, ix, ib), norm=E.exact_residual_norm(A, ix, ib))
    if c.full_diag:
        u["jacobi"] = Ao.jacobi(u["x"], u["b"], 2.0 / 3.0)
        u["gs"] = {(B, bw): (Ao.hybrid_gs_backward if bw else Ao.hybrid_gs)(u["x"], u["b"], B)
                   for B in GS_BLOCKS for bw in (False, True)}
        e["jacobi"] = E.exact_jacobi(A, ix, ib)
        e["b_fixed"] = E.b_for_fixed_point(A, ix)
    _REFS[name] = dict(Ao=Ao, oracle=u, exact=e)
    for d in (u, e):
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
    return _REFS[name]


def _vector_modes(ctx, A, x, b, y0, jacobi_omega=None):
    n = x.size
    dx, db, out = _up(ctx, x), _up(ctx, b), ctx.empty(n)
    got = {"mult": to_host(ctx, A.mult(dx, out))}
    dy = _up(ctx, y0)
    got["mult_add"] = to_host(ctx, A.mult_add(dx, dy))
    got["residual"] = to_host(ctx, A.residual(dx, db, out))
    if jacobi_omega is not None:
        got["jacobi"] = to_host(ctx, A.jacobi(dx, db, out, jacobi_omega))
    got["norm"] = A.residual_norm(dx, db)
    return got


def _check_modes(got, want, label):
    for k, g in got.items():
        if k == "norm":
            assert abs(g - want[k]) <= 1e-12 * want[k], (label, k, g, want[k])
        else:
            assert _same(g, want[k]), (label, k, np.flatnonzero(bits(g) != bits(want[k]))[:8])


def _check_poison(ctx, O, A, Asp, Ao, cols, seed=11):
    """x[c] = inf, then nan: every row without an entry in column c has the oracle's bits in
    mult, mult_add and residual.  (The rows that do reference c have a non-finite residual
    whatever b is, so no b excludes them from the fused norm: vector modes only.)"""
    nr, nc = Asp.shape
    x, b, y0 = O.vec_uniform(nc, seed), O.vec_uniform(nr, seed + 1), O.vec_uniform(nr, seed + 2)
    db, out = _up(ctx, b), ctx.empty(nr)
    for c in cols:
        keep = E.rows_without(Asp, c)
        for bad in (np.inf, np.nan):
            xp = x.copy()
            xp[c] = bad
            dx = _up(ctx, xp)
            got = [to_host(ctx, A.mult(dx, out))]
            got.append(to_host(ctx, A.mult_add(dx, _up(ctx, y0))))
            want = [Ao.spmv(xp), Ao.spmv_add(xp, y0)]
            if nr == nc:
                got.append(to_host(ctx, A.residual(dx, db, out)))
                want.append(Ao.residual(xp, b))
            for k, (g, w) in enumerate(zip(got, want)):
                bad_rows = np.flatnonzero(bits(g)[keep] != bits(w)[keep])
                assert bad_rows.size == 0, (c, bad, k, np.flatnonzero(keep)[bad_rows][:8])


# ---- the zoo: every format and the persistent variants ------------------------------------
@pytest.mark.parametrize("fmt,var", CONFIGS, ids=[f if v is None else f"{f}-v{v}" for f, v in CONFIGS])
@pytest.mark.parametrize("name", NAMES)
def test_zoo_kernels(ctx, oracle, monkeypatch, name, fmt, var):
    """Path assertions, then all modes against the oracle, against exact integers, and with
    poisoned columns."""
    import raptor_amd as ra

    O = oracle
    c = E.zoo()[name]
    ref = _refs(O, name)
    _setenv(monkeypatch, c.env, {} if var is None else {"AMG_KERNEL_VARIANT": var})
    A = _dev(ra, ctx, c.A).set_format(fmt)
    n = c.A.shape[0]
    # 1. the path
    inf = A.info
    assert inf["format"] == {"auto": ra.AMG_FORMAT_AUTO, "csr": ra.AMG_FORMAT_CSR,
                             "blocks": ra.AMG_FORMAT_BLOCKS}[fmt]
    assert inf["n_blocks"] == c.n_blocks, (inf["n_blocks"], c.n_blocks)
    if c.n_vi_blocks is not None:
        assert inf["n_vi_blocks"] == c.n_vi_blocks
    if c.n_templates is not None:
        assert inf["n_templates"] == c.n_templates
        assert inf["template_rows"] == (c.template_rows if fmt == "auto" else 0)
    elif fmt != "auto":
        assert inf["template_rows"] == 0
    if fmt == "csr":  # the plain arrays and nothing else
        assert inf["csr_bytes"] == 12 * c.A.nnz + 4 * (n + 1) + 16 * n == inf["spmv_bytes"]
    if c.tile_line_bytes is not None:
        assert inf["tile_line_bytes"] == (0 if fmt == "csr" else c.tile_line_bytes)
    # 2. against the oracle (uniform random data)  3. against exact integers
    om = 2.0 / 3.0 if c.full_diag else None
    u, e = ref["oracle"], ref["exact"]
    _check_modes(_vector_modes(ctx, A, u["x"], u["b"], u["y0"], om), u, "oracle")
    _check_modes(_vector_modes(ctx, A, e["x"], e["b"], e["y0"], 0.5 if c.full_diag else None), e, "exact")
    if c.full_diag:
        dx, db, out = _up(ctx, u["x"]), _up(ctx, u["b"]), ctx.empty(n)
        for B in GS_BLOCKS:
            for bw in (False, True):
                A.hybrid_gs(dx, db, out, B, backward=bw)
                assert _same(to_host(ctx, out), u["gs"][(B, bw)]), ("gs", B, bw)
            if B != 64:
                continue
            g = A._info()
            if c.gs_width is not None:
                assert g["gs_split"] == 1
                assert g["gs_chain_maxw"] == c.gs_width | c.gs_width << 16, hex(g["gs_chain_maxw"])
            if c.ell_wide:
                # one sliced-ELL kernel; its cells (>= kGsWide per slab: the wide variant)
                # show in the byte count: 12 or 5 B per cell x 64 lanes + slabs + rows
                slabs, cells = E.ell_slabs(c.A, 64)
                assert g["gs_split"] == 0 and cells >= E.GS_WIDE * slabs
                assert g["gs_bytes"] - 16 * slabs - 32 * n in (12 * 64 * cells, 5 * 64 * cells)
    if c.n_values is not None:  # the GS dictionary's limit has no info field: count what is stored
        assert len(np.unique(bits(A.export()[2]))) == c.n_values
    # 5. poisoned columns
    _check_poison(ctx, O, A, c.A, ref["Ao"], E.poison_columns(c.A))


@pytest.mark.parametrize("name", ["cap_nnz_plus1", "vi_255_256_257", "gs_chain_63"])
def test_checks_notice_one_changed_entry(ctx, oracle, monkeypatch, name):
    """The comparisons above are not vacuous on the device side either: with 1 added to one
    stored off-diagonal value of the uploaded operator, the exact-integer comparison fails and
    every fixed point is lost."""
    import raptor_amd as ra

    c = E.zoo()[name]
    e = _refs(oracle, name)["exact"]
    _setenv(monkeypatch, c.env)
    Am = c.A.copy()
    r = c.A.shape[0] // 2
    k = Am.indptr[r] + (1 if Am.indices[Am.indptr[r]] == r else 0)
    assert Am.indices[k] != r
    Am.data[k] += 1.0
    A = _dev(ra, ctx, Am)
    got = _vector_modes(ctx, A, e["x"], e["b"], e["y0"], 0.5)
    for mode in ("mult", "mult_add", "residual", "jacobi"):
        diff = np.flatnonzero(bits(got[mode]) != bits(e[mode]))
        assert diff.tolist() == [r], (mode, diff[:8])
    with pytest.raises(AssertionError):
        _check_modes(got, e, "exact")
    n = c.A.shape[0]
    dx, db, out = _up(ctx, e["x"]), _up(ctx, e["b_fixed"]), ctx.empty(n)
    assert not _same(to_host(ctx, A.jacobi(dx, db, out, 2.0 / 3.0)), e["x"])
    assert A.residual_norm(dx, db) > 0.0
    for B in GS_BLOCKS:
        for bw in (False, True):
            A.hybrid_gs(dx, db, out, B, backward=bw)
            assert not _same(to_host(ctx, out), e["x"]), (B, bw)


@pytest.mark.parametrize("name", E.zoo_names("cap_nnz") + E.zoo_names("vi_table") + E.zoo_names("gs_chain"))
def test_zoo_matmat(ctx, oracle, monkeypatch, name):
    """A.matmat(A): the oracle's pattern, the int64 product's values."""
    import raptor_amd as ra

    c = E.zoo()[name]
    _setenv(monkeypatch, c.env)
    A = _dev(ra, ctx, c.A)
    C = A.matmat(A).to_scipy_local()
    Ao = _refs(oracle, name)["Ao"]
    Co = (Ao @ Ao).to_scipy()
    assert np.array_equal(C.indptr, Co.indptr) and np.array_equal(C.indices, Co.indices)
    assert _same(C.data, E.exact_matmat(c.A, c.A, Co).data.astype(np.float64))


@pytest.mark.parametrize("path", list(GS_PATHS))
@pytest.mark.parametrize("name", DIAG_NAMES)
def test_zoo_fixed_points(ctx, oracle, monkeypatch, name, path):
    """b = A x formed in int64: jacobi and every hybrid GS path return x bit for bit."""
    import raptor_amd as ra

    c = E.zoo()[name]
    ref = _refs(oracle, name)["exact"]
    # the case's own GS knobs give way to the path's
    _setenv(monkeypatch, {k: v for k, v in c.env.items() if not k.startswith("AMG_GS_")}, GS_PATHS[path])
    A = _dev(ra, ctx, c.A)
    n = c.A.shape[0]
    x = ref["x"]
    dx, db, out = _up(ctx, x), _up(ctx, ref["b_fixed"]), ctx.empty(n)
    assert _same(to_host(ctx, A.jacobi(dx, db, out, 2.0 / 3.0)), x), "jacobi"
    assert A.residual_norm(dx, db) == 0.0
    for B in GS_BLOCKS:
        for bw in (False, True):
            A.hybrid_gs(dx, db, out, B, backward=bw)
            assert _same(to_host(ctx, out), x), (B, bw)
        if path == "split" and c.gs_width is not None:  # no row templates: nothing keeps the split off
            assert A._info()["gs_split"] == 1
        if path == "ell":
            assert A._info()["gs_split"] == 0


@pytest.mark.parametrize("name", NAMES)
def test_zoo_device_formats_equal_host_builders(ctx, monkeypatch, name):
    """formats.hip's device builders give the host builders' bytes on every zoo operator."""
    import raptor_amd as ra

    c = E.zoo()[name]
    _setenv(monkeypatch, c.env)
    digest = {}
    for dev in ("1", "0"):
        monkeypatch.setenv("AMG_DEVICE_FORMATS", dev)
        A = _dev(ra, ctx, c.A)
        assert A.info["n_blocks"] == c.n_blocks
        digest[dev] = A.format_digest()
    assert digest["1"] == digest["0"]


# ---- poisoned columns on the row-template kernels ------------------------------------------
STENCILS = [("7pt", (20, 20, 20)), ("27pt", (13, 13, 13)), ("27pt", (260, 8, 8))]
TPL_PATHS = {"master": {}, "generic": {"AMG_TPL_MASTER": "0"},
             "march": {"AMG_KERNEL_VARIANT": str(170 | 512), "AMG_TPL_MARCH_CHUNKS": "1"}}


@pytest.mark.parametrize("path", list(TPL_PATHS))
@pytest.mark.parametrize("kind,dims", STENCILS, ids=[f"{k}-{'x'.join(map(str, d))}" for k, d in STENCILS])
def test_stencil_poisoned_columns(ctx, oracle, monkeypatch, kind, dims, path):
    """The template kernels -- masked entries of the uniform-stencil path, per-template tables,
    the forced march -- keep a poisoned x[c] out of every row that does not reference c."""
    import raptor_amd as ra

    O = oracle
    Ao = {"7pt": O.gen_7pt, "27pt": O.gen_27pt}[kind](*dims)
    Asp = Ao.to_scipy()
    _setenv(monkeypatch, TPL_PATHS[path])
    A = _dev(ra, ctx, Asp)
    n = Asp.shape[0]
    inf = A.info
    assert inf["template_rows"] == n
    assert inf["tpl_master"] == (0 if path == "generic" else {"7pt": 7, "27pt": 27}[kind])
    if dims == (260, 8, 8):
        assert inf["tpl_lanes"] == 16
        if path == "march":
            assert inf["tpl_march_shift"] > 0
    groups = [(q, min(n, q + 512)) for q in range(0, n, 512)]  # the template kernel's row groups
    _check_poison(ctx, O, A, Asp, Ao, E.poison_columns(Asp, groups))


# ---- rectangular operators, directly ---------------------------------------------------------
RECT_ENV = {"default": {}, "gather_int32": {"AMG_GATHER_C16": "0"}, "rect_tile": {"AMG_RECT_TILE": "1"}}


@pytest.mark.parametrize("env", list(RECT_ENV))
@pytest.mark.parametrize("hier", ["pmis_7pt", "sa_graph"])
def test_rectangular_operators(ctx, oracle, monkeypatch, hier, env):
    """Every level's P and R of a PMIS and a smoothed-aggregation hierarchy: mult and mult_add
    against the oracle on the exported arrays, and a poisoned column each."""
    import raptor_amd as ra

    O = oracle
    _setenv(monkeypatch, RECT_ENV[env])
    if hier == "pmis_7pt":
        ml = ra.ParRugeStubenSolver(coarsen="pmis").setup(ra.par_stencil_grid(ctx, "7pt", (22, 21, 20)))
    else:
        ml = ra.ParSmoothedAggregationSolver().setup(ra.par_graph_laplacian(ctx, 120, 110))
    assert ml.num_levels >= 2
    for l in range(ml.num_levels - 1):
        for w in "PR":
            M = ml.level_matrix(l, w)
            rp, col, val = M.export()
            nr, nc = rp.size - 1, M.info["n_global_cols"]
            Mo = O.Csr.from_arrays(nr, nc, rp, col, val)
            Msp = sp.csr_matrix((val, col, rp), shape=(nr, nc))
            x, y0 = O.vec_uniform(nc, 21 + l), O.vec_uniform(nr, 31 + l)
            dx, out = _up(ctx, x), ctx.empty(nr)
            assert _same(to_host(ctx, M.mult(dx, out)), Mo.spmv(x)), (l, w, "mult")
            dy = _up(ctx, y0)
            assert _same(to_host(ctx, M.mult_add(dx, dy)), Mo.spmv_add(x, y0)), (l, w, "mult_add")
            inf = M.info
            assert inf["deferred"] == 0
            if env == "rect_tile":
                assert inf["tile_line_bytes"] in (32, 64), (l, w)
            if env == "gather_int32":
                assert not inf["kernel_variant"] & 256
            _check_poison(ctx, O, M, Msp, Mo, [nc // 2])


# ---- the whole cycle at an exact fixed point ---------------------------------------------------
def _int_7pt(nx, ny, nz):
    """The 7-point Laplacian with entries 6 and -1, assembled here (exact small integers)."""
    def lap(m):
        return sp.diags([-np.ones(m - 1), 2 * np.ones(m), -np.ones(m - 1)], [-1, 0, 1])
    ex, ey, ez = sp.identity(nx), sp.identity(ny), sp.identity(nz)
    A = sp.kron(ez, sp.kron(ey, lap(nx))) + sp.kron(ez, sp.kron(lap(ny), ex)) + sp.kron(lap(nz), sp.kron(ey, ex))
    A = A.tocsr()
    A.sort_indices()
    return A


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("kind", ["pmis_jacobi", "sa_gs"])
def test_cycle_fixed_point(ctx, monkeypatch, kind, graph):
    """ml.cycle(x*, b) with b = A x* formed in int64 leaves x* bit-unchanged, cycle after
    cycle: every fine residual is exactly zero, so every coarse right-hand side and correction
    must be.  A coarse buffer that is not zeroed, or a stale graph node, breaks this."""
    import raptor_amd as ra

    Asp = _int_7pt(20, 20, 20)
    n = Asp.shape[0]
    A = _dev(ra, ctx, Asp)
    if kind == "pmis_jacobi":
        ml = ra.ParRugeStubenSolver(coarsen="pmis", use_graph=graph).setup(A)
    else:
        ml = ra.ParSmoothedAggregationSolver(use_graph=graph).setup(A)
    assert ml.num_levels >= 2 and ml.graph_enabled == graph
    xs, _, b_other = E.int_vectors(n, 13)
    # a first cycle on other data leaves every coarse buffer (and the captured graph) used
    ml.cycle(_up(ctx, np.zeros(n)), _up(ctx, b_other))
    dx, db = _up(ctx, xs), _up(ctx, E.b_for_fixed_point(Asp, xs))
    for it in range(3):
        ml.cycle(dx, db)
        assert _same(to_host(ctx, dx), xs), it
