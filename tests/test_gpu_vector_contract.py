"""The C-ABI vector contract (include/raptor_amd.h, "Vectors") on the GPU: what a caller may pass
at the boundary -- sub-ranges of a larger allocation at 8-byte-aligned starts, the allowed exact
aliases -- and what is refused before anything is launched: overlaps and null vectors.

Every operand of every call lives in one arena (tests/vector_contract_cases.py) between guard
bands of 2048 doubles: NaN around inputs, index-carrying canaries around outputs.  Per run:
the output has the reference's bits (edge_cases.bits; the oracle's kernels, cheby_cases' step),
no guard word changed, no input changed.  A read outside x[0, n_cols) that reaches a product
turns a row non-finite, a write outside y[0, n_rows) changes a canary.  Operand starts take the
parities (even, even), (odd, odd), (odd x, even others) and 7 mod 8.

Why an 8-byte-aligned base is valid at every access to a caller's vector in kernels.hip (read
before the odd starts were run).  The hardware's global, buffer and scalar-free vector memory
instructions need dword alignment only (the runtime runs the device in unaligned access mode),
so the question at each site is whether the *range* stays inside the vector, not the address:
  * load_pair (x-tile path of block_main): one 16-byte load at element min(q, n - 2), any q --
    odd element offsets on a 16-byte-aligned base are what every earlier test already ran; an
    8-byte-aligned base shifts the same loads by 8.  In range for n >= 2; n == 1 (wide_x == 0)
    takes the 8-byte loads clamped to n - 1.
  * xload / plain_x (gather path, block_long, the plain-CSR kernel) and every row operand
    (a.b[rr], a.x[rr], a.y[rr], a.xprev[rr], a.dinv is the library's): 8-byte accesses at a
    clamped row (lanes past the block re-read row r0 / r1 - 1 / n - 1 and discard it).  The
    plain-CSR arrays' two padding entries are column 0, value 0: a read of x[0].
  * tpl_xrs and the raw_buffer_load_b128 / _b64 sites (TplFetch::issue_window, tpl_rows' global
    path, the march kernel, tpl_gs_acc_kernel): a raw buffer descriptor with a byte base and
    num_records = 8 n; the hardware checks offset + size against num_records, not the address,
    so an 8-byte-aligned base moves nothing.  16-byte pair loads are issued only by blocks whose
    window lies inside [0, n) (`pairs`), at even element offsets relative to the base; the
    first and last blocks load single slots and out-of-range ones (negative offsets wrap to
    large unsigned ones) return 0.
  * hybrid_gs_kernel / gs_chain_kernel (sliced ELL, split chain walk): 8-byte loads of b[r],
    x[r], x[col] and one 8-byte store of y[r] per live lane.
  * tpl_gs_chain_kernel: 16-byte loads of x and stores of y at c0 + 2 (lane % 8) + 16 batch, taken
    only when every chunk of the wave is whole (c1 - c0 == B <= n): inside [0, n) at even
    element offsets; clipped chunks walk 8 bytes at a time.
  * pack_kernel (halo exchange): x[idx[i]], 8 bytes.
None needs 16 bytes, so no entry point rejects an 8-byte-aligned vector; amg_vector_copy /
_read keep their documented 16-byte check, tested below.

The tests need torch tensors for the views (arena[o:o + n]): they skip on torch-free contexts."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

from tests import cheby_cases as CH
from tests import cycle_option_cases as K
from tests import edge_cases as E
from tests import vector_contract_cases as V
from tests.edge_cases import bits
from tests.test_gpu_kernel_edges import CONFIGS, GS_PATHS, RECT_ENV, STENCILS, TPL_PATHS
from tests.test_gpu_multirank import run_ranks
from tests.util import loopback_ctx, native_mode, to_dev, to_host

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(native_mode(), reason="arena views are torch tensors")]

C1, C2 = 0.37109375, 0.8125
OMEGA = 2.0 / 3.0
GS_B = (64, 17)
# (x start, other operands' start) modulo 8: (even, even), (odd, odd), (odd, even), 7 mod 8
PLACEMENTS = {"even-even": (0, 2), "odd-odd": (1, 3), "odd-even": (5, 0), "seven": (7, 7)}
ZOO = ["cap_nnz_plus1", "cap_rows_257", "cap_rows_nnz0", "cap_lines_513", "cap_lines_long_row",
       "vi_255_256_257", "odd_offsets", "tpl_len_63_64_65", "tpl_entries_1025", "gs_ell_wide_257"]
ZOO_DIAG = [m for m in ZOO if E.zoo()[m].full_diag]
ALIAS_ZOO = ["cap_nnz_plus1", "vi_255_256_257", "tpl_len_63_64_65"]
CFG_IDS = [f if v is None else f"{f}-v{v}" for f, v in CONFIGS]
STENCIL_IDS = [f"{k}-{'x'.join(map(str, d))}" for k, d in STENCILS]


def _setenv(monkeypatch, *envs):
    for env in envs:
        for k, v in env.items():
            monkeypatch.setenv(k, v)


def _dev(ra, ctx, A):
    return ra.ParCSRMatrix.from_csr(ctx, A.shape[0], 0, A.indptr, A.indices, A.data)


def _diff(a, b):
    return np.flatnonzero(bits(a) != bits(b))


def _up(ctx, a):
    """A device copy (of a private host copy: the shared references are read-only)."""
    return to_dev(ctx, np.array(a, np.float64))


# ---- references: once per operator, shared, read-only ---------------------------------------------
_REFS = {}


def _refs(O, key, Asp, diag):
    """x, b, y0, xp on vec_uniform data and every mode's reference.  diag: the operator is
    square with a full non-zero diagonal (Jacobi, the Chebyshev step, hybrid GS)."""
    if key in _REFS:
        return _REFS[key]
    Asp = Asp.tocsr()
    nr, nc = Asp.shape
    Ao = O.Csr.from_arrays(nr, nc, Asp.indptr, Asp.indices, Asp.data)
    r = dict(Ao=Ao, nr=nr, nc=nc, diag=diag, square=nr == nc,
             x=O.vec_uniform(nc, 3), b=O.vec_uniform(nr, 4), y0=O.vec_uniform(nr, 5), xp=O.vec_uniform(nr, 6))
    r["mult"] = Ao.spmv(r["x"])
    r["mult_add"] = Ao.spmv_add(r["x"], r["y0"])
    if nr == nc:
        r["residual"] = Ao.residual(r["x"], r["b"])
        r["norm"] = O.norm2(r["residual"])
    if diag:
        r["jacobi"] = Ao.jacobi(r["x"], r["b"], OMEGA)
        r["dinv"] = 1.0 / Asp.diagonal()
        r["cheby"] = CH.cheby_step(Ao, r["dinv"], r["x"], r["xp"], r["b"], C1, C2)
        for B in GS_B:
            r[f"gs{B}"] = Ao.hybrid_gs(r["x"], r["b"], B)
            r[f"gsb{B}"] = Ao.hybrid_gs_backward(r["x"], r["b"], B)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _REFS[key] = r
    return r


def _modes(ref, vec=True, gs=True):
    m = []
    if vec:
        m += ["mult", "mult_add"]
        if ref["square"]:
            m += ["residual"]
        if ref["diag"]:
            m += ["jacobi", "cheby"]
    if gs and ref["diag"]:
        m += [f"{k}{B}" for B in GS_B for k in ("gs", "gsb")]
    return m


def _call(A, mode, x, b, xp, out):
    if mode == "mult":
        A.mult(x, out)
    elif mode == "mult_add":
        A.mult_add(x, out)
    elif mode == "residual":
        A.residual(x, b, out)
    elif mode == "jacobi":
        A.jacobi(x, b, out, OMEGA)
    elif mode == "cheby":
        A.chebyshev_step(x, xp, b, out, C1, C2)
    elif mode.startswith("gsb"):
        A.hybrid_gs(x, b, out, int(mode[3:]), backward=True)
    else:
        A.hybrid_gs(x, b, out, int(mode[2:]))


def _arena(ref, modes, place):
    xm, om = PLACEMENTS[place]
    ar = V.Arena()
    ar.input("x", ref["x"], xm)
    ar.input("b", ref["b"], om)
    step = 0 if om == 7 else 2  # starts of one parity; "seven": every operand at 7 mod 8
    ar.input("xp", ref["xp"], om + step)
    for k, mode in enumerate(modes):
        ar.output(mode, ref["nr"], om + step * (k % 3), init=ref["y0"] if mode == "mult_add" else None)
    return ar


def _assert_clean(ar, label):
    g = ar.check()
    assert g.size == 0, (label, "guard words changed", [ar.owner(i) for i in g[:8]])
    c = ar.inputs_changed()
    assert c.size == 0, (label, "inputs changed", [ar.owner(i) for i in c[:8]])


def _run_placed(ctx, A, ref, modes, place, norm=True):
    """Every mode once on one arena: reference bits, guards intact, inputs unchanged."""
    ar = _arena(ref, modes, place).upload(ctx)
    for mode in modes:
        _call(A, mode, ar["x"], ar["b"], ar["xp"], ar[mode])
    got_norm = A.residual_norm(ar["x"], ar["b"]) if norm and ref["square"] else None
    ar.download(ctx)
    for mode in modes:
        d = _diff(ar.get(mode), ref[mode])
        assert d.size == 0, (place, mode, d[:8])
    _assert_clean(ar, place)
    if got_norm is not None:  # the fused norm: 1e-12 relative, as test_zoo_kernels
        assert abs(got_norm - ref["norm"]) <= 1e-12 * ref["norm"], (place, got_norm, ref["norm"])


def _run_all_placements(ctx, A, ref, modes, norm=True):
    for place in PLACEMENTS:
        _run_placed(ctx, A, ref, modes, place, norm)


# ---- a. the zoo ---------------------------------------------------------------------------------
def _assert_zoo_path(ra, A, c, fmt):
    """test_zoo_kernels' path assertions: the case reached the limit it names."""
    n = c.A.shape[0]
    inf = A.info
    assert inf["format"] == {"auto": ra.AMG_FORMAT_AUTO, "csr": ra.AMG_FORMAT_CSR, "blocks": ra.AMG_FORMAT_BLOCKS}[fmt]
    assert inf["n_blocks"] == c.n_blocks, (inf["n_blocks"], c.n_blocks)
    if c.n_vi_blocks is not None:
        assert inf["n_vi_blocks"] == c.n_vi_blocks
    if c.n_templates is not None:
        assert inf["n_templates"] == c.n_templates
        assert inf["template_rows"] == (c.template_rows if fmt == "auto" else 0)
    elif fmt != "auto":
        assert inf["template_rows"] == 0
    if fmt == "csr":
        assert inf["csr_bytes"] == 12 * c.A.nnz + 4 * (n + 1) + 16 * n == inf["spmv_bytes"]
    if c.tile_line_bytes is not None:
        assert inf["tile_line_bytes"] == (0 if fmt == "csr" else c.tile_line_bytes)


@pytest.mark.parametrize("fmt,var", CONFIGS, ids=CFG_IDS)
@pytest.mark.parametrize("name", ZOO)
def test_zoo_guard_bands(ctx, oracle, monkeypatch, name, fmt, var):
    import raptor_amd as ra

    c = E.zoo()[name]
    _setenv(monkeypatch, c.env, {} if var is None else {"AMG_KERNEL_VARIANT": var})
    A = _dev(ra, ctx, c.A).set_format(fmt)
    _assert_zoo_path(ra, A, c, fmt)
    ref = _refs(oracle, name, c.A, c.full_diag)
    _run_all_placements(ctx, A, ref, _modes(ref))
    if c.full_diag:
        g = A._info()
        if c.gs_width is not None:
            assert g["gs_split"] == 1
        if c.ell_wide:
            assert g["gs_split"] == 0


@pytest.mark.parametrize("path", list(GS_PATHS))
@pytest.mark.parametrize("name", ZOO_DIAG)
def test_zoo_gs_paths_guard_bands(ctx, oracle, monkeypatch, name, path):
    import raptor_amd as ra

    c = E.zoo()[name]
    # the case's own GS knobs give way to the path's (test_zoo_fixed_points)
    _setenv(monkeypatch, {k: v for k, v in c.env.items() if not k.startswith("AMG_GS_")}, GS_PATHS[path])
    A = _dev(ra, ctx, c.A)
    assert A.info["n_blocks"] == c.n_blocks
    ref = _refs(oracle, name, c.A, True)
    _run_all_placements(ctx, A, ref, _modes(ref, vec=False), norm=False)
    if path == "split" and c.gs_width is not None:
        assert A._info()["gs_split"] == 1
    if path == "ell":
        assert A._info()["gs_split"] == 0


# ---- b. the template kernels ----------------------------------------------------------------------
def _stencil(O, kind, dims):
    return {"7pt": O.gen_7pt, "27pt": O.gen_27pt, "5pt": O.gen_5pt}[kind](*dims).to_scipy()


def _assert_tpl_path(A, n, kind, dims, path):
    inf = A.info
    assert inf["template_rows"] == n
    assert inf["tpl_master"] == (0 if path == "generic" else {"7pt": 7, "27pt": 27}[kind])
    if dims == (260, 8, 8):
        assert inf["tpl_lanes"] == 16
        if path == "march":
            assert inf["tpl_march_shift"] > 0


@pytest.mark.parametrize("path", list(TPL_PATHS))
@pytest.mark.parametrize("kind,dims", STENCILS, ids=STENCIL_IDS)
def test_stencil_guard_bands(ctx, oracle, monkeypatch, kind, dims, path):
    import raptor_amd as ra

    Asp = _stencil(oracle, kind, dims)
    _setenv(monkeypatch, TPL_PATHS[path])
    A = _dev(ra, ctx, Asp)
    _assert_tpl_path(A, Asp.shape[0], kind, dims, path)
    ref = _refs(oracle, (kind, dims), Asp, True)
    _run_all_placements(ctx, A, ref, _modes(ref))


GS_TPL_SHAPE = ("5pt", (200, 61))  # the smallest of test_hybrid_gs_template_kernel's shapes


@pytest.mark.parametrize("tpl_gs", ["templates", "ell", "split"])
def test_gs_template_paths_guard_bands(ctx, oracle, monkeypatch, tpl_gs):
    """test_hybrid_gs_template_kernel's knobs: the acc + chain template pair, sliced ELL, split."""
    import raptor_amd as ra

    if tpl_gs in ("ell", "split"):
        monkeypatch.setenv("AMG_GS_TEMPLATES", "0")
    if tpl_gs == "split":
        monkeypatch.setenv("AMG_GS_SPLIT_NPR", "0")
    else:
        monkeypatch.setenv("AMG_GS_SPLIT", "0")
    kind, dims = GS_TPL_SHAPE
    Asp = _stencil(oracle, kind, dims)
    A = _dev(ra, ctx, Asp)
    assert A.info["tpl_master"] == 0
    ref = _refs(oracle, (kind, dims), Asp, True)
    _run_all_placements(ctx, A, ref, _modes(ref, vec=False), norm=False)
    assert A._info()["gs_split"] == (tpl_gs == "split")
    if tpl_gs != "split":
        # B = 64 here: templates stream ~50 B per row, sliced ELL >= 5 B per cell (the test above)
        A.hybrid_gs(_up(ctx, ref["x"]), _up(ctx, ref["b"]), ctx.empty(ref["nr"]), 8)
        per_row = A._info()["gs_bytes"] / ref["nr"]
        assert (per_row < 60) if tpl_gs == "templates" else (per_row > 60), per_row


# ---- c. degenerate lengths ------------------------------------------------------------------------
def _tiny(n, shape):
    d = np.array([4.0, 2.0, 8.0])[:n]
    if shape == "diag" or n == 1:
        return sp.diags([d], [0]).tocsr()
    off = -np.array([1.0, 3.0])[:n - 1]
    A = sp.diags([off, d, off], [-1, 0, 1]).tocsr()
    A.sort_indices()
    return A


@pytest.mark.parametrize("fmt", ["auto", "blocks", "csr"])
@pytest.mark.parametrize("shape", ["diag", "tridiag"])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_degenerate_lengths_guard_bands(ctx, oracle, n, shape, fmt):
    """load_pair's n - 2 clamp (n = 2, 3) and the 8-byte loads of a one-entry vector (n = 1)."""
    import raptor_amd as ra

    Asp = _tiny(n, shape)
    A = _dev(ra, ctx, Asp).set_format(fmt)
    assert A.info["n_local_rows"] == n and A.info["nnz_local"] == Asp.nnz
    ref = _refs(oracle, ("tiny", n, shape), Asp, True)
    _run_all_placements(ctx, A, ref, _modes(ref))


# ---- d. solver calls ------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("fam", ["jacobi", "gs"])
def test_solver_guard_bands(ctx, oracle, fam, graph):
    """cycle, solve(3) and pcg(3) with x and b inside an arena at odd starts: the bits and
    histories of a fresh solver on ordinary tensors, guards intact, b unchanged."""
    import raptor_amd as ra

    O = oracle
    _, b = K.problem(O, "7pt")
    n = b.size
    x0 = O.vec_uniform(n, 9)

    def solver():
        A = ra.par_stencil_grid(ctx, "7pt", K.PROBLEMS["7pt"])
        ml = ra.ParMultilevel(use_graph=graph, **K.product_options(fam)).setup(A)
        assert ml.num_levels >= 4 and ml.graph_enabled == graph
        return ml

    calls = [("cycle", lambda ml, x, bb: (ml.cycle(x, bb), None)[1]),
             ("solve", lambda ml, x, bb: ml.solve(x, bb, max_iter=3)[1]),
             ("pcg", lambda ml, x, bb: ml.pcg(x, bb, max_iter=3)[1])]
    want = {}
    ml = solver()
    for what, fn in calls:
        dx, db = _up(ctx, x0), _up(ctx, b)
        h = fn(ml, dx, db)
        want[what] = (to_host(ctx, dx), None if h is None else np.array(h))
    ml = solver()
    for what, fn in calls:
        ar = V.Arena().output("x", n, 1, init=x0).input("b", b, 3).upload(ctx)
        h = fn(ml, ar["x"], ar["b"])
        ar.download(ctx)
        d = _diff(ar.get("x"), want[what][0])
        assert d.size == 0, (what, d[:8])
        if h is not None:
            assert np.array_equal(bits(h), bits(want[what][1])), (what, h, want[what][1])
        _assert_clean(ar, what)


# ---- e. rectangular operators ---------------------------------------------------------------------
@pytest.mark.parametrize("env", list(RECT_ENV))
@pytest.mark.parametrize("hier", ["pmis_7pt", "sa_graph"])
def test_rectangular_guard_bands(ctx, oracle, monkeypatch, hier, env):
    """P_0 and R_0 of test_rectangular_operators' hierarchies: x of n_cols, y of n_rows."""
    import raptor_amd as ra

    _setenv(monkeypatch, RECT_ENV[env])
    if hier == "pmis_7pt":
        ml = ra.ParRugeStubenSolver(coarsen="pmis").setup(ra.par_stencil_grid(ctx, "7pt", (22, 21, 20)))
    else:
        ml = ra.ParSmoothedAggregationSolver().setup(ra.par_graph_laplacian(ctx, 120, 110))
    assert ml.num_levels >= 2
    for w in "PR":
        M = ml.level_matrix(0, w)
        rp, col, val = M.export()
        nr, nc = rp.size - 1, M.info["n_global_cols"]
        assert nr != nc
        ref = _refs(oracle, (hier, w), sp.csr_matrix((val, col, rp), shape=(nr, nc)), False)
        _run_all_placements(ctx, M, ref, _modes(ref))
        inf = M.info
        assert inf["deferred"] == 0
        if env == "rect_tile":
            assert inf["tile_line_bytes"] in (32, 64), w
        if env == "gather_int32":
            assert not inf["kernel_variant"] & 256


# ---- f. two loopback ranks ------------------------------------------------------------------------
@pytest.mark.parametrize("tpl", [False, True], ids=["csr", "templates"])
def test_two_ranks_guard_bands(oracle, monkeypatch, tpl):
    """test_slab_kernels_bit_exact's 7-pt slabs: each rank's operands in its own arena at odd
    starts -- the pack kernel reads the caller's x, the boundary blocks write the caller's y."""
    import raptor_amd as ra

    if tpl:
        monkeypatch.setenv("AMG_TPL_MIN_ROWS", "0")
    O = oracle
    dims = (14, 13, 17)
    Ao = O.gen_7pt(*dims)
    n = Ao.shape[0]
    x, b = O.vec_uniform(n, 3), O.vec_uniform(n, 4)
    want = {"mult": Ao.spmv(x), "residual": Ao.residual(x, b)}

    def rank(r, nr, world):
        ctx = loopback_ctx(r, nr, world)
        A = ra.par_stencil_grid(ctx, "7pt", dims)
        f, m = A.first_row, A.local_rows
        ar = V.Arena().input("x", x[f:f + m], 1).input("b", b[f:f + m], 3)
        ar.output("mult", m, 5).output("residual", m, 7).upload(ctx)
        A.mult(ar["x"], ar["mult"])
        A.residual(ar["x"], ar["b"], ar["residual"])
        ar.download(ctx)
        return f, m, ar, A.info["n_halo"], A.info["template_rows"]

    res = run_ranks(2, rank)
    assert sum(m for _, m, *_ in res) == n
    for f, m, ar, halo, tpl_rows in res:
        for k in ("mult", "residual"):
            d = _diff(ar.get(k), want[k][f:f + m])
            assert d.size == 0, (f, k, d[:8])
        _assert_clean(ar, f)
        assert halo > 0
        assert (0 < tpl_rows < m) if tpl else tpl_rows == 0


# ---- aliases --------------------------------------------------------------------------------------
def _check_aliases(ra, ctx, A, ref):
    """Allowed exact aliases give the out-of-place bits (= the reference's); every rejected
    combination raises before anything is written, and the context stays usable."""
    n = ref["nr"]
    x, b, xp = ref["x"], ref["b"], ref["xp"]
    # out of place, on ordinary tensors
    dx, db, dp = _up(ctx, x), _up(ctx, b), _up(ctx, xp)
    plain = {}
    for m in ("residual", "jacobi", "cheby"):
        out = ctx.empty(n)
        _call(A, m, dx, db, dp, out)
        plain[m] = to_host(ctx, out)
    plain["cheby_xx"] = to_host(ctx, A.chebyshev_step(dx, dx, db, ctx.empty(n), C1, C2))
    for m in ("residual", "jacobi", "cheby"):
        assert _diff(plain[m], ref[m]).size == 0, m
    assert _diff(plain["cheby_xx"], CH.cheby_step(ref["Ao"], ref["dinv"], x, x, b, C1, C2)).size == 0
    # allowed: the output is b (in-out in the arena), the Chebyshev output is x_prev, x_prev is x
    for mode, alias in (("residual", "b"), ("jacobi", "b"), ("cheby", "b"), ("cheby", "xp")):
        ar = V.Arena().input("x", x, 1)
        if alias == "b":
            ar.output("b", n, 3, init=b).input("xp", xp, 5)
        else:
            ar.input("b", b, 3).output("xp", n, 5, init=xp)
        ar.upload(ctx)
        _call(A, mode, ar["x"], ar["b"], ar["xp"], ar[alias])
        ar.download(ctx)
        d = _diff(ar.get(alias), plain[mode])
        assert d.size == 0, (mode, "out is", alias, d[:8])
        _assert_clean(ar, (mode, alias))
    ar = V.Arena().input("x", x, 1).input("b", b, 3).output("out", n, 5).upload(ctx)
    A.chebyshev_step(ar["x"], ar["x"], ar["b"], ar["out"], C1, C2)
    ar.download(ctx)
    assert _diff(ar.get("out"), plain["cheby_xx"]).size == 0
    _assert_clean(ar, "x_prev is x")
    # rejected
    ar = V.Arena().input("x", x, 1).input("b", b, 3).input("xp", xp, 5).output("out", n, 7).upload(ctx)
    sx, sb, sp_ = ar.start("x"), ar.start("b"), ar.start("xp")
    X, B_, P, OUT = ar["x"], ar["b"], ar["xp"], ar["out"]
    every = ["mult", "mult_add", "residual", "jacobi", "cheby", "gs64", "gsb64"]
    bad = []
    for out in (X, ar.view(sx + 8, n), ar.view(sx - 8, n)):   # output over x: all seven calls
        bad += [(m, X, B_, P, out) for m in every]
    for out in (ar.view(sb + 8, n), ar.view(sb - 8, n)):      # partially over b
        bad += [(m, X, B_, P, out) for m in ("residual", "jacobi", "cheby", "gs64", "gsb64")]
    bad += [("cheby", X, B_, P, ar.view(sp_ + 8, n)), ("cheby", X, B_, P, ar.view(sp_ - 8, n))]
    bad += [("gs64", X, B_, P, B_), ("gsb64", X, B_, P, B_)]  # GS output is b
    for mode, x_, b_, p_, out in bad:
        with pytest.raises(ra.AmgError):
            _call(A, mode, x_, b_, p_, out)
    # null vectors (x_prev alone may be None)
    null = [("mult", None, B_, P, OUT), ("mult", X, B_, P, None), ("mult_add", None, B_, P, OUT),
            ("residual", X, None, P, OUT), ("jacobi", X, None, P, OUT), ("cheby", X, None, P, OUT),
            ("cheby", None, B_, P, OUT), ("cheby", X, B_, P, None)]
    for g in ("gs64", "gsb64"):
        null += [(g, None, B_, P, OUT), (g, X, None, P, OUT), (g, X, B_, P, None)]
    for mode, x_, b_, p_, out in null:
        with pytest.raises(ra.AmgError):
            _call(A, mode, x_, b_, p_, out)
    for x_, b_ in ((None, B_), (X, None)):
        with pytest.raises(ra.AmgError):
            A.residual_norm(x_, b_)
    ar.download(ctx)
    c = ar.changed()
    assert c.size == 0, ("a rejected call wrote", [ar.owner(i) for i in c[:8]])
    # the context and the operator stay usable
    A.mult(X, OUT)
    ar.download(ctx)
    assert _diff(ar.get("out"), ref["mult"]).size == 0
    _assert_clean(ar, "mult after the rejections")


@pytest.mark.parametrize("fmt,var", CONFIGS, ids=CFG_IDS)
@pytest.mark.parametrize("name", ALIAS_ZOO)
def test_zoo_aliases(ctx, oracle, monkeypatch, name, fmt, var):
    import raptor_amd as ra

    c = E.zoo()[name]
    _setenv(monkeypatch, c.env, {} if var is None else {"AMG_KERNEL_VARIANT": var})
    A = _dev(ra, ctx, c.A).set_format(fmt)
    _assert_zoo_path(ra, A, c, fmt)
    _check_aliases(ra, ctx, A, _refs(oracle, name, c.A, True))


@pytest.mark.parametrize("path", list(TPL_PATHS))
@pytest.mark.parametrize("kind,dims", STENCILS[:2], ids=STENCIL_IDS[:2])
def test_stencil_aliases(ctx, oracle, monkeypatch, kind, dims, path):
    import raptor_amd as ra

    Asp = _stencil(oracle, kind, dims)
    _setenv(monkeypatch, TPL_PATHS[path])
    A = _dev(ra, ctx, Asp)
    _assert_tpl_path(A, Asp.shape[0], kind, dims, path)
    _check_aliases(ra, ctx, A, _refs(oracle, (kind, dims), Asp, True))


def test_solver_vectors_rejected(ctx, oracle):
    """cycle / solve / pcg / cycle_timeline: x overlapping b and null vectors raise, nothing is
    written, and the solver still gives a fresh solver's bits afterwards."""
    import raptor_amd as ra

    O = oracle
    _, b = K.problem(O, "7pt")
    n = b.size
    x0 = O.vec_uniform(n, 9)
    A = ra.par_stencil_grid(ctx, "7pt", K.PROBLEMS["7pt"])
    ml = ra.ParMultilevel(**K.product_options("jacobi")).setup(A)
    dx, db = _up(ctx, x0), _up(ctx, b)
    ml.cycle(dx, db)
    want = to_host(ctx, dx)
    ml = ra.ParMultilevel(**K.product_options("jacobi")).setup(A)
    ar = V.Arena().output("x", n, 1, init=x0).input("b", b, 3).upload(ctx)
    X, B_, sb = ar["x"], ar["b"], ar.start("b")
    for x_, b_ in ((B_, B_), (ar.view(sb + 8, n), B_), (ar.view(sb - 8, n), B_), (None, B_), (X, None)):
        for call in (lambda: ml.cycle(x_, b_), lambda: ml.solve(x_, b_, max_iter=3),
                     lambda: ml.pcg(x_, b_, max_iter=3), lambda: ml.cycle_timeline(x_, b_, reps=1)):
            with pytest.raises(ra.AmgError):
                call()
    ar.download(ctx)
    assert ar.changed().size == 0
    ml.cycle(X, B_)
    ar.download(ctx)
    assert _diff(ar.get("x"), want).size == 0
    _assert_clean(ar, "cycle after the rejections")


# ---- utility kernels ------------------------------------------------------------------------------
def _random_bits(n, seed):
    """Random bit patterns with NaNs, infinities and both zeros among them."""
    v = np.random.default_rng(seed).integers(0, 1 << 63, n, dtype=np.uint64) << np.uint64(1)
    v = v ^ np.random.default_rng(seed + 1).integers(0, 2, n, dtype=np.uint64)
    special = bits(np.array([np.nan, -np.nan, np.inf, -np.inf, 0.0, -0.0]))
    k = min(n, special.size)
    v[:k] = special[:k]
    return v.view(np.float64)


@pytest.mark.parametrize("n", V.COPY_SIZES)
def test_vector_copy(ctx, n):
    import raptor_amd as ra

    src = _random_bits(n, 17 + n)
    ar = V.Arena().input("src", src, 0).output("dst", n, 2).upload(ctx)
    ra.vector_copy(ctx, ar["src"], ar["dst"])
    ar.download(ctx)
    d = _diff(ar.get("dst"), src)
    assert d.size == 0, d[:8]
    _assert_clean(ar, n)


def test_vector_copy_needs_16_bytes(ctx):
    import raptor_amd as ra

    n = 2049
    src = _random_bits(n, 3)
    ar = V.Arena().input("src", src, 0).input("src8", src, 1).output("dst", n, 2).output("dst8", n, 3).upload(ctx)
    for s, d in (("src8", "dst"), ("src", "dst8"), ("src8", "dst8")):
        with pytest.raises(ra.AmgError, match="16-byte aligned"):
            ra.vector_copy(ctx, ar[s], ar[d])
    with pytest.raises(ra.AmgError, match="16-byte aligned"):
        ra.vector_read(ctx, ar["src8"], ar["dst"])
    ar.download(ctx)
    assert ar.changed().size == 0


@pytest.mark.parametrize("n", V.COPY_SIZES)
def test_vector_read(ctx, n):
    import raptor_amd as ra

    src = V.read_data(n)
    want = V.read_partials_expected(src)
    cnt = V.read_partial_count(n)
    ar = V.Arena().input("src", src, 0).output("part", cnt + 8, 1).upload(ctx)
    ra.vector_read(ctx, ar["src"], ar["part"])
    ar.download(ctx)
    got = ar.get("part")
    if n < 2:
        assert ar.untouched("part")  # no pair: nothing is launched
    else:
        d = _diff(got[:cnt], want)
        assert d.size == 0, (d[:8], got[:cnt][d[:8]], want[d[:8]])
        assert ar.untouched("part", cnt)
    _assert_clean(ar, n)
    if cnt > 4:
        with pytest.raises(ra.AmgError, match="too few"):
            ra.vector_read(ctx, ar["src"], ar.view(ar.start("part"), cnt - 1))
    with pytest.raises(ra.AmgError, match="too few"):
        ra.vector_read(ctx, ar["src"], ar.view(ar.start("part"), 3))


def _uniform(ra, ctx, out, n, gid, seed):
    ra.check(ra.lib().amg_vector_uniform(ctx.h, int(n), int(gid), C.c_uint64(seed), ra._ptr(out)))


def test_vector_uniform(ctx, oracle):
    import raptor_amd as ra

    for n in V.UNIFORM_SIZES:
        for gid in V.UNIFORM_GIDS:
            for seed in V.UNIFORM_SEEDS:
                ar = V.Arena().output("out", n, 1).upload(ctx)
                _uniform(ra, ctx, ar["out"], n, gid, seed)
                ar.download(ctx)
                d = _diff(ar.get("out"), oracle.vec_uniform(n, seed, gid))
                assert d.size == 0, (n, gid, seed, d[:8])
                _assert_clean(ar, (n, gid, seed))


@pytest.mark.parametrize("gid,seed", list(zip(V.UNIFORM_GIDS, V.UNIFORM_SEEDS)))
def test_vector_uniform_stride_loop(ctx, oracle, gid, seed):
    """More entries than the largest grid has lanes: the grid-stride loop runs a second time."""
    import raptor_amd as ra

    n = V.UNIFORM_STRIDE_SIZE
    ar = V.Arena().output("out", n, 1).upload(ctx)
    _uniform(ra, ctx, ar["out"], n, gid, seed)
    ar.download(ctx)
    d = _diff(ar.get("out"), oracle.vec_uniform(n, seed, gid))
    assert d.size == 0, (gid, seed, d[:8])
    _assert_clean(ar, (gid, seed))


def test_memset_and_memcpy_stay_in_range(ctx):
    """amg_memset_async and amg_memcpy on a sub-range of an arena: the bytes inside are set or
    copied, the canaries around them stay."""
    import raptor_amd as ra

    n = 1000
    data = _random_bits(n, 23)
    ar = V.Arena().output("set", n, 1).output("cpy", n, 3).input("src", data, 5).upload(ctx)
    L = ra.lib()
    base = ar.dev.data_ptr()
    lo, cnt = 17, 901
    ra.check(L.amg_memset_async(ctx.h, C.c_void_p(base + 8 * (ar.start("set") + lo)), 0xA5, 8 * cnt))
    ra.check(L.amg_memcpy(ctx.h, C.c_void_p(base + 8 * (ar.start("cpy") + lo)),
                          C.c_void_p(base + 8 * (ar.start("src") + lo)), 8 * cnt))
    host = np.ascontiguousarray(data[:cnt])  # host to device as well
    ra.check(L.amg_memcpy(ctx.h, C.c_void_p(base + 8 * ar.start("cpy")), host.ctypes.data_as(C.c_void_p), 8 * lo))
    ar.download(ctx)
    got = bits(ar.get("set"))
    assert np.all(got[lo:lo + cnt] == np.uint64(0xA5A5A5A5A5A5A5A5))
    assert ar.untouched("set", 0, lo) and ar.untouched("set", lo + cnt)
    got = ar.get("cpy")
    assert _diff(got[lo:lo + cnt], data[lo:lo + cnt]).size == 0 and _diff(got[:lo], data[:lo]).size == 0
    assert ar.untouched("cpy", lo + cnt)
    _assert_clean(ar, "memset / memcpy")
