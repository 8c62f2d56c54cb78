"""Operators that put the setup half -- strength, PMIS / MIS(2), classical interpolation in its
thread and wave forms, SA filtering and smoothing, R = P^T, the drop tolerance and the
Galerkin SpGEMM -- on the branches and table limits that M-matrix stencils never reach.

Plain numpy / scipy.  Every builder returns a sorted square CSR matrix and a small dict of the
claims it makes about itself; tests/test_setup_edges_cpu.py checks each claim with the CPU
oracle, and tests/test_gpu_setup_edges.py gives the same operators to the device kernels.

Values are dyadic rationals where a claim needs exactness (ties, order-sensitive sums) and come
from numpy.random.Generator(PCG64(seed)) elsewhere.  Every setup operator is strictly
diagonally dominant in absolute value, except the rows a case names (`undominated`)."""
from __future__ import annotations

import functools
import os
from dataclasses import dataclass, field

import numpy as np
import scipy.sparse as sp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
K_IW_MAX = 512     # setup_device.hip kIwMax: longer rows run the thread loops on lane 0
K_IW_WAVES = 4     # rows per workgroup of the wave interpolation
K_T = 256          # rows per workgroup of the thread-per-row setup kernels
WAVE_NPR = 12      # default AMG_INTERP_WAVE_NPR: wave form from nnz >= 12 n
ULP = 2.0 ** -52
GOLD = 0x9E3779B97F4A7C15  # the golden-ratio multiplier of the hashes


def _csr(M):
    M = sp.csr_matrix(M)
    M.sort_indices()
    return sp.csr_matrix((M.data.astype(np.float64), M.indices.astype(np.int64), M.indptr.astype(np.int64)),
                         shape=M.shape)


def _from_coo(n, i, j, v):
    """CSR from triplets that name every (i, j) once: explicit zeros and signs are kept."""
    i, j, v = np.asarray(i, np.int64), np.asarray(j, np.int64), np.asarray(v, np.float64)
    assert np.unique(i * n + j).size == i.size, "duplicate entry"
    order = np.lexsort((j, i))
    rp = np.zeros(n + 1, np.int64)
    np.add.at(rp, i + 1, 1)
    return sp.csr_matrix((v[order], j[order], np.cumsum(rp)), shape=(n, n))


def _with_dominant_diagonal(W, margin, flip=None):
    """W (no diagonal) + diag(sum_j |w_ij| + margin); rows in `flip` get the negative of it."""
    d = np.asarray(abs(W).sum(axis=1)).ravel() + margin
    if flip is not None:
        d[flip] = -d[flip]
    return _csr(W + sp.diags(d))


def dominance(A):
    """min over rows of |a_ii| - sum_{j != i} |a_ij| (rows without a stored diagonal: a_ii = 0)."""
    A = sp.csr_matrix(A)
    d = A.diagonal()
    return np.abs(d) - (np.asarray(abs(A).sum(axis=1)).ravel() - np.abs(d))


@dataclass
class Case:
    """One setup operator.  `pmis` / `sa`: the options of the coarsenings it is listed for
    (None: not listed); `claims`: what the builder says about it; `undominated`: rows that are
    not diagonally dominant on purpose; `cuts`: rank starts of its 2- and 3-rank partitions."""
    name: str
    A: sp.csr_matrix
    claims: dict = field(default_factory=dict)
    pmis: dict | None = None
    sa: dict | None = None
    undominated: tuple = ()
    cuts: dict = field(default_factory=dict)
    one_level: bool = False


# ---- mixed ------------------------------------------------------------------------------------
def mixed_graph(n, deg, seed):
    """The recipe of tests/golden's mixed_600, restated: deg random partners per node
    (Generator(PCG64(seed))), couplings -U(0.5, 1.5), one in eight replaced by +U(0.05, 0.6),
    symmetrised (W + W^T) / 2, diagonal sum_j |a_ij| + 0.01."""
    rng = np.random.Generator(np.random.PCG64(seed))
    i = np.repeat(np.arange(n), deg)
    j = rng.integers(0, n, size=n * deg)
    keep = i != j
    i, j = i[keep], j[keep]
    w = -rng.uniform(0.5, 1.5, size=i.size)
    pos = rng.integers(0, 8, size=i.size) == 0
    w[pos] = rng.uniform(0.05, 0.6, size=int(pos.sum()))
    W = sp.coo_matrix((w, (i, j)), shape=(n, n)).tocsr()
    W = ((W + W.T) * 0.5).tocsr()
    W.sum_duplicates()
    d = np.asarray(abs(W).sum(axis=1)).ravel() + 0.01
    return _csr(W + sp.diags(d))


def mixed_600():
    """The Ain stored with the mixed_600 fixtures: positive couplings in one entry of eight, so
    F rows have strong F neighbours whose rows hold both signs inside C_i (the sign selection
    drops the positive ones) and SA's signed strength and filtered operator see weak and
    positive entries."""
    z = np.load(os.path.join(GOLDEN, "setup_mixed_600_sa_gs_mc16.npz"))
    A = sp.csr_matrix((z["Ain_data"], z["Ain_indices"], z["Ain_indptr"]), shape=tuple(z["Ain_shape"]))
    return Case("mixed_600", _csr(A), dict(positive_fraction_min=0.05, sign_selected_min=20),
                pmis=dict(strong_threshold=0.25, max_coarse=16), sa=dict(strong_threshold=0.08, max_coarse=16),
                cuts={2: [0, 311], 3: [0, 173, 402]})


def mixed_2500():
    """mixed_graph(2500, 6, 23): rows of about 13 entries (nnz >= 12 n: the wave form by
    default), positive couplings as above."""
    A = mixed_graph(2500, 6, 23)
    return Case("mixed_2500", A, dict(positive_fraction_min=0.05, sign_selected_min=100, wave_default=True),
                pmis=dict(strong_threshold=0.25, max_coarse=16), sa=dict(strong_threshold=0.08, max_coarse=16),
                cuts={2: [0, 1301], 3: [0, 777, 1803]})


# ---- positive rows ----------------------------------------------------------------------------
def _grid_edges(nx, ny):
    idx = np.arange(nx * ny).reshape(ny, nx)
    e = np.concatenate([np.stack([idx[:, :-1].ravel(), idx[:, 1:].ravel()]),
                        np.stack([idx[:-1, :].ravel(), idx[1:, :].ravel()])], axis=1)
    return e[0], e[1]


def positive_rows():
    """26 x 26 five-point grid, couplings -1, diagonal 4.5.  Rows `with_dependents` (every
    point (x, y) with x % 5 == 2 and y % 5 == 2) have their own off-diagonals set to +1/2 while
    their neighbours keep -1 towards them: classical strength finds mx <= 0 (no strong set) but
    the row has dependents, so PMIS leaves it undecided and, having no strong neighbour that
    could turn it F, it ends C.  Rows `without_dependents` (x % 5 == 4 and y % 5 == 0) are
    positive in the row AND in the column: no strong set and |S^T_i| = 0, pmis_init marks them
    F, and with no strong C neighbour interpolation gives an empty P row (nci == 0) -- an empty
    column run in R = P^T's input.  SA's signed strength keeps no entry of the second kind in
    either direction: singleton aggregates."""
    nx = ny = 26
    n = nx * ny
    a, b = _grid_edges(nx, ny)
    i = np.concatenate([a, b])
    j = np.concatenate([b, a])
    v = -np.ones(i.size)
    x, y = np.arange(n) % nx, np.arange(n) // nx
    dep = (x % 5 == 2) & (y % 5 == 2)
    nodep = (x % 5 == 4) & (y % 5 == 0)
    assert not (dep & nodep).any()
    v[dep[i] | nodep[i]] = 0.5          # the row
    v[nodep[j]] = 0.5                   # and, for the second kind, the column
    W = _from_coo(n, i, j, v)
    A = _csr(W + sp.diags(np.full(n, 4.5)))
    return Case("positive_rows", A,
                dict(with_dependents=np.flatnonzero(dep), without_dependents=np.flatnonzero(nodep)),
                pmis=dict(strong_threshold=0.25, max_coarse=16), sa=dict(strong_threshold=0.08, max_coarse=16))


# ---- negative / missing diagonal of a strong F neighbour ---------------------------------------
def negative_diagonal():
    """banded(640, 5, width=4) (neighbours i +- 1..4 share most of their neighbours, so a strong F
    neighbour's row reaches into C_i) with every row k % 3 == 1 multiplied by -1: a_kk < 0, and
    the row holds positive entries (its former negative couplings) next to negative ones.  The
    other rows are unchanged, so a_ik < 0 stays strong in row i, and wherever PMIS leaves both i
    and k fine, s_k is formed with pos == false: the positive entries of row k inside C_i."""
    A = banded(640, 5, width=4)
    rows = np.arange(1, 640, 3)
    s = np.ones(640)
    s[rows] = -1.0
    A = _csr(sp.diags(s) @ A)
    return Case("negative_diagonal", A, dict(negated=rows, neg_arm_min=30),
                pmis=dict(strong_threshold=0.25, max_coarse=16), cuts={2: [0, 333], 3: [0, 201, 455]})


def no_diagonal_neighbour():
    """banded(640, 9, width=4) with the stored diagonal removed from every row k % 7 == 3: a
    strong F neighbour k of such a kind has akk = 0, so pos == false and only the positive
    entries of its row inside C_i form s_k (often none: s_k == 0 and a_ik moves into d).
    Neither from_csr nor the setup validates the diagonal, so the operator is kept; it is set up
    (PMIS, classical interpolation) but never smoothed or solved -- Jacobi would divide by the
    missing diagonal -- and SA, whose smoothing scales by 1 / a_ii, is not listed for it.  In
    those rows the couplings to k +- 4 are divided by 16, so they are weak and the row's own
    denominator d = 0 + (weak couplings) is not zero where the row is fine itself.  The
    rows without a diagonal are not diagonally dominant themselves (`undominated`); every other
    row is."""
    A = banded(640, 9, width=4).tocoo()
    rows = np.arange(3, 640, 7)
    drop = (A.row == A.col) & np.isin(A.row, rows)
    far = np.isin(A.row, rows) & (np.abs(A.row - A.col) == 4)
    data = np.where(far, A.data / 16.0, A.data)  # weak in those rows: their own d is not 0
    A = _from_coo(640, A.row[~drop], A.col[~drop], data[~drop])
    return Case("no_diagonal_neighbour", _csr(A), dict(no_diagonal=rows, zero_diag_arm_min=10),
                pmis=dict(strong_threshold=0.25, max_coarse=16), undominated=tuple(rows.tolist()))


# ---- s_k == 0 ------------------------------------------------------------------------------------
SK_TILE = 9  # c1, c2, i, k, k2, and two leaves on each of c1, c2


def sk_zero(tiles=200, seed=31):
    """A nine-point gadget tiled `tiles` times (values scaled per entry by U(0.9, 1.1), tiles
    chained by one weak coupling c2(t) -- c1(t + 1) of -1/64):

        c1: i, k2 and two leaves depend on it      c2: k and two leaves depend on it
        i : a_i,c1 = -1, a_ik = -3/4, a_i,k2 = -1/2 (all strong at theta = 1/4)
        k : a_k,c2 = -1 strong; a_ki = -1/8 weak; in odd tiles a_k,c1 = +1/4
        k2: a_k2,c1 = -1 strong; a_k2,i = -1/8 weak

    Nothing depends on i (|S^T_i| = 0: pmis_init marks it F); c1 and c2 carry the largest
    measures of their neighbourhoods and become C; k, k2 and the leaves then see a strong C
    neighbour and become F.  So C_i = {c1}; row k has no negative entry in C_i (none at all in
    even tiles, a positive one in odd tiles): s_k == 0 and a_ik is added to d.  Row k2 has
    a_k2,c1 < 0: s_k2 != 0.  Both arms occur in row i."""
    rng = np.random.Generator(np.random.PCG64(seed))
    n = SK_TILE * tiles
    I, J, V = [], [], []

    def sym(a, b, vab, vba):
        I.extend([a, b]); J.extend([b, a]); V.extend([vab, vba])

    for t in range(tiles):
        o = SK_TILE * t
        c1, c2, i, k, k2 = o, o + 1, o + 2, o + 3, o + 4
        f = lambda: rng.uniform(0.9, 1.1)
        sym(i, c1, -1.0 * f(), -1.0 * f())
        sym(i, k, -0.75 * f(), -0.125 * f())
        sym(i, k2, -0.5 * f(), -0.125 * f())
        sym(k, c2, -1.0 * f(), -1.0 * f())
        sym(k2, c1, -1.0 * f(), -1.0 * f())
        if t % 2:
            sym(k, c1, 0.25 * f(), 0.25 * f())
        for leaf, c in ((o + 5, c1), (o + 6, c1), (o + 7, c2), (o + 8, c2)):
            sym(leaf, c, -1.0 * f(), -1.0 * f())
        if t + 1 < tiles:
            sym(c2, o + SK_TILE, -2.0 ** -6, -2.0 ** -6)
    W = _from_coo(n, I, J, V)
    A = _with_dominant_diagonal(W, 0.25)
    rows_i = SK_TILE * np.arange(tiles) + 2
    # cuts inside a tile, between i and k / between k and k2: ghost strong F neighbours
    return Case("sk_zero", A, dict(rows_i=rows_i, both_arms_min=tiles),
                pmis=dict(strong_threshold=0.25, max_coarse=16),
                cuts={2: [0, SK_TILE * 97 + 3], 3: [0, SK_TILE * 61 + 3, SK_TILE * 140 + 4]})


# ---- hub rows -------------------------------------------------------------------------------------
HUB_LENGTHS = (63, 64, 65, 127, 128, 129, 511, 512, 513, 600)
HUB_GRID = (40, 40)


def hub():
    """A 40 x 40 five-point grid (couplings -1, diagonal 6) and ten hub rows placed in front of
    it (rows 0..9).  Hub h has L = HUB_LENGTHS[h] - 1 couplings of exactly -1 to grid points
    0 .. L-1 (diagonal L + 1): all equal, all strong, row length HUB_LENGTHS[h].  A grid point's
    coupling back to a hub is -1/16 < theta max = 1/4: weak.  So nothing depends on a hub,
    |S^T_hub| = 0 and pmis_init marks it F; the grid points split among themselves as a grid
    does, and a hub's strong set holds that share of C and of F points: nci and the strong F
    neighbour count each pass 64 from L >= 192 on (the CPU module reads both off the oracle's
    split).  Rows of 513 and 600 entries exceed kIwMax.  Grid points 0..61 neighbour every hub:
    the coarse points among them get R rows through all ten hub rows of A P, whose lengths add
    up past the SpGEMM's symbolic limits (ub > 128 and ub > 1024)."""
    nx, ny = HUB_GRID
    ng, nh = nx * ny, len(HUB_LENGTHS)
    a, b = _grid_edges(nx, ny)
    I = [a + nh, b + nh]
    J = [b + nh, a + nh]
    V = [-np.ones(a.size), -np.ones(a.size)]
    for h, length in enumerate(HUB_LENGTHS):
        L = length - 1
        g = np.arange(L) + nh
        I += [np.full(L, h), g]
        J += [g, np.full(L, h)]
        V += [-np.ones(L), np.full(L, -1.0 / 16)]
    n = ng + nh
    W = _from_coo(n, np.concatenate(I), np.concatenate(J), np.concatenate(V))
    d = np.full(n, 6.0)
    d[:nh] = np.array(HUB_LENGTHS, np.float64)  # L + 1
    A = _csr(W + sp.diags(d))
    return Case("hub", A, dict(hubs=np.arange(nh), lengths=np.array(HUB_LENGTHS)),
                pmis=dict(strong_threshold=0.25, max_coarse=16), sa=dict(strong_threshold=0.08, max_coarse=16),
                # cuts through the hubs' shared neighbourhood (grid points 0..598 are rows 10..608)
                cuts={2: [0, 37], 3: [0, 137, 431]})


# ---- ties ------------------------------------------------------------------------------------------
def ties_classical(n=600):
    """Band operator for theta = 1/4: every row couples to i +- 1 with -4 (the maximum, so the
    threshold theta m_i is exactly 1), to i +- 2 with -1 (tie: strong by >=), to i +- 3 with
    -(1 - 2^-52) (weak by one unit in the last place) and to i +- 4 with -(1 + 2^-52) (strong);
    diagonal 32.  All products theta * m_i are exact."""
    offs = {1: -4.0, 2: -1.0, 3: -(1.0 - ULP), 4: -(1.0 + ULP)}
    diags, ks = [np.full(n, 32.0)], [0]
    for o, v in offs.items():
        diags += [np.full(n - o, v)] * 2
        ks += [o, -o]
    A = _csr(sp.diags(diags, ks, format="csr"))
    return Case("ties_classical", A, dict(strong_offsets=(1, 2, 4), weak_offsets=(3,)),
                pmis=dict(strong_threshold=0.25, max_coarse=16))


def ties_sa(n=600):
    """Chain for SA's signed strength at strong_threshold = 1/4: even points have diagonal 16,
    odd points 4, so theta sqrt(|a_ii a_jj|) = 1/4 sqrt(64) = 2 exactly (the square root of 64
    is exact).  The coupling between i and i + 1 cycles through -2 (tie: strong), -1 (weak),
    -(2 - 2^-52) (one unit in the last place below 2: weak), -1, -(2 + 2^-51) (one unit above:
    strong), -1; symmetric.  An odd row holds one of the three near-ties and one -1, so its
    off-diagonals stay below its diagonal 4."""
    vals = [-2.0, -1.0, -(2.0 - ULP), -1.0, -(2.0 + 2 * ULP), -1.0]
    e = np.array([vals[t % len(vals)] for t in range(n - 1)])
    d = np.where(np.arange(n) % 2 == 0, 16.0, 4.0)
    A = _csr(sp.diags([e, d, e], [-1, 0, 1], format="csr"))
    return Case("ties_sa", A, dict(edge_values=e, strong_edges=np.isin(np.arange(n - 1) % len(vals), (0, 4))),
                sa=dict(strong_threshold=0.25, max_coarse=16), pmis=dict(strong_threshold=0.25, max_coarse=16))


# ---- kernel block edges ---------------------------------------------------------------------------
SIZES = (1, 2, 3, 255, 256, 257, 258, 1023)


def banded(n, seed, width=3):
    """Seeded symmetric band operator, couplings -U(0.5, 1.5) with one in eight +U(0.05, 0.6),
    diagonal sum_j |a_ij| + 0.5."""
    rng = np.random.Generator(np.random.PCG64(seed))
    diags, ks = [], []
    for o in range(1, min(width, n - 1) + 1):
        v = -rng.uniform(0.5, 1.5, size=n - o)
        pos = rng.integers(0, 8, size=n - o) == 0
        v[pos] = rng.uniform(0.05, 0.6, size=int(pos.sum()))
        diags += [v, v]
        ks += [o, -o]
    W = sp.diags(diags, ks, shape=(n, n), format="csr") if diags else sp.csr_matrix((n, n))
    return _with_dominant_diagonal(W, 0.5)


def sizes(n):
    """n on either side of kT = 256 rows per workgroup of the thread kernels (255, 256, 257), not
    a multiple of kIwWaves = 4 rows per workgroup of the wave kernel (255, 257, 258, 1023), and
    the degenerate 1, 2, 3.  max_coarse = 2: n = 3 still coarsens, n = 1 and 2 never do."""
    return Case(f"sizes_{n}", banded(n, 100 + n), dict(n=n),
                pmis=dict(strong_threshold=0.25, max_coarse=2), sa=dict(strong_threshold=0.08, max_coarse=2),
                one_level=n <= 2)


def avg12(short):
    """The two sides of the default wave rule nnz >= 12 n: a 300-row symmetric band of half
    width 6 has 13 n - 42 entries; dropping the pairs (i, i + 6) for the first 129 (short: 129
    and the one-sided entry (150, 156)) rows leaves exactly 12 n (12 n - 1: the thread form)."""
    n = 300
    A = banded(n, 77, width=6).tocoo()
    drop = (np.abs(A.row - A.col) == 6) & (np.minimum(A.row, A.col) < 129)
    if short:
        drop |= (A.row == 150) & (A.col == 156)
    A = _csr(_from_coo(n, A.row[~drop], A.col[~drop], A.data[~drop]))
    assert A.nnz == 12 * n - (1 if short else 0)
    return Case("avg12_below" if short else "avg12_at", A, dict(nnz=A.nnz, wave_default=not short),
                pmis=dict(strong_threshold=0.25, max_coarse=16))


PATH_RUN = 200  # points per stretch of the chain along which the PMIS / MIS(2) keys fall


def hash32(ids, seed):
    """The splitting's tie-break hash of DESIGN.md 3, restated in uint64 arithmetic:
    splitmix64(id xor seed * 0x9E3779B97F4A7C15) >> 32."""
    with np.errstate(over="ignore"):
        z = np.asarray(ids, np.uint64) ^ np.uint64((seed * GOLD) & ((1 << 64) - 1))
        z = z + np.uint64(GOLD)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return (z ^ (z >> np.uint64(31))) >> np.uint64(32)


def path(n=2000, seed=0x5EED):
    """The three-point chain (-1, 2.5, -1) through all n points, white box: the chain visits
    the points in stretches of PATH_RUN ids, each stretch sorted by hash32(id, seed) descending.
    Every interior point has |S^T_i| = 2, so along a stretch the PMIS keys fall monotonically:
    a round can only decide the stretch's highest undecided point (C) and the neighbour below
    it (F), two points, so PMIS needs at least PATH_RUN / 2 rounds where a chain in id order
    needs 3.  MIS(2) decides a root and the two points within distance two below it: at least
    PATH_RUN / 3 rounds.  The round loops run that long and end by their own 'nothing undecided'
    test."""
    ids = np.arange(n)
    h = hash32(ids, seed).astype(np.int64)
    order = np.concatenate([q + np.argsort(-h[q:q + PATH_RUN], kind="stable") for q in range(0, n, PATH_RUN)])
    a, b = order[:-1], order[1:]
    W = _from_coo(n, np.concatenate([a, b]), np.concatenate([b, a]), -np.ones(2 * (n - 1)))
    A = _csr(W + sp.diags(np.full(n, 2.5)))
    return Case("path", A, dict(order=order, pmis_rounds_min=PATH_RUN // 2, mis2_rounds_min=PATH_RUN // 3),
                pmis=dict(strong_threshold=0.25, max_coarse=16), sa=dict(strong_threshold=0.08, max_coarse=16))


@functools.lru_cache(maxsize=None)
def zoo():
    cases = [mixed_600(), mixed_2500(), positive_rows(), negative_diagonal(), no_diagonal_neighbour(),
             sk_zero(), hub(), ties_classical(), ties_sa()] + [sizes(n) for n in SIZES] + \
            [avg12(False), avg12(True), path()]
    for c in cases:
        c.A.data.setflags(write=False)
    return {c.name: c for c in cases}


def names(kind=None):
    """Case names; kind 'pmis' / 'sa': those listed for that coarsening."""
    return [k for k, c in zoo().items() if kind is None or getattr(c, kind) is not None]


def setups():
    """(name, coarsen) for every listed setup."""
    return [(k, kind) for k, c in zoo().items() for kind in ("pmis", "sa") if getattr(c, kind) is not None]


# ---- what the interpolation does on a split: the arms, counted ---------------------------------
def interp_arms(A, S, cf, lo=0, hi=None):
    """Per F row of A (scipy CSR) with strength S (scipy CSR pattern) and split cf: which arms
    of classical interpolation it takes.  Returns a dict of arrays over rows: nci (strong C
    neighbours), nsf (strong F neighbours), sk_zero / sk_nonzero (strong F neighbours by s_k),
    neg (strong F neighbours with a_kk <= 0: pos == false), neg_selected (of those, how many
    have a positive entry inside C_i), dropped_sign (entries of row k inside C_i that the sign
    selection leaves out), ghost_sf (strong F neighbours outside [lo, hi))."""
    A, S = sp.csr_matrix(A), sp.csr_matrix(S)
    n = A.shape[0]
    hi = n if hi is None else hi
    diag = A.diagonal()
    keys = ("nci", "nsf", "sk_zero", "sk_nonzero", "neg", "neg_selected", "dropped_sign", "ghost_sf")
    out = {k: np.zeros(n, np.int64) for k in keys}
    for i in range(n):
        if cf[i] == 1:
            continue
        strong = set(S.indices[S.indptr[i]:S.indptr[i + 1]].tolist()) - {i}
        ci = {j for j in strong if cf[j] == 1}
        out["nci"][i] = len(ci)
        sf = [j for j in A.indices[A.indptr[i]:A.indptr[i + 1]].tolist() if j in strong and cf[j] != 1]
        out["nsf"][i] = len(sf)
        if not ci:
            continue
        for k in sf:
            pos = diag[k] > 0.0
            sk, sel, dropped = 0.0, 0, 0
            for m, v in zip(A.indices[A.indptr[k]:A.indptr[k + 1]].tolist(), A.data[A.indptr[k]:A.indptr[k + 1]].tolist()):
                if m in ci:
                    if (v < 0.0) if pos else (v > 0.0):
                        sk += v
                        sel += 1
                    else:
                        dropped += 1
            out["sk_zero" if sk == 0.0 else "sk_nonzero"][i] += 1
            out["dropped_sign"][i] += dropped
            if not pos:
                out["neg"][i] += 1
                out["neg_selected"][i] += sel > 0
            if lo <= i < hi and not lo <= k < hi:
                out["ghost_sf"][i] += 1
    return out


# ---- SpGEMM operand pairs ----------------------------------------------------------------------------
SPGEMM_N = 8200
ROW_BINS = (1, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 4097, 8191, 8192, 8193)


def hslot(j, T):
    """spgemm.hip hslot, restated: ((j * 0x9E3779B97F4A7C15) mod 2^64) >> 40 & (T - 1)."""
    return ((int(j) * GOLD) % (1 << 64)) >> 40 & (T - 1)


@dataclass
class Pair:
    """SpGEMM operands A, B (square, same size) and, per claimed output row, the number of
    distinct columns and the bound ub = sum_k |B_k| the product's bins see."""
    name: str
    A: sp.csr_matrix
    B: sp.csr_matrix
    claims: dict = field(default_factory=dict)
    cuts: dict = field(default_factory=dict)


def _pair_from(name, n, a_rows, b_rows, claims, cuts=None, diag_a=True, diag_b=True):
    """a_rows / b_rows: {row: (cols, vals)}; every other row holds the diagonal only (1.0)."""
    def build(rows, diag):
        I, J, V = [], [], []
        for r in range(n):
            if r in rows:
                c, v = rows[r]
                I += [r] * len(c); J += list(c); V += list(v)
            elif diag:
                I.append(r); J.append(r); V.append(1.0)
        return _csr(_from_coo(n, I, J, V)) if I else sp.csr_matrix((n, n), dtype=np.float64)
    return Pair(name, build(a_rows, diag_a), build(b_rows, diag_b), claims, cuts or {})


def spgemm_row_bins():
    """For the t-th r of ROW_BINS, B rows 3t, 3t+1, 3t+2 hold the same r columns (a seeded
    choice out of 8200) with values 2^53 s_j, s_j and -2^53 s_j, s_j = 2^(j % 7 - 3): a power of
    two, so every product below is exact and the rounding is that of 2^53 + 1.  A row 1000 + 2t is the single entry (3t + 1, 1/2):
    one output row of r distinct columns with ub == r.  A row 1001 + 2t is (3t, 2), (3t+1, 2),
    (3t+2, 2): the same r columns, ub == 3 r, and in the canonical k order every column is
    (2^54 s + 2 s) - 2^54 s = 0.0 (2^54 s + 2 s is a tie and rounds to the even 2^54 s),
    while (2^54 s - 2^54 s) + 2 s and (2 s - 2^54 s) + 2^54 s both give 2 s.  Every other row of
    A and B is the diagonal entry 1, so rows 0..53 of the product repeat B's long rows
    (ub == r).  r = 8193 overflows the 8192-slot table (the host row); 8192 fills it (load
    factor 1, bitonic sort with P == T and no padding); 1024 fills the symbolic 1024-slot
    table; 1025 overflows it (the retry in 8192 slots); 128 / 129 and 512 / 513 and
    2048 / 2049 are the numeric bin boundaries."""
    n = SPGEMM_N
    rng = np.random.Generator(np.random.PCG64(7))
    a_rows, b_rows, rows = {}, {}, {}
    for t, r in enumerate(ROW_BINS):
        cols = np.sort(rng.choice(n, size=r, replace=False))
        s = 2.0 ** (cols % 7 - 3)
        b_rows[3 * t] = (cols, 2.0 ** 53 * s)
        b_rows[3 * t + 1] = (cols, s)
        b_rows[3 * t + 2] = (cols, -(2.0 ** 53) * s)
        a_rows[1000 + 2 * t] = ([3 * t + 1], [0.5])
        a_rows[1001 + 2 * t] = ([3 * t, 3 * t + 1, 3 * t + 2], [2.0, 2.0, 2.0])
        rows[1000 + 2 * t] = (r, r)
        rows[1001 + 2 * t] = (r, 3 * r)
        for q in range(3):
            rows[3 * t + q] = (r, r)
    # rank 0 owns B's long rows and an A of diagonal entries only (no halo); the A rows that
    # read them lie on the last rank: ghost rows of B, the 8192- and 8193-column ones included
    return _pair_from("row_bins", n, a_rows, b_rows, dict(rows=rows, order_rows=[1001 + 2 * t for t in range(len(ROW_BINS))]),
                      cuts={2: [0, 500], 3: [0, 500, 1017]})


def spgemm_empty():
    """Row 3 of A names columns 10, 11, 12, whose B rows are empty: a non-empty A row with an
    empty output row (count 0 in the symbolic pass, m == 0 in the numeric one).  Row 5 of A is
    empty.  Row 7 of A names one empty and one non-empty B row."""
    n = 300
    a_rows = {3: ([10, 11, 12], [1.0, 2.0, 3.0]), 5: ([], []), 7: ([10, 20], [1.5, 2.5])}
    b_rows = {10: ([], []), 11: ([], []), 12: ([], [])}
    return _pair_from("empty_rows", n, a_rows, b_rows, dict(empty_out=[3, 5], n_empty=2), cuts={2: [0, 6], 3: [0, 4, 11]})


def spgemm_zero_a():
    """nnz(A) == 0 against a diagonal B: no column to map, every bound 0, an empty product.  On
    several ranks no rank has a halo and the ghost-row exchange has length zero."""
    return _pair_from("nnz_a_0", 260, {}, {}, dict(nnz=0), cuts={2: [0, 130], 3: [0, 90, 170]}, diag_a=False)


def spgemm_zero_b():
    """A diagonal A against nnz(B) == 0: every A row names one empty B row; an empty B image."""
    return _pair_from("nnz_b_0", 260, {}, {}, dict(nnz=0), cuts={2: [0, 130], 3: [0, 90, 170]}, diag_b=False)


def spgemm_wrapped():
    """White box: rows whose columns are homed (hslot above) in the last 8 slots of a table, so
    linear probing wraps to slot 0.  Of the 8200 column ids only about 8200 * 8 / T are homed
    there, so 'all columns' is possible for T = 256 only; the larger tables get every such id
    plus filler, and more than 8 keys homed in 8 slots wrap whatever the insertion order.
      row 100: 24 ids homed in the last 8 of 256 slots; ub = count = 24 (both passes in 256);
      row 101: B rows 201..203 hold the same 40 ids homed in the last 8 of 1024 slots and row
               204 holds 16 more: ub = 136 > 128, so the symbolic pass runs in 1024 slots; the
               56 distinct columns put the numeric pass in 256 slots, where the same ids are
               homed in the last 8 as well ((z >> 40) & 255 >= 248);
      row 102: every id homed in the last 8 of 1024 slots and filler up to 300 distinct columns
               (numeric pass in 1024 slots);
      row 103: the same for 4096 slots with 600 distinct columns."""
    n = SPGEMM_N
    ids = np.arange(n)
    home = {T: np.array([j for j in ids if hslot(j, T) >= T - 8]) for T in (256, 1024, 4096)}
    rng = np.random.Generator(np.random.PCG64(19))
    val = lambda c: 1.0 + (np.asarray(c) % 16) / 16.0
    a_rows, b_rows = {}, {}
    c256 = home[256][:24]
    b_rows[200] = (c256, val(c256)); a_rows[100] = ([200], [1.0])
    c1k = home[1024][:40]
    extra = home[1024][40:56]
    for q in range(3):
        b_rows[201 + q] = (c1k, val(c1k) * (q + 1))
    b_rows[204] = (extra, val(extra))
    a_rows[101] = ([201, 202, 203, 204], [1.0, 0.5, 0.25, 2.0])

    def padded(core, total):
        rest = np.setdiff1d(ids, core)
        return np.sort(np.concatenate([core, rng.choice(rest, size=total - core.size, replace=False)]))

    c_n1k = padded(home[1024], 300)
    b_rows[205] = (c_n1k, val(c_n1k)); a_rows[102] = ([205], [1.0])
    c_n4k = padded(home[4096], 600)
    b_rows[206] = (c_n4k, val(c_n4k)); a_rows[103] = ([206], [1.0])
    claims = dict(homed={100: (256, 24, 24), 101: (1024, 56, 56), 102: (1024, int(home[1024].size), 300),
                         103: (4096, int(home[4096].size), 600)},
                  ub={100: 24, 101: 136, 102: 300, 103: 600})
    return _pair_from("wrapped_probes", n, a_rows, b_rows, claims, cuts={2: [0, 150], 3: [0, 102, 203]})


def spgemm_cancel():
    """Row 4 of A is (8, 1), (9, 1); B rows 8 and 9 hold column 2 with +3 and -3 (and columns 1
    and 5 without a partner): the terms of column 2 sum to exactly 0.0, and the stored zero
    stays in the product's pattern.  Row 6 does the same with -3 first (-3 + 3 = +0.0 again).
    Row 9 of A is (8, -1) alone: B[8, 1] is a stored 0.0, the term is -0.0, and the accumulator
    that starts at +0.0 keeps +0.0 -- compared through the bit patterns."""
    n = 300
    b_rows = {8: ([1, 2], [0.0, 3.0]), 9: ([2, 5], [-3.0, 1.0])}
    a_rows = {4: ([8, 9], [1.0, 1.0]), 6: ([8, 9], [-1.0, -1.0]), 9: ([8], [-1.0])}
    return _pair_from("exact_cancellation", n, a_rows, b_rows, dict(zero_at=[(4, 2), (6, 2), (9, 1)]),
                      cuts={2: [0, 7], 3: [0, 5, 9]})


@functools.lru_cache(maxsize=None)
def pairs():
    ps = [spgemm_row_bins(), spgemm_empty(), spgemm_zero_a(), spgemm_zero_b(), spgemm_wrapped(), spgemm_cancel()]
    for p in ps:
        p.A.data.setflags(write=False)
        p.B.data.setflags(write=False)
    return {p.name: p for p in ps}


def canonical_product(A, B, reverse_k=False, k_perm=None):
    """C = A B in the canonical order, pure Python: per row, k over A's row in CSR
    order, j over B's row k in its order, acc[j] += a * b from 0.0; columns sorted.  Explicit
    zeros are kept.  Perturbations for the liveness check: reverse_k runs the k loop backwards;
    k_perm (a permutation of 0..2) reorders the k steps of the rows that have exactly three."""
    A, B = sp.csr_matrix(A), sp.csr_matrix(B)
    ap, ai, av = A.indptr.tolist(), A.indices.tolist(), A.data.tolist()
    bp, bi, bv = B.indptr.tolist(), B.indices.tolist(), B.data.tolist()
    rp, ci, cv = [0], [], []
    for i in range(A.shape[0]):
        acc = {}
        ks = list(range(ap[i], ap[i + 1]))
        if k_perm is not None and len(ks) == 3:
            ks = [ks[t] for t in k_perm]
        for ka in (reversed(ks) if reverse_k else ks):
            k, a = ai[ka], av[ka]
            for q in range(bp[k], bp[k + 1]):
                acc[bi[q]] = acc.get(bi[q], 0.0) + a * bv[q]
        for j in sorted(acc):
            ci.append(j)
            cv.append(acc[j])
        rp.append(len(ci))
    return sp.csr_matrix((np.array(cv, np.float64), np.array(ci, np.int64), np.array(rp, np.int64)),
                         shape=(A.shape[0], B.shape[1]))


def bits(a):
    """The bit patterns of an fp64 array: -0.0 and 0.0 differ, equal NaNs compare equal."""
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(X, Y):
    """Two CSR matrices with identical shape, pattern and value bits."""
    X, Y = sp.csr_matrix(X), sp.csr_matrix(Y)
    return (X.shape == Y.shape and np.array_equal(X.indptr, Y.indptr) and np.array_equal(X.indices, Y.indices)
            and np.array_equal(bits(X.data), bits(Y.data)))
