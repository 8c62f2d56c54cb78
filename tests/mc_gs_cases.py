"""The multicolour Gauss-Seidel smoother (AMG_SMOOTH_MC_GS) restated for the tests:
the first-fit colouring as a sequential loop in key order, the sweep through the oracle's
Csr.jacobi with omega = 1 on the rows of one colour at a time, and a V-cycle scaffold over an
oracle hierarchy's exported A, P and R (cheby_cases.Scaffold; the hierarchy does not depend on
the smoother).  tests/test_mc_gs_cpu.py checks the restatement on the CPU, tests/test_gpu_mc_gs.py
runs the product against it.  numpy / scipy only."""
import numpy as np
import scipy.sparse as sp

from tests import bicgstab_cases as B
from tests import cheby_cases as CH
from tests import cycle_option_cases as K
from tests import setup_edge_cases as SE

SEED = 0x5EED        # amg_options.seed's default (level l is coloured with seed + l)
SLICE = 64           # kMcSlice: rows per slice; colours whose rows average more take a wave per row
WG_CAPACITY = 16384  # kMcWgCapacity: rows whose x fits the one-workgroup sweep's LDS
WG_ROWS = 16384      # kMcWgRows: the automatic path sweeps up to this many rows in one workgroup
MAX_COARSE = 64


# ---- the definition ------------------------------------------------------------------------------
def adjacency(A):
    """(indptr, indices) of G: the pattern of A u A^T without the diagonal.  Explicit zeros are
    entries (the pattern is taken from A's index arrays, never from its values)."""
    A = sp.csr_matrix(A)
    n = A.shape[0]
    P = sp.csr_matrix((np.ones(A.indices.size, np.int8), A.indices, A.indptr), shape=A.shape)
    G = (P + P.T).tocoo()
    keep = G.row != G.col
    G = sp.csr_matrix((np.ones(int(keep.sum()), np.int8), (G.row[keep], G.col[keep])), shape=(n, n))
    G.sort_indices()
    return G.indptr, G.indices


def key_order(n, seed, first_gid=0):
    """The global ids [first_gid, first_gid + n) in precedence order: key descending, then id."""
    ids = np.arange(first_gid, first_gid + n)
    key = SE.hash32(ids, seed).astype(np.int64)
    return np.lexsort((ids, -key))


def first_fit(A, seed):
    """colour(v) = the smallest c >= 0 no neighbour preceding v uses: a sequential loop in key
    order (when v's turn comes, its coloured neighbours are exactly the preceding ones).  Also
    the readiness rounds: round(v) = 1 + the largest round of a preceding neighbour."""
    rp, col = adjacency(A)
    n = rp.size - 1
    colour = np.full(n, -1, np.int32)
    rnd = np.zeros(n, np.int64)
    for v in key_order(n, seed):
        nb = col[rp[v]:rp[v + 1]]
        nb = nb[colour[nb] >= 0]
        used = set(colour[nb].tolist())
        c = 0
        while c in used:
            c += 1
        colour[v] = c
        rnd[v] = 1 + (rnd[nb].max() if nb.size else 0)
    return colour, int(rnd.max(initial=0))


def sweep(Ao, colour, x, b, backward=False):
    """One sweep on a copy of x: per colour c (ascending; descending when backward) the rows of c
    take Ao.jacobi(x, b, 1.0) of the current x."""
    x = np.array(x, np.float64, copy=True)
    nc = int(colour.max(initial=-1)) + 1
    for c in (range(nc - 1, -1, -1) if backward else range(nc)):
        rows = np.flatnonzero(colour == c)
        x[rows] = Ao.jacobi(x, b, 1.0)[rows]
    return x


def mc_scaffold(O, Ho, pre=1, post=1, seed=SEED):
    """The restated multicolour hierarchy over Ho's operators: forward sweeps before, backward
    sweeps after the coarse correction.  .colour / .rounds per smoothed level."""
    S = CH.Scaffold(O, Ho)
    S.pre, S.post = pre, post
    cr = [first_fit(Ho.matrix(l, "A"), seed + l) for l in range(S.nl - 1)]
    S.colour = [c for c, _ in cr]
    S.rounds = [r for _, r in cr]
    S.smoother = lambda l, x, b, x_zero, post_: sweep(S.A[l], S.colour[l], x, b, backward=post_)
    return S


def gs_scaffold(O, Ho, block):
    """Hybrid GS (the oracle's kernels) on the same scaffold: the yardstick of the 0.7 condition."""
    S = CH.Scaffold(O, Ho)
    S.smoother = lambda l, x, b, x_zero, post_: (S.A[l].hybrid_gs_backward(x, b, block) if post_
                                                 else S.A[l].hybrid_gs(x, b, block))
    return S


def cycles_to(S, b, tol, max_iter=400):
    """Cycles S.solve takes from x = 0 to a relative residual below tol."""
    _, h = S.solve(np.zeros(b.size), b, max_iter=max_iter, tol=tol)
    assert h[-1] / h[0] < tol, (len(h) - 1, h[-1] / h[0])
    return len(h) - 1


# ---- operators ------------------------------------------------------------------------------------
def _sp(csr):
    rp, col, val = csr
    return sp.csr_matrix((val, col, rp), shape=(rp.size - 1, rp.size - 1))


def upwind_lower(n, pe):
    """bicgstab_cases.upwind_chain without its superdiagonal: row i holds (i - 1, i) only, so the
    edge to i + 1 exists only in A^T -- a colouring of A's rows alone would be improper."""
    A = _sp(B.upwind_chain(n, pe)).tocoo()
    keep = A.col <= A.row
    return SE._csr(SE._from_coo(n, A.row[keep], A.col[keep], A.data[keep]))


def clique_and_chain(m, tail):
    """A dense m x m block (couplings -1, diagonal 2 m) beside a chain of `tail` points: the
    clique's rows take m different colours, the chain's only colours 0 and 1, so every colour
    >= 2 holds a single row -- of m entries: with m > 64 a wave colour whose second round of 64
    products is partial."""
    n = m + tail
    D = -np.ones((m, m)) + np.diag(np.full(m, 2.0 * m + 1.0))
    Cn = sp.diags([-np.ones(tail - 1), np.full(tail, 2.5), -np.ones(tail - 1)], [-1, 0, 1])
    return SE._csr(sp.block_diag([sp.csr_matrix(D), Cn], format="csr")), n


def operators(O):
    """name -> scipy CSR (int64 indices, sorted): the case list of the colouring and the sweep."""
    ops = {kind: K.problem(O, kind)[0].to_scipy() for kind in K.PROBLEMS}
    ops["convdiff"] = _sp(B.convdiff(*B.GRIDS[1], 8.0))        # nonsymmetric values
    ops["upwind_chain"] = _sp(B.upwind_chain(301, 2.0))
    ops["upwind_lower"] = upwind_lower(301, 2.0)                # nonsymmetric pattern: A^T matters
    ops["hub"] = SE.hub().A                                     # rows of 63 .. 600 entries, many colours
    ops["path"] = SE.path().A                                   # keys fall along the chain: long rounds
    for n in (SLICE - 1, SLICE, SLICE + 1):
        ops[f"rows_{n}"] = SE.banded(n, 100 + n)
    ops["single_row_colours"] = clique_and_chain(7, 30)[0]
    ops["wave_colours"] = clique_and_chain(80, 30)[0]
    out = {}
    for k, A in ops.items():
        A = SE._csr(A)
        A.data.setflags(write=False)
        out[k] = A
    return out


OPERATORS = ["7pt", "27pt", "convdiff", "upwind_chain", "upwind_lower", "hub", "path",
             f"rows_{SLICE - 1}", f"rows_{SLICE}", f"rows_{SLICE + 1}", "single_row_colours", "wave_colours"]


def cuts(n, nranks):
    """Rank starts and the end of the 1-, 2- and 3-way cuts (ragged; scaled to the operator)."""
    return {1: [0, n], 2: [0, n // 3, n], 3: [0, n // 7, (2 * n) // 3 + 1, n]}[nranks]


def first_fit_cut(A, seed, starts):
    """The colouring computed rank by rank as the device does: every rank colours its own rows
    in parallel readiness rounds, seeing other ranks' colours of the previous round only."""
    rp, col = adjacency(A)
    n = rp.size - 1
    ids = np.arange(n)
    key = SE.hash32(ids, seed).astype(np.int64)
    colour = np.full(n, -1, np.int32)
    rounds = 0
    while np.any(colour < 0):
        new = colour.copy()
        for lo, hi in zip(starts[:-1], starts[1:]):
            for v in range(lo, hi):
                if colour[v] >= 0:
                    continue
                nb = col[rp[v]:rp[v + 1]]
                before = nb[(key[nb] > key[v]) | ((key[nb] == key[v]) & (nb < v))]
                if np.any(colour[before] < 0):
                    continue
                used = set(colour[before].tolist())
                c = 0
                while c in used:
                    c += 1
                new[v] = c
        colour = new
        rounds += 1
    return colour, rounds


# ---- hierarchies -----------------------------------------------------------------------------------
def hierarchy(O, Ao, fam="sa", **over):
    return O.Hierarchy(Ao, **{**O.DEFAULTS[fam], "max_coarse": MAX_COARSE, **over})


def product_options(fam="sa", pre=1, post=1, max_coarse=MAX_COARSE, **over):
    return dict(coarsen=fam, smoother="mc_gs", pre_sweeps=pre, post_sweeps=post, max_coarse=max_coarse, **over)


def sa27(O, n):
    """BASELINE.json configs[2] at n^3: the anisotropic 27-point operator, b = A u."""
    Ao = O.gen_27pt(n, n, n)
    return Ao, Ao.spmv(O.vec_uniform(Ao.shape[0], 42))


def g3sub(O, n):
    """BASELINE.json configs[4]'s substitute at n^2: the seeded graph Laplacian in RCM order."""
    G = O.gen_graph_laplacian(n, n, seed=1)
    Ao = O.permute(G, O.rcm(G))
    return Ao, Ao.spmv(O.vec_uniform(Ao.shape[0], 42))
