"""Nonsymmetric operators and the numpy restatement of Solver::bicgstab
(raptor_amd/csrc/multilevel.hip): tests/test_bicgstab_cpu.py checks them on the CPU,
tests/test_gpu_bicgstab.py runs the product against them.

bicgstab_restated is the definition of include/raptor_amd.h over an oracle hierarchy and the
oracle's residual / spmv, with the dot product left open like cycle_option_cases.pcg_restated:
with dot_tree it has the product's alpha, omega and beta bit for bit.  numpy / scipy only."""
import numpy as np

KRYLOV_OK, KRYLOV_BREAKDOWN = 0, 1

GRIDS = [(16, 15, 14), (12, 11, 10)]   # 3,360 rows: two dot blocks, the second ragged; 1,320: one
PES = [0.0, 0.5, 8.0]
MAX_COARSE = 32
VELOCITY = (1.0, 0.5, 0.25)            # per axis, times the cell Peclet number


def _csr(n, rows, cols, vals):
    import scipy.sparse as sp

    M = sp.coo_matrix((vals, (rows, cols)), shape=(n, n)).tocsr()
    M.sort_indices()
    return M.indptr.astype(np.int64), M.indices.astype(np.int64), M.data.astype(np.float64)


def convdiff(nx, ny, nz, pe):
    """7-point diffusion plus first-order upwind convection, as (row_ptr, col, val) with the
    points in gen_7pt's order (x fastest).  Along an axis with velocity u pe the row of the upper
    neighbour couples to the lower one with -1 - u pe, the reverse coupling is -1, and every
    diagonal is sum over the axes of 2 + u pe (no boundary correction, as gen_7pt's 6)."""
    n = nx * ny * nz
    r = np.arange(n, dtype=np.int64)
    i, j, k = r % nx, (r // nx) % ny, r // (nx * ny)
    ux, uy, uz = (u * pe for u in VELOCITY)
    # a row's entries in ascending column order: z-, y-, x-, diagonal, x+, y+, z+
    entries = [(k > 0, -nx * ny, -1.0 - uz), (j > 0, -nx, -1.0 - uy), (i > 0, -1, -1.0 - ux),
               (None, 0, (2.0 + ux) + (2.0 + uy) + (2.0 + uz)),
               (i < nx - 1, 1, -1.0), (j < ny - 1, nx, -1.0), (k < nz - 1, nx * ny, -1.0)]
    keep = np.ones((n, 7), bool)
    col = np.empty((n, 7), np.int64)
    val = np.empty((n, 7), np.float64)
    for e, (mask, off, v) in enumerate(entries):
        if mask is not None:
            keep[:, e] = mask
        col[:, e] = r + off
        val[:, e] = v
    rp = np.zeros(n + 1, np.int64)
    np.cumsum(keep.sum(axis=1), out=rp[1:])
    return rp, col[keep], val[keep]


def upwind_chain(n, pe):
    """tridiag(-1 - pe, 2 + pe, -1) as (row_ptr, col, val)."""
    i = np.arange(n)
    rows = np.concatenate([i[1:], i, i[:-1]])
    cols = np.concatenate([i[:-1], i, i[1:]])
    vals = np.concatenate([np.full(n - 1, -1.0 - pe), np.full(n, 2.0 + pe), np.full(n - 1, -1.0)])
    return _csr(n, rows, cols, vals)


def oracle_matrix(O, csr):
    rp, col, val = csr
    return O.Csr.from_arrays(rp.size - 1, rp.size - 1, rp, col, val)


def rhs(O, n):
    return O.vec_uniform(n, 7)


def ragged_cuts(n, nranks):
    """Rank starts and the end: [0, n//3, 2n//3 + 5, n] on three ranks, [0, n//3, n] on two."""
    return {1: [0, n], 2: [0, n // 3, n], 3: [0, n // 3, 2 * n // 3 + 5, n]}[nranks]


def bicgstab_restated(H, A, x, b, max_iter, tol, dot, trace=None):
    """Right-preconditioned BiCGStab, M = H.cycle from zero.  Returns x, the squared residual
    norms rr_k (k = 0 .. iterations counted) and the status.  trace (a list) receives a copy of
    every x written."""
    x = np.array(x, np.float64, copy=True)
    n = x.size
    M = lambda v: H.cycle(np.zeros(n), v)  # noqa: E731
    r = A.residual(x, b)
    rhat = r.copy()
    p = r.copy()
    rr = [dot(r, r)]
    rho = rr[0]
    h0 = np.sqrt(rr[0])
    status = KRYLOV_OK
    with np.errstate(all="ignore"):
        for _ in range(max_iter):
            ph = M(p)
            v = A.spmv(ph)
            rv = dot(rhat, v)
            alpha = np.float64(rho) / np.float64(rv)
            if rv == 0.0 or not np.isfinite(alpha):
                status = KRYLOV_BREAKDOWN
                break
            s = r - alpha * v
            sh = M(s)
            t = A.spmv(sh)
            ts, tt = dot(t, s), dot(t, t)
            omega = np.float64(ts) / np.float64(tt)
            if tt == 0.0 or not np.isfinite(omega):
                omega = np.float64(0.0)
            x = (x + alpha * ph) + omega * sh
            r = s - omega * t
            if trace is not None:
                trace.append(x.copy())
            rr.append(dot(r, r))
            rho_new = dot(rhat, r)
            if omega == 0.0:
                status = KRYLOV_BREAKDOWN
                break
            if tol > 0.0 and h0 > 0.0 and np.sqrt(rr[-1]) / h0 < tol:
                break
            beta = (np.float64(rho_new) / np.float64(rho)) * (alpha / omega)
            if rho_new == 0.0 or not np.isfinite(beta):
                status = KRYLOV_BREAKDOWN
                break
            p = r + beta * (p - omega * v)
            rho = rho_new
    return x, np.array(rr), status
