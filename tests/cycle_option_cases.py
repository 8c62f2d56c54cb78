"""Case tables and numpy restatements for the solve layer's tests (Solver::cycle_rec, solve,
pcg, dot in raptor_amd/csrc/multilevel.hip): tests/test_cycle_options_cpu.py checks them on the
CPU, tests/test_gpu_cycle_options.py runs the product against them.

dot_tree restates the product's dot product (dot_partials_kernel + block_sum_span +
finish_sum_kernel in kernels.hip) operation for operation, so a PCG run that uses it has the
product's alpha and beta bit for bit; pcg_restated is the oracle's orc_hier_pcg loop with the
dot left open.  numpy only."""
import numpy as np

# ---- the dot product of kernels.hip, restated ------------------------------------------------
K_TPB = 256              # kTPB: threads per block
DOT_SPAN = K_TPB * 8     # kDotSpan: entries one dot_partials_kernel block covers
RED_SPAN = K_TPB * 16    # kRedSpan: partials one block_sum_span block covers


def _block_tree(lane):
    """lane: (G, 256) per-lane sums -> (G,) block values.  Per 64-lane wave the shuffle tree
    s[t] += s[t + off], off = 32 .. 1 (only lane 0 is read), then (w0 + w1) + (w2 + w3)."""
    w = lane.reshape(-1, 4, 64)
    for off in (32, 16, 8, 4, 2, 1):
        w = w[:, :, :off] + w[:, :, off:2 * off]
    w = w[:, :, 0]
    return (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])


def _strided_blocks(v, loads):
    """v: values; block g holds [span g, span (g + 1)) with span = 256 loads; lane t sums its
    entries t, t + 256, ... in order from 0.0.  A lane's sum starts at +0.0 and so never is
    -0.0: adding +0.0 for an entry past the end equals skipping it."""
    span = K_TPB * loads
    g = max(1, -(-v.size // span))
    p = np.zeros(g * span)
    p[:v.size] = v
    p = p.reshape(g, loads, K_TPB)
    lane = np.zeros((g, K_TPB))
    for j in range(loads):
        lane = lane + p[:, j, :]
    return _block_tree(lane)


def _dot_local(a, b):
    """One rank's launch_dot_partials + launch_reduce_partials."""
    part = _strided_blocks(a * b, 8)        # each product rounded (-ffp-contract=off)
    while True:
        part = _strided_blocks(part, 16)    # recurses while more than 4096 partials are left
        if part.size == 1:
            return part[0]


def dot_tree(a, b, cuts=None):
    """The product's dot(a, b).  cuts: the ranks' first rows and the end ([0, ..., n]); each
    rank reduces its own slice, finish_sum_kernel adds the rank values in rank order from 0.0."""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    cuts = [0, a.size] if cuts is None else list(cuts)
    s = np.float64(0.0)
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        s = s + _dot_local(a[lo:hi], b[lo:hi])
    return s


def dot_seq(a, b):
    """The oracle's dotp: products summed front to back."""
    a = np.asarray(a, np.float64)
    if a.size == 0:
        return np.float64(0.0)
    return np.add.accumulate(a * np.asarray(b, np.float64))[-1]


def pcg_restated(H, A, x, b, max_iter, tol, dot):
    """orc_hier_pcg with H.cycle, A's oracle kernels and `dot`.  Returns x and the squared
    residual norms rr_k (before any sqrt), k = 0 .. iterations."""
    x = np.array(x, np.float64, copy=True)
    n = x.size
    r = A.residual(x, b)
    rr = [dot(r, r)]
    r0 = np.sqrt(rr[0])
    z = H.cycle(np.zeros(n), r)
    p = z.copy()
    rz = dot(r, z)
    it = 0
    while it < max_iter:
        q = A.spmv(p)
        alpha = rz / dot(p, q)
        x = x + alpha * p
        r = r - alpha * q
        rr.append(dot(r, r))
        it += 1
        if tol > 0.0 and r0 > 0.0 and np.sqrt(rr[-1]) / r0 < tol:
            break
        if it == max_iter:
            break
        z = H.cycle(np.zeros(n), r)
        rzn = dot(r, z)
        beta = rzn / rz
        p = z + beta * p
        rz = rzn
    return x, np.array(rr)


# ---- the option matrix ---------------------------------------------------------------------
PROBLEMS = {"7pt": (16, 15, 14), "27pt": (12, 11, 10)}
MAX_COARSE = 32          # at least 4 levels on both problems (asserted where it is used)
SWEEPS = [(0, 0), (0, 1), (1, 0), (2, 1), (1, 2), (2, 2), (3, 0)]
OMEGAS = [2.0 / 3.0, 1.0, 0.5]
GS_BLOCKS = [1, 8, 64]
FAMILIES = {"jacobi": ("pmis", "jacobi"), "gs": ("sa", "hybrid_gs")}
# tpl: no size floor for row templates (coarse levels take them too); split: hybrid-GS sweeps
# split on every level (level 0's GS templates, which keep its sweeps whole, are turned off)
ENVS = {"built": {}, "tpl": {"AMG_TPL_MIN_ROWS": "0"},
        "split": {"AMG_GS_SPLIT_NPR": "0", "AMG_GS_TEMPLATES": "0"}}


def _rotated(values, width):
    """Per (pre, post): `width` consecutive values of the other option, starting one further
    along each time -- every value meets several (pre, post) and the other way round."""
    return [(pre, post, values[(i + k) % len(values)])
            for i, (pre, post) in enumerate(SWEEPS) for k in range(width)]


# (family, pre, post, jacobi_omega, gs_block): two omegas / blocks per (pre, post)
OPTION_CASES = ([("jacobi", pre, post, w, 64) for pre, post, w in _rotated(OMEGAS, 2)] +
                [("gs", pre, post, 2.0 / 3.0, B) for pre, post, B in _rotated(GS_BLOCKS, 2)])


def gpu_matrix():
    """(kind, env, family, pre, post, omega, gs_block): the whole option table as built, one
    omega / block per (pre, post) -- another rotation -- in the other builds."""
    one = ([("jacobi", pre, post, w, 64) for pre, post, w in _rotated(OMEGAS[::-1], 1)] +
           [("gs", pre, post, 2.0 / 3.0, B) for pre, post, B in _rotated(GS_BLOCKS[::-1], 1)])
    out = []
    for kind in PROBLEMS:
        out += [(kind, "built") + c for c in OPTION_CASES]
        out += [(kind, "tpl") + c for c in one]
        out += [(kind, "split") + c for c in one if c[0] == "gs"]
    return out


def case_id(c):
    *head, fam, pre, post, w, B = c
    opt = f"w{w:.2f}" if fam == "jacobi" else f"B{B}"
    return "-".join([*head, fam, f"{pre}{post}", opt])


def oracle_options(O, fam, pre=1, post=1, omega=2.0 / 3.0, gs_block=64, max_coarse=MAX_COARSE):
    coarsen = FAMILIES[fam][0]
    return dict(O.DEFAULTS[coarsen], pre_sweeps=pre, post_sweeps=post, jacobi_omega=omega,
                gs_block=gs_block, max_coarse=max_coarse)


def product_options(fam, pre=1, post=1, omega=2.0 / 3.0, gs_block=64, max_coarse=MAX_COARSE):
    coarsen, smoother = FAMILIES[fam]
    return dict(coarsen=coarsen, smoother=smoother, pre_sweeps=pre, post_sweeps=post,
                jacobi_omega=omega, gs_block=gs_block, max_coarse=max_coarse)


def problem(O, kind):
    """(oracle matrix, b = A * vec_uniform) of a section-3 problem."""
    Ao = {"7pt": O.gen_7pt, "27pt": O.gen_27pt}[kind](*PROBLEMS[kind])
    return Ao, Ao.spmv(O.vec_uniform(Ao.shape[0], 42))


# ---- stopping rules (7-pt problem, default options, one solver per family) -------------------
# test_cycle_options_cpu.py checks that the oracle stops strictly inside (0, max_iter) and that
# no hist[k] / hist[0] lies within 1 % of the tolerance: the stop index is then the same for any
# history that agrees with the oracle's to a few digits.
STOP = {
    ("jacobi", "solve"): dict(tol=1e-4, max_iter=40),
    ("gs", "solve"): dict(tol=1e-6, max_iter=40),
    ("jacobi", "pcg"): dict(tol=1e-8, max_iter=40),
    ("gs", "pcg"): dict(tol=1e-10, max_iter=40),
}

# ---- PCG on the 1-D chain --------------------------------------------------------------------
CHAIN_SIZES = [255, 2047, 2048, 2049, 4097]   # the dot span's edges; 4097: two spans + 1
CHAIN_MAX_COARSE = 16
CHAIN_CUTS = [0, 2049, 2050, 4097]            # three ranks: one span + 1 | one row | 2047


def chain_csr(n):
    """tridiag(-1, 2.5, -1) as (row_ptr, col, val), columns ascending."""
    i = np.arange(n)
    rows = np.concatenate([i[1:], i, i[:-1]])
    cols = np.concatenate([i[1:] - 1, i, i[:-1] + 1])
    vals = np.concatenate([-np.ones(n - 1), 2.5 * np.ones(n), -np.ones(n - 1)])
    order = np.lexsort((cols, rows))
    rp = np.zeros(n + 1, np.int64)
    np.add.at(rp, rows + 1, 1)
    return np.cumsum(rp), cols[order].astype(np.int64), vals[order]


def chain_problem(O, n):
    rp, col, val = chain_csr(n)
    Ao = O.Csr.from_arrays(n, n, rp, col, val)
    return Ao, Ao.spmv(O.vec_uniform(n, 42)), (rp, col, val)
