"""The restatements and case tables of tests/cycle_option_cases.py, checked on the CPU: the
dot tree against exact integers, the restated PCG loop against the oracle's, and the oracle's
own handling of every cycle option the GPU tests compare the product with.  No GPU needed."""
import numpy as np
import pytest

from tests import cycle_option_cases as K


@pytest.mark.parametrize("n", [1, 255, 256, 2047, 2048, 2049, 4097])
def test_dot_tree_exact_on_integers(n):
    """Integer-valued vectors with every partial sum far below 2^53: any summation order is
    exact, so the tree must give the Python-integer dot -- on one rank and over rank slices."""
    rng = np.random.default_rng(n)
    a = rng.integers(-1000, 1001, n)
    b = rng.integers(-1000, 1001, n)
    want = sum(int(u) * int(v) for u, v in zip(a, b))
    assert abs(want) < 2 ** 53 and int(np.abs(a * b).sum()) < 2 ** 53
    got = K.dot_tree(a.astype(np.float64), b.astype(np.float64))
    assert got == want and float(got).is_integer()
    cuts = sorted({0, n // 3, n // 3 + 1 if n > 1 else 0, n})
    assert K.dot_tree(a.astype(np.float64), b.astype(np.float64), cuts) == want
    assert K.dot_seq(a.astype(np.float64), b.astype(np.float64)) == want


def test_dot_tree_skips_nothing_and_counts_once():
    """Every position is summed exactly once: a single 1.0 moved through the vector."""
    n = 4097
    ones = np.ones(n)
    for i in (0, 63, 64, 255, 256, 2047, 2048, 4095, 4096):
        e = np.zeros(n)
        e[i] = 3.0
        assert K.dot_tree(e, ones) == 3.0
    assert K.dot_tree(ones, ones) == n
    assert K.dot_tree(np.zeros(0), np.zeros(0)) == 0.0


def test_dot_tree_is_not_the_sequential_sum():
    """Liveness: a = [2^53, 1, 1, ..., 1] (n = 2049), b = 1.  Front to back every 1 is absorbed
    by 2^53 (ties to even): 2^53.  In the tree only lane 0 of block 0 holds 2^53; the 1s of the
    other lanes first add up among themselves and arrive as exact multiples of 2 or more."""
    n = 2049
    a = np.ones(n)
    a[0] = 2.0 ** 53
    b = np.ones(n)
    seq = K.dot_seq(a, b)
    tree = K.dot_tree(a, b)
    assert seq == 2.0 ** 53
    assert tree != seq
    assert tree.tobytes() != seq.tobytes()
    # lane 0 of block 0: 2^53 + 7 ones in turn (all absorbed); the other 2041 ones are exact
    assert tree == 2.0 ** 53 + 2040  # 2041 rounds to even at this magnitude's spacing of 2


@pytest.mark.parametrize("fam", ["jacobi", "gs"])
def test_pcg_restated_is_the_oracles_loop(oracle, fam):
    """With the sequential dot the restated loop is orc_hier_pcg bit for bit (x and every
    history entry), with and without a tolerance: only the dot differs on the GPU side."""
    O = oracle
    Ao, b = K.problem(O, "7pt")
    H = O.Hierarchy(Ao, **K.oracle_options(O, fam))
    n = Ao.shape[0]
    for tol in (0.0, K.STOP[(fam, "pcg")]["tol"]):
        xo, ho = H.pcg(np.zeros(n), b, max_iter=12, tol=tol)
        x, rr = K.pcg_restated(H, Ao, np.zeros(n), b, 12, tol, K.dot_seq)
        assert np.array_equal(x, xo)
        assert np.array_equal(np.sqrt(rr), ho)
    # and the dot does matter: the tree's history is not the sequential one's
    _, rr_t = K.pcg_restated(H, Ao, np.zeros(n), b, 12, 0.0, K.dot_tree)
    assert not np.array_equal(rr_t, rr)
    assert np.allclose(np.sqrt(rr_t), np.sqrt(rr), rtol=1e-6, atol=0)


@pytest.fixture(scope="module")
def default_cycles(oracle):
    out = {}
    for kind in K.PROBLEMS:
        Ao, b = K.problem(oracle, kind)
        for fam in K.FAMILIES:
            H = oracle.Hierarchy(Ao, **K.oracle_options(oracle, fam))
            out[kind, fam] = H.cycle(np.zeros(b.size), b)
    return out


@pytest.mark.parametrize("kind", list(K.PROBLEMS))
def test_oracle_honours_every_option(oracle, default_cycles, kind):
    """Every option tuple of the GPU matrix changes the oracle's cycle (an option the oracle
    ignored would make the GPU comparison vacuous): against the default options, and -- where
    anything is smoothed at all -- between the omegas / GS blocks of one (pre, post)."""
    O = oracle
    Ao, b = K.problem(O, kind)
    n = b.size
    seen = {}
    for fam, pre, post, w, B in K.OPTION_CASES:
        H = O.Hierarchy(Ao, **K.oracle_options(O, fam, pre, post, w, B))
        assert H.num_levels >= 4
        x = H.cycle(np.zeros(n), b)
        assert np.all(np.isfinite(x))
        assert not np.array_equal(x, default_cycles[kind, fam]), (fam, pre, post, w, B)
        for (w2, B2), x2 in seen.setdefault((fam, pre, post), {}).items():
            if pre + post > 0:
                assert not np.array_equal(x, x2), (fam, pre, post, (w, B), (w2, B2))
            else:  # nothing smoothed: omega and the block size cannot matter
                assert np.array_equal(x, x2)
        seen[fam, pre, post][w, B] = x
    # the tables: every value of each option with at least two values of the others
    for fam, idx, vals in (("jacobi", 3, K.OMEGAS), ("gs", 4, K.GS_BLOCKS)):
        cs = [c for c in K.OPTION_CASES if c[0] == fam]
        assert {c[1:3] for c in cs} == set(K.SWEEPS)
        for v in vals:
            assert len({c[1:3] for c in cs if c[idx] == v}) >= 2
        for s in K.SWEEPS:
            assert len({c[idx] for c in cs if c[1:3] == s}) >= 2
    assert len(K.gpu_matrix()) == len(set(K.gpu_matrix())) <= 100


@pytest.mark.parametrize("fam,what", list(K.STOP))
def test_stop_index_is_well_defined(oracle, fam, what):
    """The stopping tests' tolerances: the oracle stops strictly inside (0, max_iter), and every
    hist[k] / hist[0] stays at least 1 % (relative) away from tol, so a history that agrees with
    the oracle's to far better than that stops at the same k.  For pcg both the oracle's loop
    and the restated loop on the product's dot tree are held to it."""
    O = oracle
    Ao, b = K.problem(O, "7pt")
    H = O.Hierarchy(Ao, **K.oracle_options(O, fam))
    n = b.size
    tol, max_iter = K.STOP[fam, what]["tol"], K.STOP[fam, what]["max_iter"]
    if what == "solve":
        hists = [H.solve(np.zeros(n), b, max_iter=max_iter, tol=tol)[1]]
    else:
        hists = [H.pcg(np.zeros(n), b, max_iter=max_iter, tol=tol)[1],
                 np.sqrt(K.pcg_restated(H, Ao, np.zeros(n), b, max_iter, tol, K.dot_tree)[1])]
        assert len(hists[0]) == len(hists[1])
    for h in hists:
        assert 2 <= len(h) - 1 < max_iter
        ratio = h / h[0]
        assert ratio[-1] < tol and np.all(ratio[:-1] >= tol)
        assert np.all(np.abs(ratio - tol) >= 0.01 * tol), ratio


def test_chain_problem_and_cuts(oracle):
    """The 1-D chain of the PCG tests: diagonal 2.5, off-diagonals -1, sorted columns; its
    hierarchies have several levels for both families at every size used."""
    O = oracle
    rp, col, val = K.chain_csr(5)
    assert rp.tolist() == [0, 2, 5, 8, 11, 13]
    assert col.tolist() == [0, 1, 0, 1, 2, 1, 2, 3, 2, 3, 4, 3, 4]
    assert val[:5].tolist() == [2.5, -1.0, -1.0, 2.5, -1.0]
    assert K.CHAIN_CUTS[0] == 0 and K.CHAIN_CUTS[-1] == 4097
    for n in (K.CHAIN_SIZES[0], K.CHAIN_SIZES[-1]):
        Ao, b, _ = K.chain_problem(O, n)
        for fam in K.FAMILIES:
            H = O.Hierarchy(Ao, **K.oracle_options(O, fam, max_coarse=K.CHAIN_MAX_COARSE))
            assert H.num_levels >= 3
            _, h = H.pcg(np.zeros(n), b, max_iter=10)
            assert np.all(np.isfinite(h)) and np.all(h > 0) and h[-1] < h[0]


@pytest.mark.parametrize("field", ["pre_sweeps", "post_sweeps"])
def test_host_setup_refuses_negative_sweeps(oracle, field):
    """build_hierarchy checks the sweep counts beside max_levels (they were taken as 0)."""
    import raptor_amd as ra
    from raptor_amd import host

    Ao = oracle.gen_5pt(12, 11)
    rp, col, val = Ao.arrays()
    with pytest.raises(ra.AmgError, match="sweeps"):
        host.HostHierarchy(Ao.shape[0], 0, rp, col, val, host.options(**{field: -1}))
    with pytest.raises(ra.AmgError, match="max_levels"):
        host.HostHierarchy(Ao.shape[0], 0, rp, col, val, host.options(max_levels=0))
    assert host.HostHierarchy(Ao.shape[0], 0, rp, col, val, host.options(**{field: 0})).num_levels >= 1
