"""CPU side of the setup edge cases (tests/setup_edge_cases.py): every builder's claims, checked
with the oracle's stage functions; the oracle against the independent numpy restatement of
tests/golden/gen_golden.py, stage by stage and bit for bit, on these non-M-matrix operators;
the product's host setup against the oracle; the SpGEMM reference; and liveness -- each edge is
one that a subtly wrong kernel would trip on, shown with perturbed copies of the restatement.

Comparisons are on bit patterns (setup_edge_cases.same_bits) unless stated."""
import importlib.util
import os

import numpy as np
import pytest
import scipy.sparse as sp

from tests import setup_edge_cases as E
from tests.setup_edge_cases import bits, same_bits

SEED = 0x5EED
RESTATE_MAX = 2000  # rows up to which the Python-loop restatement runs every stage


def _load_restatement():
    path = os.path.join(E.GOLDEN, "gen_golden.py")
    spec = importlib.util.spec_from_file_location("_gen_golden_restatement", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


G = _load_restatement()


def _orc(O, M):
    M = sp.csr_matrix(M)
    return O.Csr.from_arrays(M.shape[0], M.shape[1], M.indptr, M.indices, M.data)


_STAGE = {}


def stage0(O, name):
    """Level-0 oracle stages of a case, computed once: S, split, arms (PMIS)."""
    if name not in _STAGE:
        c = E.zoo()[name]
        Ao = _orc(O, c.A)
        out = dict(Ao=Ao)
        if c.pmis:
            S = O.strength_classical(Ao, c.pmis["strong_threshold"])
            cf = O.pmis_split(S, SEED)
            out.update(S=S, cf=cf, P=O.interp_classical(Ao, S, cf), arms=E.interp_arms(c.A, S.to_scipy(), cf))
        _STAGE[name] = out
    return _STAGE[name]


def oracle_hierarchy(O, name, kind, **kw):
    c = E.zoo()[name]
    opts = dict(getattr(c, kind), **kw)
    return O.Hierarchy(_orc(O, c.A), coarsen=O.COARSEN_PMIS if kind == "pmis" else O.COARSEN_SA,
                       smoother=O.SMOOTH_JACOBI if kind == "pmis" else O.SMOOTH_HYBRID_GS, **opts)


# ---- 1. the builders' claims --------------------------------------------------------------------
@pytest.mark.parametrize("name", E.names())
def test_operator_is_well_formed(oracle, name):
    """Square, sorted, no duplicate, finite; strictly diagonally dominant outside the rows the
    case names; every listed hierarchy is finite down to the dense coarse inverse and has the
    level count its case states (one level for n <= max_coarse, else at least two)."""
    O = oracle
    c = E.zoo()[name]
    A = c.A
    n = A.shape[0]
    assert A.shape == (n, n) and A.has_sorted_indices and np.isfinite(A.data).all()
    for i in range(n):
        assert np.all(np.diff(A.indices[A.indptr[i]:A.indptr[i + 1]]) > 0)
    dom = E.dominance(A)
    keep = np.ones(n, bool)
    keep[list(c.undominated)] = False
    assert dom[keep].min() > 0.0
    assert n <= 3000
    for kind in ("pmis", "sa"):
        if getattr(c, kind) is None:
            continue
        H = oracle_hierarchy(O, name, kind)
        assert (H.num_levels == 1) if c.one_level else (H.num_levels >= 2), (kind, H.num_levels)
        for l in range(H.num_levels):
            assert np.isfinite(H.matrix(l, "A").data).all()
            if l + 1 < H.num_levels:
                assert np.isfinite(H.matrix(l, "P").data).all()
        assert np.isfinite(O.dense_inverse(_orc(O, H.matrix(H.num_levels - 1, "A")))).all()


def test_mixed_recipe_is_the_fixtures(oracle):
    """mixed_graph restates the recipe of the stored mixed_600 operator: the same bits."""
    assert same_bits(E.mixed_graph(600, 2, 11), E.zoo()["mixed_600"].A)


@pytest.mark.parametrize("name", ["mixed_600", "mixed_2500"])
def test_claims_mixed(oracle, name):
    c = E.zoo()[name]
    A = c.A
    off = A.data[A.indices != np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))]
    assert (off > 0).mean() >= c.claims["positive_fraction_min"]
    arms = stage0(oracle, name)["arms"]
    # the sign selection leaves entries of strong F neighbours' rows inside C_i out; both arms
    # of s_k occur, and some row takes both
    assert arms["dropped_sign"].sum() >= 1
    assert arms["sk_zero"].sum() > 0 and arms["sk_nonzero"].sum() > 0
    assert ((arms["sk_zero"] > 0) & (arms["sk_nonzero"] > 0)).any()
    if c.claims.get("wave_default"):
        assert A.nnz >= E.WAVE_NPR * A.shape[0]
    # SA: positive couplings are never strong, weak entries exist (lumped into f_i)
    Ao = stage0(oracle, name)["Ao"]
    S = oracle.strength_symmetric(Ao, 0.08).to_scipy()
    assert S.data.max() < 0.0 and S.nnz < A.nnz - A.shape[0]
    F = oracle.sa_filter(Ao, 0.08).to_scipy()
    assert not np.array_equal(F.diagonal(), A.diagonal())


def test_claims_positive_rows(oracle):
    O = oracle
    c = E.zoo()["positive_rows"]
    st = stage0(O, "positive_rows")
    S, cf, P = st["S"].to_scipy(), st["cf"], st["P"].to_scipy()
    ST = sp.csr_matrix(S.T)
    dep, nodep = c.claims["with_dependents"], c.claims["without_dependents"]
    assert dep.size >= 20 and nodep.size >= 20
    for i in np.concatenate([dep, nodep]):
        off = c.A[i].data[c.A[i].indices != i]
        assert off.size and off.min() > 0.0  # mx <= 0
    assert np.all(np.diff(S.indptr)[dep] == 0) and np.all(np.diff(S.indptr)[nodep] == 0)
    assert np.all(np.diff(ST.indptr)[dep] > 0) and np.all(np.diff(ST.indptr)[nodep] == 0)
    assert np.all(cf[dep] == 1) and np.all(cf[nodep] != 1)
    assert np.all(np.diff(P.indptr)[nodep] == 0)  # nci == 0: empty P rows
    assert np.all(st["arms"]["nci"][nodep] == 0)
    # SA: the rows of the second kind are singleton aggregates
    Ss = O.strength_symmetric(st["Ao"], 0.08)
    agg, na = O.mis2_aggregate(Ss, SEED)
    size = np.bincount(agg, minlength=na)
    assert np.all(size[agg[nodep]] == 1)


def test_claims_negative_diagonal(oracle):
    c = E.zoo()["negative_diagonal"]
    d = c.A.diagonal()
    assert np.all(d[c.claims["negated"]] < 0) and (d > 0).sum() == c.A.shape[0] - c.claims["negated"].size
    both = []
    for k in c.claims["negated"]:
        v = c.A[k].data[c.A[k].indices != k]
        both.append(v.min() < 0.0 < v.max())
    assert np.mean(both) >= 0.5  # both signs of off-diagonal in most of the negated rows
    arms = stage0(oracle, "negative_diagonal")["arms"]
    # pos == false taken, and with positive entries inside C_i actually selected
    assert arms["neg"].sum() >= c.claims["neg_arm_min"]
    assert arms["neg_selected"].sum() >= c.claims["neg_arm_min"]
    assert arms["dropped_sign"].sum() > 0


def test_claims_no_diagonal_neighbour(oracle):
    c = E.zoo()["no_diagonal_neighbour"]
    rows = c.claims["no_diagonal"]
    for k in rows:
        assert k not in c.A.indices[c.A.indptr[k]:c.A.indptr[k + 1]]
    st = stage0(oracle, "no_diagonal_neighbour")
    cf, S, A = st["cf"], st["S"].to_scipy(), c.A
    # rows without a diagonal that are strong F neighbours of an F row with C neighbours
    hits = 0
    for i in np.flatnonzero((cf != 1) & (st["arms"]["nci"] > 0)):
        for k in S.indices[S.indptr[i]:S.indptr[i + 1]]:
            hits += cf[k] != 1 and k in rows
    assert hits >= c.claims["zero_diag_arm_min"]
    assert st["arms"]["neg"].sum() == hits  # every diagonal that is stored is positive


def test_claims_sk_zero(oracle):
    c = E.zoo()["sk_zero"]
    st = stage0(oracle, "sk_zero")
    arms, cf = st["arms"], st["cf"]
    ri = c.claims["rows_i"]
    assert ri.size == 200 and np.all(cf[ri] != 1)
    assert np.all(cf[ri - 2] == 1) and np.all(cf[ri - 1] == 1)          # c1, c2
    assert np.all(cf[ri + 1] != 1) and np.all(cf[ri + 2] != 1)          # k, k2
    assert np.all(arms["nci"][ri] == 1) and np.all(arms["sk_zero"][ri] == 1) and np.all(arms["sk_nonzero"][ri] == 1)
    assert arms["dropped_sign"][ri].sum() == 100  # the positive a_k,c1 of the odd tiles
    assert ((arms["sk_zero"] > 0) & (arms["sk_nonzero"] > 0)).sum() >= c.claims["both_arms_min"]


def test_claims_hub(oracle):
    O = oracle
    c = E.zoo()["hub"]
    st = stage0(O, "hub")
    arms, cf, A = st["arms"], st["cf"], c.A
    hubs, lengths = c.claims["hubs"], c.claims["lengths"]
    assert np.array_equal(np.diff(A.indptr)[hubs], lengths)
    assert np.all(cf[hubs] != 1)
    S = st["S"].to_scipy()
    assert np.array_equal(np.diff(S.indptr)[hubs], lengths - 1)            # every coupling strong
    assert np.all(np.diff(sp.csr_matrix(S.T).indptr)[hubs] == 0)           # nothing depends on a hub
    assert np.array_equal(arms["nci"][hubs] + arms["nsf"][hubs], lengths - 1)
    long = lengths - 1 >= 192
    assert long.sum() == 4
    assert np.all(arms["nci"][hubs][long] > 64) and np.all(arms["nsf"][hubs][long] > 64)
    assert np.all(arms["nci"][hubs] > 0) and np.all(arms["nsf"][hubs] > 0)
    assert (lengths > E.K_IW_MAX).sum() == 2 and (lengths == E.K_IW_MAX).sum() == 1
    # the chunk loops: rows of more than 64 entries whose s_k take both values
    assert (arms["sk_nonzero"][hubs] > 64).any()
    # Galerkin bounds: ub = sum_k |B_k| of A P and of R (A P) pass 128 and 1024
    P = st["P"].to_scipy()
    R = sp.csr_matrix(P.T)
    plen = np.diff(P.indptr)
    ub_ap = np.array([plen[A.indices[A.indptr[i]:A.indptr[i + 1]]].sum() for i in range(A.shape[0])])
    AP = (st["Ao"] @ st["P"]).to_scipy()
    aplen = np.diff(AP.indptr)
    ub_rap = np.array([aplen[R.indices[R.indptr[i]:R.indptr[i + 1]]].sum() for i in range(R.shape[0])])
    for ub in (ub_ap, ub_rap):
        assert ((ub > 128) & (ub <= 1024)).any() and (ub > 1024).any(), ub.max()
    # and distinct counts on both sides of the numeric 128 boundary
    assert aplen.max() > 128 and (np.diff((st["P"].transpose() @ (st["Ao"] @ st["P"])).to_scipy().indptr) > 128).any()


def test_claims_ties(oracle):
    O = oracle
    c = E.zoo()["ties_classical"]
    S = stage0(O, "ties_classical")["S"].to_scipy()
    n = c.A.shape[0]
    i = n // 2
    strong = set(S.indices[S.indptr[i]:S.indptr[i + 1]] - i)
    assert strong == {s * o for o in c.claims["strong_offsets"] for s in (1, -1)}
    assert 0.25 * 4.0 == 1.0 and c.A[i, i + 2] == -1.0 and -c.A[i, i + 3] < 1.0 < -c.A[i, i + 4]
    assert np.nextafter(1.0, 2.0) == -c.A[i, i + 4] and np.nextafter(1.0, 0.0) > -c.A[i, i + 3] >= 1.0 - 2 ** -52
    c = E.zoo()["ties_sa"]
    Ss = O.strength_symmetric(_orc(O, c.A), 0.25).to_scipy()
    e, want = c.claims["edge_values"], c.claims["strong_edges"]
    assert set(np.unique(-e)) == {1.0, 2.0, np.nextafter(2.0, 0.0), np.nextafter(2.0, 4.0)}
    assert 0.25 * np.sqrt(abs(16.0 * 4.0)) == 2.0
    got_up = np.array([Ss[t, t + 1] != 0 for t in range(n - 1)])
    got_dn = np.array([Ss[t + 1, t] != 0 for t in range(n - 1)])
    assert np.array_equal(got_up, want) and np.array_equal(got_dn, want)
    assert np.array_equal(want, -e >= 2.0)
    # the weak entries are lumped into f_i
    F = O.sa_filter(_orc(O, c.A), 0.25).to_scipy()
    assert F.nnz == n + 2 * int(want.sum()) and not np.array_equal(F.diagonal(), c.A.diagonal())


def test_claims_sizes_avg12_path(oracle):
    O = oracle
    assert [E.zoo()[f"sizes_{n}"].A.shape[0] for n in E.SIZES] == list(E.SIZES)
    assert {n % E.K_T for n in E.SIZES} >= {255, 0, 1, 2} and any(n % E.K_IW_WAVES for n in E.SIZES)
    for n in E.SIZES:
        A = E.zoo()[f"sizes_{n}"].A
        off = A.data[A.indices != np.repeat(np.arange(n), np.diff(A.indptr))]
        assert n < 100 or (off.min() < 0.0 < off.max())
    at, below = E.zoo()["avg12_at"].A, E.zoo()["avg12_below"].A
    assert at.nnz == 12 * at.shape[0] and below.nnz == 12 * below.shape[0] - 1
    assert at.nnz >= E.WAVE_NPR * at.shape[0] > below.nnz
    # the chain: along a stretch of falling keys a round decides two (PMIS) or three (MIS(2))
    # points.  Rounds counted with the restatement's loops on the oracle's strength.
    c = E.zoo()["path"]
    n = c.A.shape[0]
    assert np.array_equal(E.hash32(np.arange(n), SEED), G.hash32(np.arange(n), SEED))
    order = c.claims["order"]
    assert np.array_equal(np.sort(order), np.arange(n))
    h = G.hash32(order, SEED).astype(np.int64)
    falls = np.diff(h) < 0
    assert all(falls[q:q + E.PATH_RUN - 1].all() for q in range(0, n, E.PATH_RUN))
    S = stage0(O, "path")["S"]
    rp, col, _ = S.arrays()
    lists = [col[rp[i]:rp[i + 1]].tolist() for i in range(n)]
    assert sum(len(r) == 2 for r in lists) == n - 2 and len(lists[order[0]]) == len(lists[order[-1]]) == 1
    assert _pmis_rounds(lists, SEED) >= c.claims["pmis_rounds_min"] == 100
    Sv = G.strength_symmetric(c.A, c.sa["strong_threshold"])
    assert [[j for j, _ in r] for r in Sv] == lists
    assert _mis2_rounds(lists, SEED) >= c.claims["mis2_rounds_min"] == 66


def _mis2_rounds(S, seed):
    """The round loop of gen_golden.mis2_aggregate, counting."""
    n = len(S)
    h = [int(v) for v in G.hash32(np.arange(n), seed)]
    st = [1] * n  # 0 out, 1 undecided, 2 in
    rounds = 0
    while 1 in st:
        rounds += 1
        t = [(st[i], h[i], i) for i in range(n)]
        for _ in range(2):
            t = [max([t[i]] + [t[j] for j in S[i]]) for i in range(n)]
        for i in range(n):
            if st[i] == 1:
                if t[i][2] == i:
                    st[i] = 2
                elif t[i][0] == 2:
                    st[i] = 0
    return rounds


def _pmis_rounds(S, seed):
    n = len(S)
    ST = G.transpose_lists(S, n)
    h = G.hash32(np.arange(n), seed)
    key = [(len(ST[i]) << 32) | int(h[i]) for i in range(n)]
    cf = [0 if not ST[i] else -1 for i in range(n)]
    rounds = 0
    while any(v == -1 for v in cf):
        rounds += 1
        newc = [i for i in range(n) if cf[i] == -1
                and all(not (cf[j] == -1 and (key[j], j) > (key[i], i)) for j in S[i] + ST[i])]
        for i in newc:
            cf[i] = 1
        for i in range(n):
            if cf[i] == -1 and any(cf[j] == 1 for j in S[i]):
                cf[i] = 0
    return rounds


@pytest.mark.parametrize("name", [k for k, c in E.zoo().items() if c.cuts])
def test_claims_cuts_make_ghost_strong_f_neighbours(oracle, name):
    """Every cut of every partition of a case has, on one of its two sides, an F row whose
    strong F neighbour lies on another rank (a ghost row of A in the interpolation), and every
    partition has strong C neighbours in a halo."""
    c = E.zoo()[name]
    st = stage0(oracle, name)
    S, cf = st["S"].to_scipy(), st["cf"]
    n = c.A.shape[0]
    for nr, cuts in c.cuts.items():
        assert len(cuts) == nr and cuts[0] == 0 and np.all(np.diff(cuts + [n]) > 0)
        halo_c, ghosts = 0, []
        for r in range(nr):
            lo, hi = cuts[r], (cuts + [n])[r + 1]
            ghosts.append(int(E.interp_arms(c.A, S, cf, lo, hi)["ghost_sf"][lo:hi].sum()))
            for i in range(lo, hi):
                if cf[i] != 1:
                    js = S.indices[S.indptr[i]:S.indptr[i + 1]]
                    halo_c += int(((cf[js] == 1) & ((js < lo) | (js >= hi))).sum())
        assert halo_c >= 1, nr
        assert all(ghosts[r - 1] + ghosts[r] >= 1 for r in range(1, nr)), (nr, ghosts)


# ---- 2. the oracle against the numpy restatement ----------------------------------------------------
def _strength_lists(Scsr):
    rp, col, val = Scsr.arrays()
    return [col[rp[i]:rp[i + 1]].tolist() for i in range(rp.size - 1)], \
           [list(zip(col[rp[i]:rp[i + 1]].tolist(), val[rp[i]:rp[i + 1]].tolist())) for i in range(rp.size - 1)]


@pytest.mark.parametrize("name", E.names("pmis"))
def test_oracle_equals_restatement_pmis(oracle, name):
    """strength_classical, pmis_split, interp_classical, transpose, R (A P) and sparsify of the
    oracle against gen_golden.py's restatements, on every level of the oracle's hierarchy (levels
    above RESTATE_MAX rows: strength and split only)."""
    O = oracle
    c = E.zoo()[name]
    H = oracle_hierarchy(O, name, "pmis")
    theta = c.pmis["strong_threshold"]
    for l in range(max(H.num_levels - 1, 1)):
        A = H.matrix(l, "A")
        Ao = _orc(O, A)
        n = A.shape[0]
        So = O.strength_classical(Ao, theta)
        Sr = G.strength_classical(A, theta)
        assert _strength_lists(So)[0] == Sr, ("S", l)
        cfo = O.pmis_split(So, SEED + l)
        assert np.array_equal(cfo, G.pmis_split(Sr, SEED + l)), ("split", l)
        if H.num_levels > 1:
            assert np.array_equal(cfo, H.split(l))
        if n > RESTATE_MAX or H.num_levels == 1:
            continue
        Po = O.interp_classical(Ao, So, cfo)
        assert same_bits(Po.to_scipy(), G.interp_classical(A, Sr, cfo)), ("P", l)
        assert same_bits(Po.to_scipy(), H.matrix(l, "P"))
        Ro = Po.transpose()
        assert same_bits(Ro.to_scipy(), _scipy_transpose(Po.to_scipy())), ("R", l)
        Aco = (Ro @ (Ao @ Po)).to_scipy()
        assert same_bits(Aco, E.canonical_product(Ro.to_scipy(), E.canonical_product(A, Po.to_scipy()))), ("RAP", l)
        assert same_bits(Aco, H.matrix(l + 1, "A"))
        for tau in (0.01, 10.0):
            assert same_bits(O.sparsify(_orc(O, Aco), tau).to_scipy(), G.sparsify(Aco, tau)), ("sparsify", l, tau)


def _scipy_transpose(M):
    T = sp.csr_matrix(sp.csr_matrix(M).T)
    T.sort_indices()
    return T


@pytest.mark.parametrize("name", E.names("sa"))
def test_oracle_equals_restatement_sa(oracle, name):
    """strength_symmetric, mis2_aggregate, sa_filter, sa_rho and sa_prolongator of the oracle
    against the restatements, level 0 (operators above RESTATE_MAX rows: strength and
    aggregates only).  The restated prolongator goes through scipy's product, which drops
    explicit zeros: both sides are compared without them."""
    O = oracle
    c = E.zoo()[name]
    A = c.A
    Ao = _orc(O, A)
    theta = c.sa["strong_threshold"]
    So = O.strength_symmetric(Ao, theta)
    Sv = G.strength_symmetric(A, theta)
    got = _strength_lists(So)[1]
    assert [[t[0] for t in r] for r in got] == [[t[0] for t in r] for r in Sv]
    assert all(bits([t[1] for t in a]).tolist() == bits([t[1] for t in b]).tolist() for a, b in zip(got, Sv))
    aggo, nao = O.mis2_aggregate(So, SEED)
    if A.shape[0] > 1:
        aggr, nar = G.mis2_aggregate(Sv, SEED)
        assert nao == nar and np.array_equal(aggo, aggr)
    if A.shape[0] > RESTATE_MAX or A.shape[0] < 2:
        return
    Fo = O.sa_filter(Ao, theta)
    assert same_bits(Fo.to_scipy(), G.sa_filter(A, theta))
    d = A.diagonal()
    rho = O.sa_rho(Fo, d, SEED)
    assert bits([rho])[0] == bits([G.sa_rho(G.sa_filter(A, theta), d, SEED)])[0]
    Po = O.sa_prolongator(Ao, aggo, nao, theta, SEED)
    assert same_bits(G.canon(Po.to_scipy()), G.canon(G.sa_prolongator(A, aggo, nao, theta, SEED)))


# ---- 3. the product's host path -----------------------------------------------------------------------
def _host_vs_oracle(O, name, kind, **kw):
    from raptor_amd import host

    c = E.zoo()[name]
    A = c.A
    opts = dict(getattr(c, kind), **kw)
    Hp = host.HostHierarchy(A.shape[0], 0, A.indptr, A.indices, A.data,
                            host.options(coarsen=kind, smoother="jacobi" if kind == "pmis" else "hybrid_gs", **opts))
    Ho = oracle_hierarchy(O, name, kind, **kw)
    assert Hp.num_levels == Ho.num_levels
    for l in range(Ho.num_levels):
        assert same_bits(Hp.to_scipy(l, "A"), Ho.matrix(l, "A")), ("A", l)
        assert np.isfinite(Ho.matrix(l, "A").data).all()
        if l + 1 < Ho.num_levels:
            for w in "PR":
                assert same_bits(Hp.to_scipy(l, w), Ho.matrix(l, w)), (w, l)
                assert np.isfinite(Ho.matrix(l, w).data).all()
            assert np.array_equal(Hp.split(l), Ho.split(l)), ("split", l)
    inv = O.dense_inverse(_orc(O, Ho.matrix(Ho.num_levels - 1, "A")))
    assert np.array_equal(bits(Hp.coarse_inverse()), bits(inv))
    return Ho, inv


@pytest.mark.parametrize("name,kind", E.setups())
def test_host_hierarchy_equals_oracle(oracle, name, kind):
    """HostHierarchy against the oracle's Hierarchy: every level's A, P, R, split and the coarse
    inverse, bit for bit; every value finite."""
    c = E.zoo()[name]
    Ho, inv = _host_vs_oracle(oracle, name, kind)
    assert (Ho.num_levels == 1) if c.one_level else (Ho.num_levels >= 2)
    assert np.isfinite(inv).all()


@pytest.mark.parametrize("name", ["mixed_600", "mixed_2500"])
def test_host_hierarchy_drop_tol_mixed(oracle, name):
    """SA with drop_tol = 0.01: entries are dropped, and level 1 is the oracle's sparsify of its
    own Galerkin product."""
    O = oracle
    Ho, inv = _host_vs_oracle(O, name, "sa", drop_tol=0.01)
    Hg = oracle_hierarchy(O, name, "sa")
    G1 = Hg.matrix(1, "A")
    assert Ho.matrix(1, "A").nnz < G1.nnz and np.isfinite(inv).all()
    assert same_bits(O.sparsify(_orc(O, G1), 0.01).to_scipy(), Ho.matrix(1, "A"))


def test_host_hierarchy_drop_tol_hub_goes_diagonal(oracle):
    """SA with drop_tol = 10 on hub: a diagonal coarse operator, after which coarsening stops."""
    Ho, inv = _host_vs_oracle(oracle, "hub", "sa", drop_tol=10.0)
    assert Ho.num_levels == 2
    A1 = Ho.matrix(1, "A")
    assert A1.nnz == A1.shape[0] and np.array_equal(A1.indices, np.arange(A1.shape[0]))
    assert np.isfinite(inv).all()


# ---- 4. the SpGEMM reference ------------------------------------------------------------------------------
_PRODUCTS = {}


def reference_product(O, name):
    """The pure-Python canonical product of a pair, computed once and shared (read-only)."""
    if name not in _PRODUCTS:
        p = E.pairs()[name]
        C = E.canonical_product(p.A, p.B)
        C.data.setflags(write=False)
        _PRODUCTS[name] = C
    return _PRODUCTS[name]


@pytest.mark.parametrize("name", list(E.pairs()))
def test_spgemm_reference_and_claims(oracle, name):
    """The oracle's @ equals the canonical-order product bit for bit (stored zeros included);
    its transpose equals scipy's; and the pair's claims hold: distinct columns and bounds per
    row, empty rows, restated hash slots, exact zeros."""
    O = oracle
    p = E.pairs()[name]
    A, B = p.A, p.B
    assert A.shape == B.shape and A.shape[0] == A.shape[1]
    C = reference_product(O, name)
    assert same_bits((_orc(O, A) @ _orc(O, B)).to_scipy(), C)
    for M in (A, B, C):
        assert same_bits(_orc(O, M).transpose().to_scipy(), _scipy_transpose(M))
    blen = np.diff(B.indptr)
    ub = np.array([blen[A.indices[A.indptr[i]:A.indptr[i + 1]]].sum() for i in range(A.shape[0])])
    clen = np.diff(C.indptr)
    if name == "row_bins":
        rows = p.claims["rows"]
        assert sorted({v[0] for v in rows.values()}) == sorted(E.ROW_BINS)
        for i, (r, u) in rows.items():
            assert clen[i] == r and ub[i] == u, i
        assert {u for r, u in rows.values() if u == 3 * r} == {3 * r for r in E.ROW_BINS}
        others = np.setdiff1d(np.arange(A.shape[0]), list(rows))
        assert np.all(clen[others] == 1) and np.all(ub[others] == 1)
        assert clen.max() == 8193 > 8192
        for i in p.claims["order_rows"]:  # canonical order: every column cancels to +0.0
            assert np.all(bits(C.data[C.indptr[i]:C.indptr[i + 1]]) == 0)
    elif name == "empty_rows":
        assert all(clen[i] == 0 for i in p.claims["empty_out"])
        assert np.diff(A.indptr)[3] == 3 and np.diff(A.indptr)[5] == 0 and clen[7] == 1
        assert (clen == 0).sum() == p.claims["n_empty"] + 3  # and the three empty B rows themselves
    elif name.startswith("nnz_"):
        assert C.nnz == 0 and (A.nnz == 0) != (B.nnz == 0)
        assert sorted(p.cuts) == [2, 3]
        for M in (A, B):  # diagonal or empty: no rank of any partition has a halo
            assert np.array_equal(M.indices, np.repeat(np.arange(M.shape[0]), np.diff(M.indptr)))
    elif name == "wrapped_probes":
        for i, (T, homed, distinct) in p.claims["homed"].items():
            cols = C.indices[C.indptr[i]:C.indptr[i + 1]]
            assert clen[i] == distinct and ub[i] == p.claims["ub"][i]
            assert sum(E.hslot(j, T) >= T - 8 for j in cols) == homed > 8  # more keys than slots left: a wrap
        assert ub[100] <= 128 < ub[101] and clen[101] <= 128          # 256 / symbolic 1024, numeric 256
        assert all(E.hslot(j, 256) >= 248 for j in C.indices[C.indptr[101]:C.indptr[101 + 1]])
        assert 128 < clen[102] <= 512 < clen[103] <= 2048             # numeric 1024 and 4096
        assert E.hslot(1, 256) == ((0x9E3779B97F4A7C15 >> 40) & 255) == 0x9E3779 & 255
    elif name == "exact_cancellation":
        for i, j in p.claims["zero_at"]:
            k = C.indptr[i] + int(np.searchsorted(C.indices[C.indptr[i]:C.indptr[i + 1]], j))
            assert C.indices[k] == j and bits(C.data[k:k + 1])[0] == 0
        assert sp.csr_matrix(A @ B).nnz <= C.nnz
    for nr, cuts in p.cuts.items():
        assert len(cuts) == nr and np.all(np.diff(cuts + [A.shape[0]]) > 0)
    if name == "row_bins":  # rank 0: no halo; the long rows of the last rank read ghost rows of B
        for nr, cuts in p.cuts.items():
            assert np.all(A[:cuts[1]].indices < cuts[1])
            lo = cuts[-1]
            for i in (1000 + 2 * E.ROW_BINS.index(8192), 1001 + 2 * E.ROW_BINS.index(8193)):
                assert i >= lo and np.all(A.indices[A.indptr[i]:A.indptr[i + 1]] < lo)


# ---- 5. liveness: a wrong kernel would trip on each edge --------------------------------------------------
def _interp_variant(A, S, cf, keep_sk_zero=True, use_sign=True, truncate=None):
    """gen_golden.interp_classical's loops with three switches: keep_sk_zero=False skips the
    s_k == 0 branch (a_ik is dropped instead of added to d); use_sign=False sums every entry of
    row k inside C_i whatever its sign; truncate=m reads only the first m entries of a row."""
    R = G.rows(A)
    n = len(R)
    diag = {i: dict(zip(*R[i])).get(i, 0.0) for i in range(n)}
    if truncate is not None:
        R = [(c[:truncate], v[:truncate]) for c, v in R]
    cidx = np.cumsum(cf == 1) - 1
    indptr, indices, data = [0], [], []
    for i in range(n):
        if cf[i] == 1:
            indices.append(int(cidx[i])); data.append(1.0); indptr.append(len(indices))
            continue
        Si = set(S[i])
        cols, vals = R[i]
        d = diag[i]
        num = {}
        for c, v in zip(cols, vals):
            if c == i:
                continue
            if c in Si and cf[c] == 1:
                num[c] = v
            elif c not in Si:
                d = d + v
        if num:
            for k, aik in zip(cols, vals):
                if k == i or k not in Si or cf[k] == 1:
                    continue
                kc, kv = R[k]
                pos = diag[k] > 0.0
                sel = [(m, v) for m, v in zip(kc, kv)
                       if m in num and (not use_sign or ((v < 0.0) if pos else (v > 0.0)))]
                sk = 0.0
                for _, v in sel:
                    sk = sk + v
                if sk == 0.0:
                    if keep_sk_zero:
                        d = d + aik
                else:
                    for m, v in sel:
                        num[m] = num[m] + (aik * v) / sk
        for c in sorted(num):
            indices.append(int(cidx[c])); data.append(-num[c] / d)
        indptr.append(len(indices))
    return sp.csr_matrix((np.array(data), np.array(indices, np.int64), np.array(indptr, np.int64)),
                         shape=(n, int((cf == 1).sum())))


def _restated_level0(O, name):
    c = E.zoo()[name]
    st = stage0(O, name)
    S = _strength_lists(st["S"])[0]
    return c.A, S, st["cf"], st["P"].to_scipy()


def test_liveness_strength_tie(oracle):
    """> instead of >= changes S on ties_classical (and the SA tie on ties_sa)."""
    c = E.zoo()["ties_classical"]
    good = G.strength_classical(c.A, 0.25)
    bad = []
    for i, (cols, vals) in enumerate(G.rows(c.A)):
        off = [-v for cc, v in zip(cols, vals) if cc != i]
        bad.append([cc for cc, v in zip(cols, vals) if cc != i and -v > 0.25 * max(off)])
    assert good == _strength_lists(stage0(oracle, "ties_classical")["S"])[0]
    assert sum(len(g) - len(b) for g, b in zip(good, bad)) >= c.A.shape[0]  # the +-2 ties, every row
    s = E.zoo()["ties_sa"]
    d = s.A.diagonal()
    n_ge = sum(-v >= 0.25 * np.sqrt(abs(d[i] * d[j])) for i, (cs, vs) in enumerate(G.rows(s.A)) for j, v in zip(cs, vs) if j != i)
    n_gt = sum(-v > 0.25 * np.sqrt(abs(d[i] * d[j])) for i, (cs, vs) in enumerate(G.rows(s.A)) for j, v in zip(cs, vs) if j != i)
    assert n_ge - n_gt >= 100


@pytest.mark.parametrize("name,switch", [("sk_zero", "keep_sk_zero"), ("mixed_600", "keep_sk_zero"),
                                         ("negative_diagonal", "use_sign"), ("mixed_600", "use_sign"),
                                         ("no_diagonal_neighbour", "use_sign"), ("sk_zero", "use_sign")])
def test_liveness_interpolation_arms(oracle, name, switch):
    """With every switch on, the variant is the restatement (and the oracle); dropping the
    s_k == 0 branch, or ignoring the sign selection, changes P."""
    A, S, cf, P = _restated_level0(oracle, name)
    assert same_bits(_interp_variant(A, S, cf), P)
    bad = _interp_variant(A, S, cf, **{switch: False})
    assert np.array_equal(bad.indptr, P.indptr) and np.array_equal(bad.indices, P.indices)
    assert (bits(bad.data) != bits(P.data)).sum() >= 3


def test_liveness_hub_rows_beyond_512(oracle):
    """Reading only the first 512 entries of a row changes P in the 513- and 600-entry hub rows
    and in no other hub row."""
    A, S, cf, P = _restated_level0(oracle, "hub")
    assert same_bits(_interp_variant(A, S, cf), P)
    bad = _interp_variant(A, S, cf, truncate=E.K_IW_MAX)
    lengths = E.zoo()["hub"].claims["lengths"]
    for h, length in enumerate(lengths):
        same = (bad.indptr[h + 1] - bad.indptr[h] == P.indptr[h + 1] - P.indptr[h]
                and np.array_equal(bits(bad.data[bad.indptr[h]:bad.indptr[h + 1]]), bits(P.data[P.indptr[h]:P.indptr[h + 1]])))
        assert same == (length <= E.K_IW_MAX), (h, length)


def test_liveness_spgemm_order(oracle):
    """Reversing the k loop changes the bits of every order-sensitive row, and of no other.  Of
    the six orders of the three k steps, only the canonical one and the one that swaps its
    first two steps -- the same sum, since a + b == b + a in floating point and the accumulator
    starts at +0.0 -- give the canonical bits: every other order changes every column of every
    such row."""
    import itertools

    p = E.pairs()["row_bins"]
    C = reference_product(oracle, "row_bins")
    for perm in [None] + list(itertools.permutations(range(3))):
        bad = E.canonical_product(p.A, p.B, reverse_k=perm is None, k_perm=perm)
        assert np.array_equal(bad.indptr, C.indptr) and np.array_equal(bad.indices, C.indices)
        diff = bits(bad.data) != bits(C.data)
        if perm in ((0, 1, 2), (1, 0, 2)):
            assert not diff.any(), perm
            continue
        rows = np.unique(np.searchsorted(C.indptr, np.flatnonzero(diff), side="right") - 1)
        assert rows.tolist() == p.claims["order_rows"], perm
        for i in rows:
            assert diff[C.indptr[i]:C.indptr[i + 1]].all()
