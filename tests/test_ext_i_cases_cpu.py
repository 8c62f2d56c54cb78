"""CPU side of tests/ext_i_cases.py: every claim a builder makes about its operator, proven
with the oracle's stage functions (strength_classical, pmis_split, interp_ext_i) on level 0,
and the product's one-rank host setup against the oracle's hierarchy, bit for bit."""
import numpy as np
import pytest
import scipy.sparse as sp

from tests import ext_i_cases as X
from tests.setup_edge_cases import same_bits

SEED = 0x5EED
_STAGE = {}


def _orc(O, M):
    M = sp.csr_matrix(M)
    return O.Csr.from_arrays(M.shape[0], M.shape[1], M.indptr, M.indices, M.data)


def stage0(O, name):
    if name not in _STAGE:
        c = X.cases()[name]
        Ao = _orc(O, c.A)
        S = O.strength_classical(Ao, c.pmis["strong_threshold"])
        cf = O.pmis_split(S, SEED)
        hubs = sorted(c.claims["chat"])
        _STAGE[name] = dict(Ao=Ao, S=S, Ss=S.to_scipy(), cf=cf, sets=X.chat_sets(c.A, S.to_scipy(), cf, hubs))
    return _STAGE[name]


@pytest.mark.parametrize("name", X.names())
def test_split_is_the_one_the_gadget_is_built_for(oracle, name):
    c, st = X.cases()[name], stage0(oracle, name)
    cf, f0, c0, l0 = st["cf"], c.claims["f0"], c.claims["c0"], c.claims["l0"]
    assert (cf[:c0] == 0).all(), "hubs and their strong neighbours are F"
    assert (cf[c0:l0] == 1).all(), "the points with leaves are C"
    assert (cf[l0:] == 0).all(), "leaves are F"
    assert np.isfinite(c.A.data).all() and c.A.has_sorted_indices


@pytest.mark.parametrize("name", X.names())
def test_candidate_set_sizes(oracle, name):
    """|C^_h| of every hub is what the builder states, and the untruncated oracle row has
    exactly that many entries; with P_max the row has min(|C^_h|, P_max)."""
    O = oracle
    c, st = X.cases()[name], stage0(O, name)
    P0 = O.interp_ext_i(st["Ao"], st["S"], st["cf"], 0).to_scipy()
    P4 = O.interp_ext_i(st["Ao"], st["S"], st["cf"], X.P_MAX).to_scipy()
    for h, m in c.claims["chat"].items():
        chat, ncand, sf = st["sets"][h]
        assert len(chat) == m, (h, len(chat), m)
        assert P0.indptr[h + 1] - P0.indptr[h] == m
        assert P4.indptr[h + 1] - P4.indptr[h] == min(m, X.P_MAX)
    for h, ncand in c.claims.get("candidates", {}).items():
        assert st["sets"][h][1] == ncand


def test_capacity_rows_sit_on_the_limit(oracle):
    c, st = X.cases()["ext_capacity"], stage0(oracle, "ext_capacity")
    got = sorted(len(st["sets"][h][0]) for h in (0, 1, 2))
    assert got == [X.K_EXT_CAP - 1, X.K_EXT_CAP, X.K_EXT_CAP + 1]
    chat, ncand, sf = st["sets"][3]
    assert ncand > X.K_EXT_CAP >= len(chat), "duplicates exceed the capacity, the distinct set does not"
    assert all(len(st["sets"][h][2]) <= X.K_EXT_CAP for h in range(4))


def test_rows_of_the_scratch_path(oracle):
    """ext_capacity has exactly one row over the LDS capacity (hub 2, 257 members); the hub
    operator of the setup zoo has its four rows of more than K_EXT_CAP strong neighbours
    (lengths 511 to 600) among them.  tests/test_gpu_ext_i_device.py compares these lists with the
    device's count."""
    from tests import setup_edge_cases as E

    c, st = X.cases()["ext_capacity"], stage0(oracle, "ext_capacity")
    assert X.scratch_rows(c.A, st["Ss"], st["cf"]) == [2]
    h = E.zoo()["hub"]
    S = oracle.strength_classical(_orc(oracle, h.A), h.pmis["strong_threshold"])
    cf = oracle.pmis_split(S, SEED)
    rows = X.scratch_rows(h.A, S.to_scipy(), cf)
    long_hubs = [int(i) for i, L in zip(h.claims["hubs"], h.claims["lengths"]) if L - 1 > X.K_EXT_CAP]
    assert len(long_hubs) == 4 and set(long_hubs) <= set(rows)


def test_weak_entry_inside_chat(oracle):
    """Row h stores an entry to a C point that is not strong in row h but is in C^_h through a
    strong F neighbour: a_hj joins num_j, it is not added to d."""
    c, st = X.cases()["ext_capacity"], stage0(oracle, "ext_capacity")
    A, S = c.A, st["Ss"]
    for h in c.claims["weak_in_chat"]:
        row = set(A.indices[A.indptr[h]:A.indptr[h + 1]].tolist()) - {h}
        strong = set(S.indices[S.indptr[h]:S.indptr[h + 1]].tolist())
        weak_in = [j for j in row - strong if j in set(st["sets"][h][0])]
        assert weak_in, "no weak entry inside C^_h"


def test_back_entry_arms(oracle):
    """Row k stores column i: once with the sign opposite to a_kk (selected: it enters s_k and
    d), once with the sign of a_kk (not selected)."""
    c = X.cases()["ext_capacity"]
    A = c.A
    for i, k in c.claims["back_selected"]:
        assert A[k, k] > 0 and A[k, i] < 0
    for i, k in c.claims["back_unselected"]:
        assert A[k, k] > 0 and A[k, i] > 0


def test_pmax_edge(oracle):
    c, st = X.cases()["ext_pmax_edge"], stage0(oracle, "ext_pmax_edge")
    sizes = {len(st["sets"][h][0]) for h in c.claims["chat"]}
    assert sizes == {X.P_MAX, X.P_MAX + 1}


def test_seven_point_rows_tie_at_the_truncation_boundary(oracle):
    """A constant-coefficient 7-pt operator has F rows whose P_max-th and (P_max + 1)-th largest
    |w| are equal: the tie-break (smaller column) decides what is kept."""
    O = oracle
    A = O.gen_7pt(10, 9, 8)
    S = O.strength_classical(A, 0.25)
    cf = O.pmis_split(S, SEED)
    P = O.interp_ext_i(A, S, cf, 0).to_scipy()
    ties = 0
    for i in np.flatnonzero(cf != 1):
        w = np.sort(np.abs(P.data[P.indptr[i]:P.indptr[i + 1]]))[::-1]
        ties += w.size > X.P_MAX and w[X.P_MAX - 1] == w[X.P_MAX]
    assert ties > 0


@pytest.mark.parametrize("name", X.names())
def test_second_halo_is_needed_on_every_cut(oracle, name):
    c, st = X.cases()[name], stage0(oracle, name)
    n = c.A.shape[0]
    for ws, cuts in c.cuts.items():
        b = list(cuts) + [n]
        assert len(b) == ws + 1 and all(x < y for x, y in zip(b, b[1:]))
        found = sum(len(X.two_deep(c.A, st["Ss"], st["cf"], b[r], b[r + 1])) for r in range(ws))
        assert found > 0, (name, ws)


@pytest.mark.parametrize("p_max", [4, 0])
@pytest.mark.parametrize("name", X.names())
def test_host_setup_equals_oracle(oracle, name, p_max):
    from raptor_amd import host

    O = oracle
    c = X.cases()[name]
    A = c.A
    Hp = host.HostHierarchy(A.shape[0], 0, A.indptr, A.indices, A.data,
                            host.options(coarsen="pmis", interp="ext+i", p_max=p_max, **c.pmis))
    Ho = O.Hierarchy(_orc(O, A), interp=O.INTERP_EXT_I, p_max=p_max, **c.pmis)
    assert Hp.num_levels == Ho.num_levels >= 2
    for l in range(Ho.num_levels):
        for w in "APR":
            if w != "A" and l == Ho.num_levels - 1:
                continue
            assert np.isfinite(Ho.matrix(l, w).data).all()
            assert same_bits(Hp.to_scipy(l, w), Ho.matrix(l, w)), (name, l, w)
        if l + 1 < Ho.num_levels:
            assert np.array_equal(Hp.split(l), Ho.split(l))
