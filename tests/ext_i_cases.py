"""Operators on the limits of the device extended+i interpolation (setup_device.hip
interp_ext_kernel): the capacity of the per-wave candidate set, the P_max boundary, the weak
entry that joins the numerator, the two arms of the a_ki lookup and the two-deep state halo.

Plain numpy / scipy, in the manner of tests/setup_edge_cases.py: every builder returns a Case
whose claims tests/test_ext_i_cases_cpu.py proves with the CPU oracle; the multi-rank host test
and the device test then run the same operators.

The gadget.  A hub row h couples with -1 to p points f_1..f_p and to q points c directly; every
f_k couples with -1 to r points c; every c has two leaves coupled with -1 in both directions.
The couplings back (f -> h, c -> f, c -> h) are -1/16: weak at theta = 1/4.  So nothing depends
on h (pmis_init marks it F), a c has its leaves and the f's as dependents and the largest
measure of its neighbourhood (C in round one), and the f's and leaves turn F.  C^_h is then the
q direct points and the distinct c's of the f's: the builder chooses how many those are.
Values carry a seeded factor in [0.9, 1.1], which moves no entry across the threshold."""
from __future__ import annotations

import functools

import numpy as np
import scipy.sparse as sp

from tests.setup_edge_cases import Case, _from_coo, _with_dominant_diagonal

K_EXT_CAP = 256   # setup_device.hip kExtCap: members of C^_i (and strong neighbours) a wave holds in LDS
P_MAX = 4
THETA = 0.25


class _Builder:
    def __init__(self, seed):
        self.rng = np.random.Generator(np.random.PCG64(seed))
        self.I, self.J, self.V = [], [], []
        self.hubs, self.fs, self.cs = [], [], []   # per gadget: ids within their class
        self.nf = self.nc = 0

    def gadget(self, p, r, q, pool=None, weak_to_far_c=False, back=None):
        """One hub with p strong F neighbours of r C points each (drawn round-robin from a pool
        of `pool` points when given, else all distinct) and q direct C points.  back[k]: the
        value of a_{f_k, h} (default -1/16)."""
        f = list(range(self.nf, self.nf + p))
        self.nf += p
        nfar = pool if pool is not None else p * r
        far = list(range(self.nc, self.nc + nfar))
        direct = list(range(self.nc + nfar, self.nc + nfar + q))
        self.nc += nfar + q
        self.hubs.append(dict(f=f, far=far, direct=direct, r=r, weak=weak_to_far_c, back=back or {}))
        return len(self.hubs) - 1

    def build(self):
        nh = len(self.hubs)
        f0, c0 = nh, nh + self.nf
        l0 = c0 + self.nc
        n = l0 + 2 * self.nc
        u = lambda: self.rng.uniform(0.9, 1.1)

        def add(a, b, v):
            self.I.append(a), self.J.append(b), self.V.append(v)

        for h, g in enumerate(self.hubs):
            t = 0
            for k, fk in enumerate(g["f"]):
                add(h, f0 + fk, -1.0 * u())
                add(f0 + fk, h, g["back"].get(k, -1.0 / 16))
                for _ in range(g["r"]):
                    c = g["far"][t % len(g["far"])]
                    t += 1
                    add(f0 + fk, c0 + c, -1.0 * u())
                    add(c0 + c, f0 + fk, -1.0 / 16)
            for c in g["direct"]:
                add(h, c0 + c, -1.0 * u())
                add(c0 + c, h, -1.0 / 16)
            if g["weak"]:  # a weak entry of row h to a C point reached through f_0 only
                c = g["far"][0]
                add(h, c0 + c, -1.0 / 8)
                add(c0 + c, h, -1.0 / 16)
        for c in range(self.nc):
            for s in range(2):
                add(c0 + c, l0 + 2 * c + s, -1.0 * u())
                add(l0 + 2 * c + s, c0 + c, -1.0 * u())
        W = _from_coo(n, self.I, self.J, self.V)
        return _with_dominant_diagonal(W, 0.25), f0, c0, l0


def capacity():
    """Hubs 0, 1, 2: |C^_h| = K_EXT_CAP - 1, K_EXT_CAP, K_EXT_CAP + 1 (51 strong F neighbours of
    5 distinct C points = 255, plus 0, 1, 2 direct ones): the last set held in LDS, the full one,
    and the first row of the overflow path.  Hub 3: 60 strong F neighbours of 5 points out of a
    pool of 200: 300 candidates, 200 distinct -- the set dedupes as it gathers, so the row stays
    in LDS.  Hub 0 also stores a weak entry (-1/8) to a C point it reaches through f_0 only, and
    its f_1 couples back with +1/16: row k stores column i, but not with the selected sign."""
    b = _Builder(41)
    for q in range(3):
        b.gadget(51, 5, q, weak_to_far_c=(q == 0), back={1: 1.0 / 16} if q == 0 else None)
    b.gadget(60, 5, 0, pool=200)
    A, f0, c0, l0 = b.build()
    sizes = {0: K_EXT_CAP - 1, 1: K_EXT_CAP, 2: K_EXT_CAP + 1, 3: 200}
    cands = {3: 300}
    # rank 0: the hubs and a few f's; the other f's are ghost strong F neighbours whose C points
    # no row of rank 0 names
    return Case("ext_capacity", A, dict(chat=sizes, candidates=cands, weak_in_chat=[0], back_unselected=[(0, f0 + 1)],
                                        back_selected=[(0, f0)], f0=f0, c0=c0, l0=l0),
                pmis=dict(strong_threshold=THETA, max_coarse=16),
                cuts={2: [0, 4 + 9], 3: [0, 4 + 9, c0 + 301]})


def pmax_edge():
    """Hub 0: |C^_h| = P_MAX (one strong F neighbour of 4 points): nothing is truncated.  Hub 1:
    P_MAX + 1 (the same and one direct point): one entry goes and the rest is rescaled.  Fifty
    more pairs of the two follow so that the operator coarsens over several levels."""
    b = _Builder(43)
    for t in range(51):
        b.gadget(1, P_MAX, 0)
        b.gadget(1, P_MAX, 1)
    A, f0, c0, l0 = b.build()
    chat = {h: P_MAX + (h % 2) for h in range(102)}
    return Case("ext_pmax_edge", A, dict(chat=chat, f0=f0, c0=c0, l0=l0),
                pmis=dict(strong_threshold=THETA, max_coarse=16),
                cuts={2: [0, 57], 3: [0, 57, c0 + 203]})


@functools.lru_cache(maxsize=None)
def cases():
    cs = [capacity(), pmax_edge()]
    for c in cs:
        c.A.data.setflags(write=False)
    return {c.name: c for c in cs}


def names():
    return list(cases())


# ---- what extended+i does on a split, read off the pattern ---------------------------------------
def chat_sets(A, S, cf, rows):
    """Per row of `rows`: (C^_i as a sorted list, number of candidates with duplicates, strong F
    neighbours) from the strength pattern S and the split cf."""
    S = sp.csr_matrix(S)
    out = {}
    for i in rows:
        si = S.indices[S.indptr[i]:S.indptr[i + 1]].tolist()
        cand = [j for j in si if cf[j] == 1]
        sf = [k for k in si if cf[k] != 1]
        for k in sf:
            cand += [j for j in S.indices[S.indptr[k]:S.indptr[k + 1]].tolist() if cf[j] == 1]
        out[i] = (sorted(set(cand)), len(cand), sf)
    return out


def scratch_rows(A, S, cf, lo=0, hi=None):
    """The F rows in [lo, hi) that cannot be held in LDS: more than K_EXT_CAP members of C^_i
    or more than K_EXT_CAP strong neighbours.  The device reports how many rows it built
    through global scratch (level_ext_stats): the two must agree, which ties K_EXT_CAP to the
    kernel's constant."""
    n = sp.csr_matrix(A).shape[0]
    hi = n if hi is None else hi
    S = sp.csr_matrix(S)
    rows = [i for i in range(lo, hi) if cf[i] != 1]
    sets = chat_sets(A, S, cf, rows)
    return [i for i in rows if len(sets[i][0]) > K_EXT_CAP or S.indptr[i + 1] - S.indptr[i] > K_EXT_CAP]


def two_deep(A, S, cf, lo, hi):
    """Triples (i, k, j): local F row i in [lo, hi), ghost strong F neighbour k, strong C
    neighbour j of k that is neither local nor a column of any local row -- its state reaches
    this rank through the second halo only."""
    A, S = sp.csr_matrix(A), sp.csr_matrix(S)
    cols = set(A[lo:hi].indices.tolist())
    out = []
    for i in range(lo, hi):
        if cf[i] == 1:
            continue
        for k in S.indices[S.indptr[i]:S.indptr[i + 1]].tolist():
            if lo <= k < hi or cf[k] == 1:
                continue
            for j in S.indices[S.indptr[k]:S.indptr[k + 1]].tolist():
                if cf[j] == 1 and not lo <= j < hi and j not in cols:
                    out.append((i, k, j))
    return out
