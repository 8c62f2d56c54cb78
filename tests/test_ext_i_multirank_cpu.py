"""Extended+i interpolation on several ranks, host path, over gloo on the CPU (world sizes 2 and
3, ragged cuts): every rank's slice of A, P, R and the split on every level, and the coarse
inverse, equal the serial oracle's -- extended+i depends on global ids and each row's own order
only, so the serial oracle is the reference at every rank count.  The states two halos deep
(tests/ext_i_cases.py two_deep) travel through the second halo plan."""
import os
import socket
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _cases(O, ws):
    """(name, scipy A, pmis options, p_max, drop_tol, cuts)"""
    import scipy.sparse as sp

    from tests import ext_i_cases as X
    from tests import setup_edge_cases as E

    def ragged(n):
        cuts = [0] + [n * (r + 1) // ws - (5 * (ws - 1 - r)) for r in range(ws)]
        return cuts[:-1]

    out = []
    dflt = dict(strong_threshold=0.25, max_coarse=32)
    for name, A, p_max, tol in (("7pt p4", O.gen_7pt(14, 13, 12), 4, 0.0), ("7pt p0", O.gen_7pt(14, 13, 12), 0, 0.0),
                                ("27pt", O.gen_27pt(11, 10, 12), 4, 0.0), ("7pt drop", O.gen_7pt(14, 13, 12), 4, 0.02)):
        M = sp.csr_matrix(A.to_scipy())
        out.append((name, M, dflt, p_max, tol, ragged(M.shape[0])))
    for name in ("mixed_600", "hub", "sk_zero", "negative_diagonal"):
        c = E.zoo()[name]
        out.append((name, c.A, c.pmis, 4, 0.0, c.cuts[ws]))
    for name, c in X.cases().items():
        out.append((name, c.A, c.pmis, 4, 0.0, c.cuts[ws]))
    return out


def _worker(rank, ws, port, q):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=ws)
    try:
        from oracle import oracle as O
        from raptor_amd import host
        from tests.setup_edge_cases import bits

        fails = []
        for name, M, opts, p_max, tol, cuts in _cases(O, ws):
            n = M.shape[0]
            b = list(cuts) + [n]
            lo, hi = b[rank], b[rank + 1]
            Ml = M[lo:hi]
            Hp = host.HostHierarchy(n, lo, Ml.indptr, Ml.indices, Ml.data,
                                    host.options(coarsen="pmis", interp="ext+i", p_max=p_max, drop_tol=tol, **opts),
                                    rank=rank, nranks=ws, group=dist.group.WORLD)
            Ao = O.Csr.from_arrays(n, n, M.indptr, M.indices, M.data)
            Ho = O.Hierarchy(Ao, interp=O.INTERP_EXT_I, p_max=p_max, drop_tol=tol, **opts)
            if Hp.num_levels != Ho.num_levels:
                fails.append((name, "levels", Hp.num_levels, Ho.num_levels))
                continue
            for l in range(Ho.num_levels):
                for w in "APR":
                    if w != "A" and l == Ho.num_levels - 1:
                        continue
                    P = Hp.to_scipy(l, w)
                    f = Hp.sizes(l, w)["first_row"]
                    G = Ho.matrix(l, w)[f:f + P.shape[0]]
                    if not (np.array_equal(P.indptr, G.indptr) and np.array_equal(P.indices, G.indices)
                            and np.array_equal(bits(P.data), bits(G.data))):
                        fails.append((name, l, w))
                if l + 1 < Ho.num_levels:
                    f = Hp.sizes(l, "A")["first_row"]
                    s = Hp.split(l)
                    if not np.array_equal(s, Ho.split(l)[f:f + s.size]):
                        fails.append((name, l, "split"))
            inv = O.dense_inverse(O.Csr.from_scipy(Ho.matrix(Ho.num_levels - 1, "A")))
            if not np.array_equal(bits(Hp.coarse_inverse()), bits(inv)):
                fails.append((name, "inverse"))
        q.put((rank, fails))
    except Exception as e:  # report, do not hang the parent
        q.put((rank, [repr(e)]))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("ws", [2, 3])
def test_ext_i_multirank_setup_matches_serial_oracle(oracle, ws):
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, ws, port, q)) for r in range(ws)]
    for p in procs:
        p.start()
    res = [q.get(timeout=600) for _ in range(ws)]
    for p in procs:
        p.join(timeout=60)
    for rank, fails in res:
        assert fails == [], (rank, fails)
