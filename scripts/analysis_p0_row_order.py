"""Block-cut simulation for P_0's row order (segment row map): distinct x-tile
bytes of one x += P_0 e launch on the oracle's 7-pt PMIS hierarchy, for
  - rows and columns in the hierarchy's order (before the cycle order),
  - rows in grid order, columns in level 1's 8x8x8-brick order (the cycle order without a map),
  - rows in S x 8 x 8 bricks of the grid (inside a brick z, then y, then x), cut only at
    segment boundaries (S consecutive rows of one grid line), columns in brick order.
Caps: 2,048 entries, 1,024 rows (four rows per lane), 256 lines of 64 B or 512 of 32 B.
Usage: python scripts/analysis_p0_row_order.py 64   (runs the CPU oracle; analysis, not a test)"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oracle import oracle as O  # noqa: E402

N = int(sys.argv[1]) if len(sys.argv) > 1 else 64
t = time.time()
H = O.Hierarchy(O.gen_7pt(N, N, N), **O.DEFAULTS["pmis"])
print(f"7-pt {N}^3 PMIS: setup {time.time() - t:.1f} s, {H.num_levels} levels", flush=True)
P = H.matrix(0, "P")
P = P.tocsr() if hasattr(P, "tocsr") else P
n, nc = P.shape
print(f"P_0 {P.shape}, {P.nnz} entries; level-1 vector {8 * nc / 1e6:.2f} MB", flush=True)


def cut(order, colmap, LW, cap_l, unit, cap_e=2048, cap_r=1024):
    """Greedy cut of P's rows taken in `order`, `unit` rows at a time: (blocks, tile lines)."""
    ip, ix = P.indptr, colmap[P.indices]
    nb = lt = 0
    cur, ce, cr = set(), 0, 0
    for q in range(0, n, unit):
        rows = order[q:q + unit]
        ls, ne = set(), 0
        for r in rows:
            ls.update((ix[ip[r]:ip[r + 1]] // LW).tolist())
            ne += ip[r + 1] - ip[r]
        u = cur | ls
        if ce and (ce + ne > cap_e or len(u) > cap_l or cr + unit > cap_r):
            nb += 1
            lt += len(cur)
            cur, ce, cr = ls, ne, unit
        else:
            cur, ce, cr = u, ce + ne, cr + unit
    return nb + 1, lt + len(cur)


# level 1's points in 8x8x8 bricks of the fine grid (CycleOrder): old column -> new position
c1 = np.nonzero(np.asarray(H.split(0)) == 1)[0]
i, j, k = c1 % N, (c1 // N) % N, c1 // (N * N)
nb8 = (N + 7) // 8
key = ((k // 8) * nb8 + j // 8) * nb8 + i // 8
brick_cols = np.argsort(np.argsort(key, kind="stable"), kind="stable")
ident_cols = np.arange(nc)


def row_bricks(S):
    """Level-0 rows in S x 8 x 8 bricks (bricks x fastest; inside z, then y, then x)."""
    p = np.arange(n)
    i, j, k = p % N, (p // N) % N, p // (N * N)
    nbx = N // S
    key = ((((k // 8) * nb8 + j // 8) * nbx + i // S) * 8 + k % 8) * 8 + j % 8
    return np.argsort(key * S + i % S, kind="stable")


grid = np.arange(n)
rows = [("hierarchy order / hierarchy order", grid, ident_cols, 1),
        ("grid order / brick order", grid, brick_cols, 1)]
for S in (8, 16, 32):
    if N % S == 0:
        rows.append((f"{S}x8x8 row bricks, segments of {S} / brick order", row_bricks(S), brick_cols, S))
print(f"{'P_0 rows / columns':52s} {'64-byte lines':>24s} {'32-byte lines':>24s}")
for name, order, cols, unit in rows:
    out = []
    for LW, cap in ((8, 256), (4, 512)):
        nb, lt = cut(order, cols, LW, cap, unit)
        out.append(f"{nb:5d} blocks {lt * LW * 8 / 1e6:6.2f} MB")
    print(f"{name:52s} {out[0]:>24s} {out[1]:>24s}", flush=True)
